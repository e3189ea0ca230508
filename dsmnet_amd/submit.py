"""A named dataset through a model, results to files (the reference's ``submit()``, stereo.py:115-187).

    model = model_create_by_name("psmnet", 192); deploy.load_weights(model, "weight_best.pkl")
    dataset = dataset_stereo_by_name("kitti2015-te", root, Train=False)
    submit(model.cuda(), dataset, "submit/kitti2015-te_psmnet", pad_multiple=16, formats=("u16", "viridis"))

    python -m dsmnet_amd.submit --net psmnet --path_weight weight_best.pkl --dataset kitti2015-te \\
        --root ./kitti --out submit/kitti2015-te_psmnet --format u16 --format viridis

The forward's map never reaches the host as fp32: ``costvolume.encode_disparity`` turns it into the files'
bytes on the device (csrc/encode.hip), ``ResultWriter`` copies those to pinned memory without blocking
and hands PNG compression to worker threads.

Files: ``<dirpath_save>/<format>/<filename stem>.png``, one subfolder per requested format:

    u16      16-bit gray, KITTI's encoding: value * 256, 0 = invalid.  What the KITTI server takes and what
             ``Dataset_stereo(disp_png="kitti")`` reads back as value / 256.
    u8       8-bit gray, ``clip(rint(d), 0, 255)``: what the reference's ``cv2.imwrite`` of the float map writes
    viridis  RGB, viridis over ``vrange``, or over each image's own range (``plt.imsave``'s picture)
    error    RGB, the KITTI devkit's log-scale error picture; needs a dataset with ground truth

and ``<dirpath_save>.pkl``: ``{"filename", "time", "D1", "epe"}``, lists with one entry per file (``D1`` and
``epe`` empty without ground truth), written with ``torch.save`` and read with ``weights_only=True``.
"""
import argparse
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import transforms

MAX_THREADS = 16
FORMATS = {"u16": "u16", "u8": "u8", "viridis": "rgb", "error": "err"}      # format -> encode_disparity's name


def write_png(path, image):
    if image.dtype == np.uint16:
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(image)).save(path)          # mode I;16
    else:
        from .img_rw import imwrite
        imwrite(path, image)


class ResultWriter(object):
    """Encoded maps to PNG files under ``dirpath``, off the thread that feeds the GPU.

    ``write(encoded, filenames)``: ``encoded`` maps a subfolder name to a (B,h,w) uint16 / uint8 or
    (B,h,w,3) uint8 batch, ``filenames`` are the B file names inside every subfolder.  Device tensors are
    copied with ``non_blocking=True`` into one of two sets of pinned buffers; the set's event is recorded
    behind the copies and the workers wait on it, so the calling thread does not wait for the GPU.  A set
    is written again only when its previous copies have landed and its previous files are on disk.
    Host arrays (numpy, CPU tensors) go to the workers as they are.  At most ``4 * threads`` files wait
    in the queue: ``write`` blocks beyond that.  ``close()`` joins the pool and re-raises the first
    error a worker met; the writer is a context manager that closes itself."""

    def __init__(self, dirpath, threads=4):
        self.dirpath = dirpath
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self._pool = ThreadPoolExecutor(max_workers=self.threads)
        self._slots = threading.BoundedSemaphore(4 * self.threads)
        self._error = None
        self._lock = threading.Lock()
        self._stage = [{}, {}]               # per set: name -> pinned buffer
        self._event = [None, None]           # per set: recorded behind its copies
        self._pending = [[], []]             # per set: the futures that read it
        self._turn = 0
        self._dirs = set()
        if not os.path.isdir(dirpath):
            os.makedirs(dirpath)

    def _job(self, path, image, event):
        try:
            if event is not None:
                event.synchronize()
            write_png(path, image)
        except BaseException as err:         # kept for close()
            with self._lock:
                if self._error is None:
                    self._error = err
        finally:
            self._slots.release()

    def _submit(self, path, image, event=None):
        self._slots.acquire()
        try:
            return self._pool.submit(self._job, path, image, event)
        except BaseException:
            self._slots.release()
            raise

    def write(self, encoded, filenames):
        filenames = list(filenames)
        device = [n for n, t in encoded.items() if torch.is_tensor(t) and t.is_cuda]
        k = self._turn
        event = None
        if device:
            self._turn ^= 1
            # State that outlives a launch: set k's buffers are read by its copies' consumers.
            for f in self._pending[k]:
                f.result()
            self._pending[k] = []
            if self._event[k] is not None:
                self._event[k].synchronize()
        host = {}
        for name, t in encoded.items():
            if len(t) != len(filenames):
                raise ValueError("ResultWriter: %s holds %d images for %d file names" % (name, len(t), len(filenames)))
            if name in device:
                view = t.view(torch.int16) if t.dtype == torch.uint16 else t     # the same bytes
                buf = self._stage[k].get(name)
                if buf is None or buf.numel() < view.numel() or buf.dtype != view.dtype:
                    buf = self._stage[k][name] = torch.empty(view.numel(), dtype=view.dtype, pin_memory=True)
                stage = buf[:view.numel()].view(view.shape)
                stage.copy_(view, non_blocking=True)
                arr = stage.numpy()
                host[name] = arr.view(np.uint16) if t.dtype == torch.uint16 else arr
            else:
                host[name] = t.numpy() if torch.is_tensor(t) else np.asarray(t)
            sub = os.path.join(self.dirpath, name)
            if sub not in self._dirs:
                if not os.path.isdir(sub):
                    os.makedirs(sub)
                self._dirs.add(sub)
        if device:
            event = self._event[k] = torch.cuda.Event()
            event.record()
        for name, arr in host.items():
            for i, fname in enumerate(filenames):
                path = os.path.join(self.dirpath, name, os.path.splitext(os.path.basename(fname))[0] + ".png")
                f = self._submit(path, arr[i], event if name in device else None)
                if name in device:
                    self._pending[k].append(f)

    def close(self):
        self._pool.shutdown(wait=True)
        err, self._error = self._error, None
        if err is not None:
            raise err

    def __enter__(self):
        return self

    def __exit__(self, kind, value, tb):
        if kind is None:
            self.close()
        else:                                # the caller's error wins
            self._pool.shutdown(wait=True)
        return False


def _print_results(data):
    """stereo.py:130-136 / 184-187: the per-file lines, then the means."""
    names, times, D1s, epes = data["filename"], data["time"], data["D1"], data["epe"]
    scored = len(D1s) == len(names) and len(names) > 0
    for i, name in enumerate(names):
        if scored:
            print("submit: %s | time: %6.3f, D1: %6.3f, epe: %6.3f" % (name, times[i], D1s[i], epes[i]))
        else:
            print("submit: %s | time: %6.3f" % (name, times[i]))
    if scored:
        print(np.mean(times), np.mean(D1s), np.mean(epes))
    elif names:
        print(np.mean(times))


def _pad_sizes(H, W, multiple):
    if not multiple:
        return 0, 0
    return -H % int(multiple), -W % int(multiple)


def submit(model, dataset, dirpath_save, batch_size=1, pad_multiple=None, formats=("u16",), vrange=None,
           lr_check=False, augment=transforms.Stereo_normalize(), threads=4, speckle=None):
    """Every file of ``dataset`` through ``model``; results under ``dirpath_save`` as the module text says.

    ``dataset``: a ``Dataset_stereo`` (``dataset_stereo_by_name(..., Train=False)``); its transform is not
    used: ``DeviceLoader`` builds ``Stereo_ToTensor`` batches on the device and ``augment`` (the
    reference's choice: ImageNet normalisation) is applied to the copy the network sees, as in
    ``train.evaluate_step``.  ``pad_multiple``: the images are padded with zeros at the top and on the
    right (``F.pad``) to multiples of it, and the encoder's window cuts the padding off the results.
    With ground truth (a 7-channel dataset) each file's D1 / EPE come from ``costvolume.stereo_metrics``
    over the un-padded map, one host read per batch.  ``vrange``: viridis' fixed range; None: each image's
    own.  ``lr_check=True``: both views are predicted (``postprocess.left_right_check``) and the pixels the
    check rejects are 0 in ``u16`` and ``u8`` and black in the pictures.  ``speckle=(max_size, max_diff)``:
    the connected regions of at most ``max_size`` pixels (``costvolume.filter_speckles``) are rejected in the
    same way -- alone, of the predicted map; with ``lr_check``, among the consistent pixels
    (``left_right_check(speckle=)``).  The regions are those of the frame the network saw, padding included.

    When ``<dirpath_save>.pkl`` exists, its lines are printed and nothing runs (stereo.py:124-137).
    Returns the saved dict.  ``time``: the wall time of the file's batch, loading included, over its size."""
    from . import costvolume as cv
    from .datasets import DeviceLoader
    formats = tuple(formats)
    if not formats or any(f not in FORMATS for f in formats) or len(set(formats)) != len(formats):
        raise ValueError("submit: formats is a non-empty subset of %s, got %r" % (tuple(FORMATS), formats))
    filepath_save = dirpath_save.rstrip("/\\") + ".pkl"
    if os.path.exists(filepath_save):
        data = torch.load(filepath_save, map_location="cpu", weights_only=True)
        _print_results(data)
        return data
    if "error" in formats and dataset.channels < 7:
        raise ValueError("submit: the error picture needs a dataset with ground truth")
    names, times, D1s, epes = [], [], [], []
    loader = DeviceLoader(dataset, transforms.Stereo_ToTensor(), batch_size, threads=threads)
    want = tuple(FORMATS[f] for f in formats)
    model.eval()
    with ResultWriter(dirpath_save, threads) as writer:
        time_end = time.time()
        for batch, filenames in loader:
            B, C, H, W = batch.shape
            seen = batch[:, :6]
            if augment is not None:
                seen = augment(seen.clone())
            up, right = _pad_sizes(H, W, pad_multiple)
            if up or right:
                seen = torch.nn.functional.pad(seen, (0, right, up, 0))
            gt = batch[:, 6:7] if C >= 7 else None
            mask = None
            with torch.no_grad():
                if lr_check:
                    from .postprocess import left_right_check
                    res = left_right_check(model, seen[:, :3].contiguous(), seen[:, 3:6].contiguous(), fill=False,
                                           speckle=speckle)
                    disp, mask = res["dispL"], res["maskL" if speckle is None else "keepL"]
                else:
                    with cv.amax_scope(batch.device):
                        disp = model(seen[:, :3], seen[:, 3:6])[1][0]
                    if speckle is not None:
                        mask = cv.filter_speckles(disp, speckle[0], speckle[1], want=("keep",)).keep
                gt_frame = gt
                if gt is not None and (up or right) and "err" in want:
                    gt_frame = torch.nn.functional.pad(gt, (0, right, up, 0))
                if gt_frame is not None and disp.dim() == 3:
                    gt_frame = gt_frame[:, 0]
                encoded = cv.encode_disparity(disp, gt=gt_frame if "err" in want else None, mask=mask,
                                              window=(up, 0, H, W), want=want, vrange=vrange)
                scores = None
                if gt is not None:
                    d = disp if disp.dim() == 4 else disp.unsqueeze(1)
                    sums = cv.stereo_metrics(d[:, :, up:up + H, :W], gt)
                    m = cv.stereo_metrics_finish(sums, per_image=True)
                    scores = torch.stack([m["d1"], m["epe"]])
            writer.write({f: encoded[FORMATS[f]] for f in formats}, filenames)
            if scores is not None:
                scores = scores.cpu().tolist()                 # the batch's one host read
            else:
                torch.cuda.current_stream().synchronize()      # `time` is the batch's, not the enqueue's
            now = time.time()
            for i, name in enumerate(filenames):
                names.append(name)
                times.append((now - time_end) / len(filenames))
                if scores is not None:
                    D1s.append(scores[0][i])
                    epes.append(scores[1][i])
                    print("submit: %s | time: %6.3f, D1: %6.3f, epe: %6.3f" % (name, times[-1], D1s[-1], epes[-1]))
                else:
                    print("submit: %s | time: %6.3f" % (name, times[-1]))
            time_end = now
    data = {"filename": names, "time": times, "D1": D1s, "epe": epes}
    torch.save(data, filepath_save)
    if D1s:
        print(np.mean(times), np.mean(D1s), np.mean(epes))
    elif names:
        print(np.mean(times))
    return data


def build_parser():
    ap = argparse.ArgumentParser(description="run a stereo dataset through a model and write the results (MI355X)")
    ap.add_argument("--net", default="psmnet", type=str, help="dispnet / dispnetcorr / iresnet / gcnet / psmnet")
    ap.add_argument("--maxdisparity", default=192, type=int)
    ap.add_argument("--path_weight", default="", type=str)
    ap.add_argument("--dataset", default="kitti2015-te", type=str, help="'_'-separated dataset names")
    ap.add_argument("--root", default="./kitti", type=str)
    ap.add_argument("--out", default=None, type=str, help="default submit/<dataset>_<net>")
    ap.add_argument("--format", action="append", choices=sorted(FORMATS), default=None,
                    help="may be given several times; default u16")
    ap.add_argument("--vrange", nargs=2, type=float, default=None, metavar=("LO", "HI"),
                    help="viridis' fixed range (default: each image's own)")
    ap.add_argument("--batch_size", default=1, type=int)
    ap.add_argument("--pad_multiple", default=64, type=int, help="pad top / right to multiples of this (0: no padding)")
    ap.add_argument("--lr_check", action="store_true", help="predict both views and zero the inconsistent pixels")
    ap.add_argument("--speckle", nargs=2, type=float, default=None, metavar=("SIZE", "DIFF"),
                    help="zero the connected regions of at most SIZE pixels, neighbours joined where they differ by at "
                         "most DIFF (OpenCV's filterSpeckles); with --lr_check among the consistent pixels")
    ap.add_argument("--threads", default=4, type=int, help="decoding and PNG-writing threads (at most 16)")
    return ap


def main(argv=None):
    from .datasets import dataset_stereo_by_name
    from .deploy import load_weights, speckle_args
    from .models import model_create_by_name
    args = build_parser().parse_args(argv)
    speckle = speckle_args(args.speckle)
    if not torch.cuda.is_available():
        raise SystemExit("dsmnet_amd.submit needs an MI355X: the HIP path has no CPU fallback")
    out = args.out or os.path.join("submit", "%s_%s" % (args.dataset, args.net))
    dataset = dataset_stereo_by_name(args.dataset, args.root, Train=False)
    model = model_create_by_name(args.net, args.maxdisparity)
    load_weights(model, args.path_weight)
    submit(model.eval().cuda(), dataset, out, batch_size=args.batch_size, pad_multiple=args.pad_multiple or None,
           formats=tuple(args.format or ("u16",)), vrange=args.vrange, lr_check=args.lr_check, threads=args.threads,
           speckle=speckle)
    return out


if __name__ == "__main__":
    main()
