"""Single-pair inference with reference-format weights.

Mirrors deploy/deploy.py:15-32 (``disp_predict``) and :49-73 (the command line), the checkpoint
wire format of stereo.py:57-92 / utils/utils.py:31-53 (``{'epoch','best_prec','state_dict',
'optim'}`` saved with ``torch.save``; weights-only files ``{'state_dict': ...}``), and the
normalisation transform of myTransforms (``__init__.py:8,121-124``, ``aug_color.py:28-45``).

    python -m dsmnet_amd.deploy --net psmnet --path_weight weight_best.pkl \\
        --path_left 10L.png --path_right 10R.png

Checkpoints are read with ``torch.load(..., weights_only=True)`` only: nothing in the file is
executed.  A file the safe loader refuses is reported, never unpickled.
"""
import argparse
import os
import shutil

import numpy as np
import torch

IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]


class Normalize(object):
    """myTransforms/aug_color.py:28-45, in place, on a (3*g, H, W) tensor.

    ``group = min(self.group, img.shape[0] // 3)`` -- so a batched (1,3,H,W) tensor, which is
    what ``disp_predict`` passes, has ``1 // 3 == 0`` groups and comes back UNnormalised.  That
    is the reference's behaviour, weights trained and deployed with it expect it, and it is
    kept."""

    def __init__(self, mean, std, group=1):
        assert len(mean) == 3 and len(std) == 3
        self.group, self.mean, self.std = group, mean, std

    def __call__(self, img):
        group = min(self.group, img.shape[0] // 3)
        for grp in range(group):
            idx = grp * 3
            for i in range(3):
                if self.mean[i] != 0:
                    img[idx + i] -= self.mean[i]
                if self.std[i] != 1:
                    img[idx + i] /= self.std[i]
        return img


def Stereo_normalize():
    """myTransforms/__init__.py:121-124: ImageNet normalisation of a 6-channel L|R stack."""
    return Normalize(IMAGENET_MEAN, IMAGENET_STD, group=2)


# ----------------------------------------------------------------------------
# checkpoint wire format
# ----------------------------------------------------------------------------
def _safe_load(path):
    try:
        return torch.load(path, map_location="cpu", weights_only=True)
    except Exception as first:
        try:                                    # Python-2 pickles: byte strings are latin-1
            return torch.load(path, map_location="cpu", weights_only=True, encoding="latin1")
        except Exception:
            raise RuntimeError("%s was refused by the weights-only loader (%s); it is not "
                               "unpickled any other way" % (path, first))


def load_state(path):
    """The whole checkpoint dict (``state_dict`` plus, for training checkpoints, ``epoch``,
    ``best_prec``, ``optim``)."""
    state = _safe_load(path)
    if not isinstance(state, dict) or "state_dict" not in state:
        raise ValueError("%s is not a reference-format checkpoint: no 'state_dict' entry" % path)
    return state


def load_weights(model, path, strict=True):
    """``model.load_state_dict(torch.load(path)['state_dict'])`` (stereo.py:61-62,
    deploy.py:51-52).  A ``module.`` prefix left by ``nn.DataParallel`` is stripped."""
    sd = load_state(path)["state_dict"]
    if sd and all(k.startswith("module.") for k in sd):
        sd = {k[len("module."):]: v for k, v in sd.items()}
    model.load_state_dict(sd, strict=strict)
    return model


def save_checkpoint(state, is_best, dirpath="./output", filename="model_checkpoint.pkl"):
    """utils/utils.py:31-43: write to ``<file>.tmp``, move into place, copy to
    ``model_best.pkl`` when ``is_best``."""
    if not os.path.exists(dirpath):
        os.makedirs(dirpath)
    path = os.path.join(dirpath, filename)
    torch.save(state, path + ".tmp")
    shutil.move(path + ".tmp", path)
    if is_best:
        shutil.copyfile(path, os.path.join(dirpath, "model_best.pkl"))
    return path


def load_checkpoint(dirpath="./output", best=False):
    """utils/utils.py:46-53: ``None`` when the file does not exist."""
    path = os.path.join(dirpath, "model_best.pkl" if best else "model_checkpoint.pkl")
    if not os.path.exists(path):
        return None
    return load_state(path)


# ----------------------------------------------------------------------------
# prediction
# ----------------------------------------------------------------------------
def disp_predict(model, imgL_np, imgR_np, use_cuda=None):
    """deploy/deploy.py:15-32: (H,W,3) uint8/float RGB arrays -> (H,W) float32 disparity, the
    first of the model's outputs.  ``use_cuda=None``: wherever the model's parameters live."""
    if use_cuda is None:
        use_cuda = next(model.parameters()).is_cuda
    imgL = torch.from_numpy(imgL_np.copy().transpose(2, 0, 1)[None]).float()
    imgR = torch.from_numpy(imgR_np.copy().transpose(2, 0, 1)[None]).float()
    if use_cuda:
        imgL, imgR = imgL.cuda(), imgR.cuda()
    transform = Stereo_normalize()
    imgL = transform(imgL / 255.0)
    imgR = transform(imgR / 255.0)
    with torch.no_grad():
        _, disps = model(imgL, imgR, mode="test")
    d = disps[0]            # (B,1,H,W) for DispNetC / iResNet / GCNet; PSMNet returns (B,H,W), where the
    d = d[0, 0] if d.dim() == 4 else d[0]      # reference's `disps[0][0, 0]` would keep one row only
    return d.detach().cpu().numpy()


def evaluate_pair(imgL_np, imgR_np, disp, path_disp_gt, flip=False):
    """(d1, epe, pixelerror) of a predicted (H,W) disparity against the ground-truth file (PFM or PNG,
    read by ``img_rw.load_disp``; holes <= 0): ``dsmnet_amd.evaluate.evaluate`` on the raw [0,1]
    images.  ``flip``: ``disp`` is the right view's -- the pair is mirrored and swapped back into the
    frame it was predicted in, the ground truth with it."""
    from .evaluate import evaluate
    from .img_rw import load_disp
    gt = np.asarray(load_disp(path_disp_gt), dtype=np.float32)
    if flip:
        imgL_np, imgR_np = np.flip(imgR_np, axis=1), np.flip(imgL_np, axis=1)
        disp, gt = np.flip(disp, axis=-1), np.flip(gt, axis=-1)
    if gt.shape != disp.shape:
        raise ValueError("ground truth %s does not match the prediction %s" % (gt.shape, disp.shape))
    chw = lambda im: np.ascontiguousarray(im, dtype=np.float32).transpose(2, 0, 1)[None] / 255.0
    return evaluate(chw(imgL_np), chw(imgR_np), np.ascontiguousarray(disp, dtype=np.float32)[None, None],
                    np.ascontiguousarray(gt)[None, None])


def lr_predict(model, imgL_np, imgR_np, threshold=1.0, fill=False, speckle=None):
    """``disp_predict`` of both views with the left-right check (``postprocess.left_right_check``): the
    images go through the same preparation; the dict's (H,W) maps come back as numpy arrays, masks as bool.
    ``speckle=(max_size, max_diff)``: as there (``keepL`` / ``keepR``, the fill from ``keep``)."""
    from .postprocess import left_right_check
    transform = Stereo_normalize()
    prep = lambda im: transform(torch.from_numpy(im.copy().transpose(2, 0, 1)[None]).float().cuda() / 255.0)
    res = left_right_check(model, prep(imgL_np), prep(imgR_np), threshold=threshold, fill=fill, speckle=speckle)
    return {k: (v[0, 0] if v.dim() == 4 else v[0]).cpu().numpy() for k, v in res.items()}


def speckle_filter(disp, max_size, max_diff):
    """An (H,W) float32 map through ``postprocess.remove_speckles`` on the device: ``(out, keep)`` as numpy
    arrays, ``out`` with the removed (and the non-finite) pixels 0, ``keep`` bool."""
    from .postprocess import remove_speckles
    d = torch.from_numpy(np.ascontiguousarray(disp, dtype=np.float32))[None].cuda()
    out, keep = remove_speckles(d, max_size, max_diff)
    return out[0].cpu().numpy(), keep[0].cpu().numpy()


def speckle_args(pair):
    """``--speckle SIZE DIFF`` as ``(int, float)`` or None; ``SystemExit`` for values the filter refuses."""
    if pair is None:
        return None
    size, diff = pair
    if not (size >= 0 and size == int(size) and size < 2 ** 31):
        raise SystemExit("--speckle SIZE is a whole number of pixels >= 0, got %r" % (size,))
    if not (0.0 <= diff <= 3.402823466e38):
        raise SystemExit("--speckle DIFF is a finite disparity difference >= 0, got %r" % (diff,))
    return int(size), float(diff)


def conf_predict(model, imgL_np, imgR_np, radius=4):
    """``disp_predict`` with the cost head's confidence (``postprocess.predict_confidence``): the images go
    through the same preparation; ``disp``, ``peak``, ``pmax``, ``pwin`` and ``entropy`` come back as (H,W)
    numpy arrays."""
    from .postprocess import predict_confidence
    transform = Stereo_normalize()
    prep = lambda im: transform(torch.from_numpy(im.copy().transpose(2, 0, 1)[None]).float().cuda() / 255.0)
    res = predict_confidence(model, prep(imgL_np), prep(imgR_np), radius=radius)
    return {k: (v[0, 0] if v.dim() == 4 else v[0]).cpu().numpy() for k, v in res.items()}


def evaluate_consistent(imgL_np, imgR_np, disp, mask, path_disp_gt, flip=False):
    """``evaluate_pair`` over the consistent pixels only: the ground truth is zeroed (a hole) where ``mask``
    is false.  ``disp`` / ``mask`` / the file are the predicted view's, as for ``evaluate_pair``."""
    from .evaluate import evaluate
    from .img_rw import load_disp
    gt = np.asarray(load_disp(path_disp_gt), dtype=np.float32)
    if gt.shape != disp.shape:
        raise ValueError("ground truth %s does not match the prediction %s" % (gt.shape, disp.shape))
    gt = np.where(mask, gt, np.float32(0))
    if flip:
        imgL_np, imgR_np = np.flip(imgR_np, axis=1), np.flip(imgL_np, axis=1)
        disp, gt = np.flip(disp, axis=-1), np.flip(gt, axis=-1)
    chw = lambda im: np.ascontiguousarray(im, dtype=np.float32).transpose(2, 0, 1)[None] / 255.0
    return evaluate(chw(imgL_np), chw(imgR_np), np.ascontiguousarray(disp, dtype=np.float32)[None, None],
                    np.ascontiguousarray(gt)[None, None])


def build_parser():
    ap = argparse.ArgumentParser(description="stereo matching, single pair (MI355X)")
    ap.add_argument("--net", default="dispnetcorr", type=str,
                    help="dispnet / dispnetcorr / iresnet / gcnet / psmnet")
    ap.add_argument("--maxdisparity", default=192, type=int)
    ap.add_argument("--path_weight", default="", type=str)
    ap.add_argument("--path_left", default="10L.png", type=str)
    ap.add_argument("--path_right", default="10R.png", type=str)
    ap.add_argument("--flip", default=False, type=bool,
                    help="predict the right view's disparity (mirror both images, swap them)")
    ap.add_argument("--out", default=None, type=str, help="default dispL.png / dispR.png")
    ap.add_argument("--path_disp_gt", default=None, type=str,
                    help="ground-truth disparity of the predicted view (PFM or PNG): print D1, EPE and "
                         "the photometric error (utils/evaluate.py evaluate)")
    ap.add_argument("--lr_check", action="store_true",
                    help="predict both views, check them against each other and write <stem>_mask.png "
                         "next to the disparity (white: consistent)")
    ap.add_argument("--lr_threshold", default=1.0, type=float,
                    help="largest left-right disagreement of a consistent pixel, in pixels")
    ap.add_argument("--fill", action="store_true",
                    help="with --lr_check: write the disparity with the inconsistent pixels filled from "
                         "the background")
    ap.add_argument("--speckle", nargs=2, type=float, default=None, metavar=("SIZE", "DIFF"),
                    help="remove the connected regions of at most SIZE pixels, neighbours being joined where they "
                         "differ by at most DIFF (OpenCV's filterSpeckles; costvolume.filter_speckles).  With "
                         "--lr_check: among the consistent pixels, and --fill, --encode, the mask picture and the "
                         "consistent-pixel scores use what is kept.  Without: the written map is filtered alone, "
                         "the removed pixels are 0 (invalid for --encode).  With --peak, or --confidence without "
                         "--lr_check, it is that forward's written map that is filtered; the confidence picture "
                         "and --conf_threshold's scores are never filtered")
    ap.add_argument("--confidence", action="store_true",
                    help="psmnet / gcnet: write <stem>_conf.png next to the disparity, the probability mass of "
                         "the window around the cost head's arg-max bin as 8-bit gray (white: confident)")
    ap.add_argument("--peak", action="store_true",
                    help="psmnet / gcnet: write the peak-window disparity (the regression over the window around "
                         "the arg-max bin) in place of the expectation over the whole range")
    ap.add_argument("--conf_radius", default=4, type=int, help="half-width of that window, in disparity bins")
    ap.add_argument("--conf_threshold", default=None, type=float,
                    help="with --confidence and --path_disp_gt: also print D1 / EPE over the pixels whose window "
                         "mass is at least this, and their share")
    ap.add_argument("--encode", default=None, choices=("kitti16", "u8", "viridis"),
                    help="write the disparity PNG from the device encoder (costvolume.encode_disparity): kitti16 = "
                         "16-bit value * 256 with 0 invalid (with --lr_check the inconsistent pixels), u8 = "
                         "clip(rint(d), 0, 255), viridis = colours over --vrange (default: the map's own range)")
    ap.add_argument("--vrange", nargs=2, type=float, default=None, metavar=("LO", "HI"),
                    help="with --encode viridis: the fixed range of the colour map, so that frames compare")
    ap.add_argument("--error_map", action="store_true",
                    help="with --path_disp_gt: write <stem>_err.png next to the disparity, the KITTI devkit's "
                         "log-scale error picture")
    return ap


def encode_outputs(disp, out, encode=None, vrange=None, mask=None, path_disp_gt=None, error_map=False):
    """The files of ``--encode`` / ``--error_map``: ``disp`` (H,W) float32 (and ``mask`` (H,W) bool, the ground
    truth file) go to the device, ``costvolume.encode_disparity`` makes the bytes, ``submit.write_png``
    writes ``out`` and ``<stem>_err.png``.  Returns the paths written."""
    from . import costvolume as cv
    from .submit import write_png
    dev = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))[None].cuda()
    want = {"kitti16": "u16", "u8": "u8", "viridis": "rgb", None: None}[encode]
    gt = None
    if error_map:
        from .img_rw import load_disp
        gt = np.asarray(load_disp(path_disp_gt), dtype=np.float32)
        if gt.shape != disp.shape:
            raise ValueError("ground truth %s does not match the prediction %s" % (gt.shape, disp.shape))
    res = cv.encode_disparity(dev(disp, np.float32), gt=None if gt is None else dev(gt, np.float32),
                              mask=None if mask is None else dev(mask, np.uint8),
                              want=tuple(n for n in (want, "err" if error_map else None) if n), vrange=vrange)
    paths = []
    for name, path in ((want, out), ("err" if error_map else None, os.path.splitext(out)[0] + "_err.png")):
        if name:
            write_png(path, res[name][0].cpu().numpy())
            paths.append(path)
    return paths


def main(argv=None):
    from .img_rw import imread
    from .models import model_create_by_name
    args = build_parser().parse_args(argv)
    if args.fill and not args.lr_check:
        raise SystemExit("--fill needs --lr_check")
    if args.peak and args.lr_check:
        raise SystemExit("--peak cannot be combined with --lr_check: the check compares the two views' expectation maps")
    if args.conf_threshold is not None and not args.confidence:
        raise SystemExit("--conf_threshold needs --confidence")
    if args.conf_radius < 0:
        raise SystemExit("--conf_radius must be >= 0")
    if args.vrange is not None and args.encode != "viridis":
        raise SystemExit("--vrange needs --encode viridis")
    if args.error_map and not args.path_disp_gt:
        raise SystemExit("--error_map needs --path_disp_gt")
    if args.encode and (args.out or "").endswith(".pfm"):
        raise SystemExit("--encode writes a PNG, --out names a PFM")
    speckle = speckle_args(args.speckle)
    if not torch.cuda.is_available():
        raise SystemExit("dsmnet_amd.deploy needs an MI355X: the HIP path has no CPU fallback")
    imgL, imgR = imread(args.path_left), imread(args.path_right)
    model = model_create_by_name(args.net, args.maxdisparity)
    load_weights(model, args.path_weight)
    model = model.eval().cuda()
    mask = conf = keep = None
    if args.confidence or args.peak:
        # one forward of the pair that predicts the written view (with --lr_check too: the check's own
        # forwards are not touched); --flip mirrors and swaps, and the maps are flipped back
        pair = (np.flip(imgR, axis=1), np.flip(imgL, axis=1)) if args.flip else (imgL, imgR)
        try:
            conf = conf_predict(model, pair[0], pair[1], args.conf_radius)
        except TypeError as e:                   # a network without a cost head
            raise SystemExit("--confidence / --peak: %s" % e)
        if args.flip:
            conf = {k: np.flip(v, axis=-1) for k, v in conf.items()}
    if args.peak or (conf is not None and not args.lr_check):
        disp, out = conf["peak" if args.peak else "disp"], args.out or "disp%s.png" % ("R" if args.flip else "L")
    elif args.lr_check:
        side = "R" if args.flip else "L"
        res = lr_predict(model, imgL, imgR, args.lr_threshold, args.fill, speckle)
        raw, out = res["disp" + side], args.out or "disp%s.png" % side
        mask = res[("keep" if speckle else "mask") + side]
        disp = res["filled" + side] if args.fill else raw
        if args.path_disp_gt:
            print("D1 %.4f %%  EPE %.4f px  pixelerror %.4f" % evaluate_pair(imgL, imgR, raw, args.path_disp_gt, args.flip))
            print("consistent pixels (%.2f %%): D1 %.4f %%  EPE %.4f px  pixelerror %.4f"
                  % ((100.0 * mask.mean(),) + tuple(evaluate_consistent(imgL, imgR, raw, mask, args.path_disp_gt, args.flip))))
    elif args.flip:
        disp = disp_predict(model, np.flip(imgR, axis=1), np.flip(imgL, axis=1), True)
        disp, out = np.flip(disp, axis=-1), args.out or "dispR.png"
    else:
        disp, out = disp_predict(model, imgL, imgR, True), args.out or "dispL.png"
    if args.path_disp_gt and mask is None:
        print("D1 %.4f %%  EPE %.4f px  pixelerror %.4f" % evaluate_pair(imgL, imgR, disp, args.path_disp_gt, args.flip))
    if speckle and not args.lr_check:
        raw = disp
        disp, keep = speckle_filter(raw, *speckle)
        if args.path_disp_gt:
            print("kept pixels (%.2f %%): D1 %.4f %%  EPE %.4f px  pixelerror %.4f"
                  % ((100.0 * keep.mean(),) + tuple(evaluate_consistent(imgL, imgR, raw, keep, args.path_disp_gt, args.flip))))
    if args.path_disp_gt and conf is not None and args.conf_threshold is not None:
        sure = conf["pwin"] >= args.conf_threshold
        scored = raw if (args.lr_check or speckle) else disp
        print("confident pixels (pwin >= %g, %.2f %%): D1 %.4f %%  EPE %.4f px  pixelerror %.4f"
              % ((args.conf_threshold, 100.0 * sure.mean()) +
                 tuple(evaluate_consistent(imgL, imgR, scored, sure, args.path_disp_gt, args.flip))))
    if args.encode or args.error_map:
        # kitti16 / u8 mark what the check rejects as invalid; a filled map has no such pixel
        encode_outputs(disp, out, args.encode, args.vrange, None if args.fill else (keep if mask is None else mask),
                       args.path_disp_gt, args.error_map)
    if args.encode:
        pass
    elif out.endswith(".pfm"):
        from .img_rw import save_pfm
        save_pfm(out, np.ascontiguousarray(disp, dtype=np.float32))
    else:
        import matplotlib.pyplot as plt
        plt.imsave(out, disp)
    if mask is not None:
        import matplotlib.pyplot as plt
        plt.imsave(os.path.splitext(out)[0] + "_mask.png", mask.astype(np.uint8) * 255, cmap="gray", vmin=0, vmax=255)
    if args.confidence:
        from .img_rw import imwrite
        gray = np.rint(np.clip(conf["pwin"], 0.0, 1.0) * 255.0).astype(np.uint8)
        # the levels themselves, R = G = B (a colour map would quantise them a second time)
        imwrite(os.path.splitext(out)[0] + "_conf.png", np.repeat(gray[:, :, None], 3, axis=2))
    return out


if __name__ == "__main__":
    main()
