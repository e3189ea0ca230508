"""Result maps of a disparity batch: the device encoder (csrc/encode.hip, costvolume.encode_disparity)
against the host path the tree had before it, and ``submit``'s file rate against the forward's.

  encode   every call event-timed after warm-up, eager (what a caller pays: allocations + launch) and as
           a captured graph of 20 calls replayed (the launches alone), for u16 alone, the four outputs at
           a fixed range, and the four outputs with auto-range (two launches).  Floor: the bytes the
           form moves, at the 6.3 TB/s a device copy reaches.
  host     the same outputs on one host thread: D2H of the fp32 map (and ground truth), then numpy /
           matplotlib -- rint + clip for u16, ``Normalize`` + ``viridis(bytes=True)`` for the colours, the
           bin search for the error picture.  Host clock around work that ends in a synchronise.
  submit   (--submit N) N synthetic 375x1242 pairs with ground truth written to a temporary directory,
           PSMNet with random weights, pad_multiple 64 (384x1280), formats u16 + viridis + error:
           files per second at threads 1, 4 and 16 and batch 1 and 4, against the forward alone on a
           resident batch and against the loader + forward without encoding or writing.

Prints one JSON line.

    python scripts/bench_encode.py [--reps 30] [--warmup 5] [--submit 24]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsmnet_amd import costvolume as cv          # noqa: E402

COPY_BYTES_PER_S = 6.3e12                        # MI355X: what a device copy reaches
ALL = ("u16", "u8", "rgb", "err")
EDGES = [np.float32(2.0 ** k) for k in range(-4, 5)]
COLOURS = np.array([[49, 54, 149], [69, 117, 180], [116, 173, 209], [171, 217, 233], [224, 243, 248],
                    [254, 224, 144], [253, 174, 97], [244, 109, 67], [215, 48, 39], [165, 0, 38]], np.uint8)


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def host_outputs(disp, gt, auto):
    """The parent path: fp32 to the host, then numpy / matplotlib on one thread."""
    import matplotlib
    from matplotlib.colors import Normalize
    d, g = disp.cpu().numpy(), gt.cpu().numpy()
    u16 = np.clip(np.rint(d * np.float32(256.0)), 1, 65535).astype(np.uint16)
    u8 = np.clip(np.rint(d), 0, 255).astype(np.uint8)
    cmap = matplotlib.colormaps["viridis"]
    rgb = np.stack([cmap(Normalize(None if auto else 0.0, None if auto else 192.0)(x), bytes=True)[..., :3] for x in d])
    e = np.abs(g - d)
    with np.errstate(all="ignore"):
        n = np.fmin(e / np.float32(3.0), (e / g) / np.float32(0.05))
    err = np.where((g > 0)[..., None], COLOURS[np.searchsorted(np.array(EDGES), n, side="right")], 0).astype(np.uint8)
    return u16, u8, rgb, err


def graphed(fn, n=20):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [fn() for _ in range(n)]
    return graph, keep, n


def encode_case(B, H, W, reps, warmup):
    g = torch.Generator().manual_seed(0)
    disp = (torch.rand(B, H, W, generator=g) * 190.0).cuda()
    gt = (disp.cpu() + torch.randn(B, H, W, generator=g) * 2.0).clamp_(min=0.0).cuda()
    px = float(B * H * W)
    forms = {"u16": (lambda: cv.encode_disparity(disp, want=("u16",)), 6.0),
             "all4_fixed": (lambda: cv.encode_disparity(disp, gt, want=ALL, vrange=(0.0, 192.0)), 17.0),
             "all4_auto": (lambda: cv.encode_disparity(disp, gt, want=ALL), 21.0)}
    host = {"host_fixed": lambda: host_outputs(disp, gt, False), "host_auto": lambda: host_outputs(disp, gt, True)}
    out = {"shape": [B, H, W]}
    for _ in range(warmup):
        for fn, _b in forms.values():
            fn()
    for fn in host.values():
        fn()
    graphs = {k: graphed(fn) for k, (fn, _b) in forms.items()}
    ts = {k: [] for k in list(forms) + [k + "_graph" for k in forms]}
    for _ in range(reps):
        for k, (fn, _b) in forms.items():                                # alternate
            ts[k].append(one(fn))
            graph, _keep, n = graphs[k]
            ts[k + "_graph"].append(one(graph.replay) / n)
    for k, (fn, b) in forms.items():
        out[k] = dict(stats(ts[k]), graph_per_call=stats(ts[k + "_graph"]), bytes_per_px=b,
                      floor_ms=b * px / COPY_BYTES_PER_S * 1e3)
    for k, fn in host.items():
        out[k] = stats([wall(fn) for _ in range(max(3, reps // 6))])
    same = host_outputs(disp, gt, True)
    dev = cv.encode_disparity(disp, gt, want=ALL)
    out["host_equals_device"] = {n: bool(np.array_equal(dev[n].cpu().view(torch.uint8).numpy().reshape(-1),
                                                        a.reshape(-1).view(np.uint8)))
                                 for n, a in zip(ALL, same)}
    return out


def submit_case(files, threads_list):
    from dsmnet_amd import transforms
    from dsmnet_amd.datasets import Dataset_stereo, DeviceLoader
    from dsmnet_amd.models import model_create_by_name
    from dsmnet_amd.submit import submit
    from PIL import Image
    root = tempfile.mkdtemp(prefix="bench_encode_")
    try:
        rng = np.random.RandomState(0)
        paths = [[], [], []]
        yy, xx = np.mgrid[0:375, 0:1242]
        for i in range(files):
            # smooth pictures, so that PNG decoding and encoding cost what photographs cost rather than noise
            base = (np.sin(xx / (17.0 + i)) * 60 + np.cos(yy / 23.0) * 60 + 128)[..., None] + rng.randint(0, 12, (375, 1242, 3))
            left = base.clip(0, 255).astype(np.uint8)
            disp = ((np.sin(xx / 90.0 + i) + 1.5) * 20 * 256).astype(np.uint16)
            for k, a in enumerate((left, np.roll(left, -7, axis=1), disp)):
                p = os.path.join(root, "in%d" % k, "%06d_10.png" % i)
                os.makedirs(os.path.dirname(p), exist_ok=True)
                Image.fromarray(a).save(p)
                paths[k].append(p)
        ds = Dataset_stereo(paths[0], paths[1], paths[2])
        torch.manual_seed(0)
        model = model_create_by_name("psmnet", 192).cuda().eval()
        x = torch.rand(1, 6, 384, 1280).cuda()
        with torch.no_grad(), cv.amax_scope(x.device):
            for _ in range(3):
                model(x[:, :3], x[:, 3:])
            fwd = stats([one(lambda: model(x[:, :3], x[:, 3:])) for _ in range(10)])
        out = {"files": files, "forward_alone": fwd, "forward_files_per_s": 1e3 / fwd["median_ms"]}
        norm = transforms.Stereo_normalize()

        def load_and_forward():
            with torch.no_grad():
                for batch, _ in DeviceLoader(ds, transforms.Stereo_ToTensor(), 1, threads=4):
                    seen = torch.nn.functional.pad(norm(batch[:, :6].clone()), (0, 38, 9, 0))
                    with cv.amax_scope(batch.device):
                        model(seen[:, :3], seen[:, 3:6])
        out["loader_forward_files_per_s"] = files / (wall(load_and_forward) / 1e3)
        import contextlib
        import io
        for bs in (1, 4):                                                 # two sets of buffers: 2 * bs * 3 PNGs in flight
            for t in threads_list:
                dst = os.path.join(root, "out_b%d_t%d" % (bs, t))
                with contextlib.redirect_stdout(io.StringIO()):
                    ms = wall(lambda: submit(model, ds, dst, batch_size=bs, pad_multiple=64,
                                             formats=("u16", "viridis", "error"), threads=t))
                out["submit_batch_%d_threads_%d_files_per_s" % (bs, t)] = files / (ms / 1e3)
        dst = os.path.join(root, "out_u16")
        with contextlib.redirect_stdout(io.StringIO()):
            ms = wall(lambda: submit(model, ds, dst, batch_size=4, pad_multiple=64, formats=("u16",), threads=16))
        out["submit_u16_only_batch_4_threads_16_files_per_s"] = files / (ms / 1e3)
        return out
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--submit", type=int, default=0, help="files of the submit measurement (0: skip it)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_encode.py measures on the GPU: none found")
    res = {"reps": a.reps, "cases": [encode_case(1, 384, 1280, a.reps, a.warmup), encode_case(8, 384, 1280, a.reps, a.warmup)]}
    if a.submit:
        res["submit"] = submit_case(a.submit, (1, 4, 16))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
