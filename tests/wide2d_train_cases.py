"""Shapes, inputs and float64 references shared by tests/test_wide2d_train_reference.py (CPU) and
tests/test_wide2d_train_gpu.py: training through the wide 3x3 layers (``costvolume.wide_conv2d_relu``).

Inputs follow tests/test_wide2d_gpu.py::case_data: ``w`` scaled by sqrt(2 / (9 Cin)) and a bias with the spread
of the pre-activation, so that ReLU clips about half the outputs.  Everything is computed once and never
modified."""
import functools

import torch
import torch.nn.functional as F

from tests.helpers import seeded

# id: ((B, Cin, H, W), Cout, stride)
CASES = {
    "A": ((1, 1024, 6, 20), 1024, 1),      # the real conv6b: one M-block, 16 K-ranges, the largest K
    "B": ((2, 256, 7, 11), 512, 2),        # odd H and W: gradient extent 7 x 11 = 2*4-1 x 2*6-1, batch 2
    "C": ((2, 512, 5, 33), 512, 1),        # a 33-wide row crosses a 32-pixel M-tile
    "D": ((1, 512, 12, 40), 1024, 2),      # even extents (Ho = 2 Hi), 480 gradient pixels in one block
    "E": ((1, 256, 22, 36), 256, 2),       # dx launch: two M-blocks of 11 rows, the second begins at the odd row 11
    "F": ((1, 256, 21, 75), 512, 2),       # dx launch: seven column blocks of 11, origins 11, 33, 55 are odd
    "G": ((2, 256, 9, 70), 256, 1),        # five column blocks at stride 1, batch 2
}
IDS = sorted(CASES)
STRIDE2 = [k for k in IDS if CASES[k][2] == 2]

F16X2_MAX, F16X2_RMS = 1.5e-6, 6e-7        # the wide kernel's bands (tests/test_wide2d_gpu.py)
F16_MAX, F16_RMS = 3e-3, 6e-4
BANDS = {"f16x2": (F16X2_MAX, F16X2_RMS), "f16": (F16_MAX, F16_RMS)}
TOL = {"f16x2": 1e-4, "f16": 4e-3}         # the gradient bounds of tests/test_bwd_ranges_gpu.py


def out_size(key):
    (B, cin, H, W), cout, s = CASES[key]
    return (H - 1) // s + 1, (W - 1) // s + 1


@functools.lru_cache(maxsize=None)
def case_data(key):
    """(x, w, bias, float64 pre-activation conv + bias, cotangent) of CASES[key]."""
    i = IDS.index(key)
    shape, cout, stride = CASES[key]
    cin = shape[1]
    x = seeded(900 + i, *shape)
    w = seeded(1000 + i, cout, cin, 3, 3, scale=(2.0 / (9 * cin)) ** 0.5)
    pre = F.conv2d(x.double(), w.double(), stride=stride, padding=1)
    b = (seeded(1100 + i, cout).double() * pre.std()).float()
    pre = pre + b.double().view(1, -1, 1, 1)
    cot = seeded(1200 + i, *pre.shape)
    return x, w, b, pre, cot


def grads64(key, mask):
    """float64 autograd of relu(conv2d(x, w) + b) with the ReLU mask given: (dX, dW, db) for the cotangent
    ``cot * mask``."""
    x, w, b, _, cot = case_data(key)
    stride = CASES[key][2]
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    g = cot.double() * mask.double()
    dx, dw = torch.autograd.grad(F.conv2d(x64, w64, stride=stride, padding=1), [x64, w64], g)
    return dx, dw, g.sum(dim=(0, 2, 3))


def zero_interleave(g, H, W):
    """X' of H x W with X'[2i][2j] = g[i][j], zero elsewhere."""
    z = g.new_zeros(g.shape[0], g.shape[1], H, W)
    z[:, :, ::2, ::2] = g
    return z


def rel(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item() / ref.abs().max().item()


def band_errors(y, ref):
    err = (y.detach().double().cpu() - ref).abs()
    return err.max().item() / ref.abs().max().item(), (err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


# ---- a restatement of the kernel's M-block choice (csrc/conv_common.hpp wide2d_geometry) at stride 1 ----
WIDE_SLOTS, WIDE_PIXELS = 768, 512


def geometry_s1(Ho, Wo):
    """(R, CW, nby, nbx) of a stride-1 launch over Ho x Wo: the fewest rounds of M-tiles, then the fewest blocks."""
    best = None
    for nbx in range(1, 9):
        CW = (Wo + nbx - 1) // nbx
        XP = CW + 2
        if CW > WIDE_PIXELS or 3 * XP > WIDE_SLOTS:
            continue
        R = min(WIDE_PIXELS // CW, WIDE_SLOTS // XP - 2, Ho)
        nby = (Ho + R - 1) // R
        R = (Ho + nby - 1) // nby
        tiles = (R * CW + 31) // 32
        cost = nbx * nby * ((tiles + 3) // 4) * 1024 + nbx * nby
        if best is None or cost < best[0]:
            best = (cost, R, CW, nby, nbx)
    return best[1:]
