"""Shared by tests/test_extent_plans.py (CPU) and tests/test_large_extents_gpu.py: the table of convolution launches
whose tensors cross 2 GiB / 4 GiB, the window finder and the windowed float64 reference.

A tensor of several GiB has no full float64 reference on the CPU.  A case is checked on *windows* instead: boxes of
a few z-planes x 12 rows x 48 columns x all channels of the output, placed where 32-bit addressing goes wrong --
the first and the last voxel, both sides of every 2^31 / 2^32 byte boundary of the input, the output and the
residual -- and at seeded random places.  The reference of a window needs the input crop with its halo only.
Both pieces are checked on the CPU (test_extent_plans.py): the finder on the shapes of every case (no tensors),
the windowed reference against the full-tensor reference of tests/test_conv_plans_gpu.py on small shapes."""
import collections
import random

import torch
import torch.nn.functional as F

from tests.test_conv_plans import CHUNKED, R

GIB = 1 << 30
BOUNDARIES = (1 << 31, 1 << 32, 1 << 33)
ITEM32 = (24, 353, 1010)            # at 32 channels 1.0200 GiB; ragged tiles in y (353 = 44 * 8 + 1) and x (1010 = 31 * 32 + 18)
ITEM64 = (12, 353, 1010)            # the same bytes at 64 channels
SPAN = (3, 12, 48)                  # window: z-planes x rows x columns
SPAN_COUT1 = (4, 24, 64)            # one channel per voxel: larger boxes, so that a case still covers 20,000 values

# row: the launch (tests/test_conv_plans.py ``Row``; ``name`` is the plan the launched arguments must give).
# res: None | "full" (the output's size) | "short" (one voxel shorter in z, y, x: the output is the common corner).
# gib: the ceiling of the case's peak of live device memory (tensors + the item-by-item comparisons), GiB; the
# measured peak (torch.cuda.max_memory_allocated) is asserted against it.
Big = collections.namedtuple("Big", "row res gib")


def nbytes(B, C, size):
    return 4 * B * C * size[0] * size[1] * size[2]


def out_dims(row):
    return tuple(2 * v if row.tr else (v - 1) // row.stride + 1 for v in row.size)


def res_dims(big):
    o = out_dims(big.row)
    return None if big.res is None else (o if big.res == "full" else tuple(v - 1 for v in o))


def y_dims(big):
    r = res_dims(big)
    return out_dims(big.row) if r is None else tuple(min(a, b) for a, b in zip(out_dims(big.row), r))


def _cases():
    out = []
    for m in ("f16x2", "bf16x3"):
        zs = "conv3d_zs_%s_mfma_kernel" % m
        # 1. 32 -> 32 (kind 7): 2.04 and 4.08 GiB in, out and residual
        out += [Big(R(zs, m, 32, 32, ITEM32, B=2), "full", 8.2), Big(R(zs, m, 32, 32, ITEM32, B=4), "full", 14.3)]
        # 2. the same layer from a virtual volume of 2 x 32 feature channels: only y and the residual are large
        out += [Big(R(zs + "<vol>", m, 64, 32, ITEM32, B=2, vol=1), "full", 6.3),
                Big(R(zs + "<vol>", m, 64, 32, ITEM32, B=4, vol=1), "full", 10.6)]
        # 3. 64 -> 32 (kind 7): 4.08 GiB in, 2.04 GiB out
        out += [Big(R(zs, m, 64, 32, ITEM64, B=4), "full", 9.2)]
        # 4. / 5. the split kernels (kind 5) with one item of 0.9775 / 0.9988 x 2^31 bytes: the out-of-range marker
        # of their staged loads sits at 2^31, the halo offsets of the last tiles come closest to it here
        out += [Big(R("conv3d_%s_mfma_kernel<NT=2,TM=2>", m, 64, 64, (23, 353, 1010)), "full", 9.8),
                Big(R("conv3d_%s_mfma_kernel<S=2,NT=2,TM=1>", m, 32, 64, (47, 353, 1010), stride=2), "full", 4.1)]
    # ... and their fp32-input fallback (kind 0) from 2^31 bytes to just under 2^32
    # (2^31 bytes is 1.96 items of 1.02 GiB: with two items the boundary falls into the LAST plane of item 1, whose tiles
    # stick out of the volume in z and are staged through 64-bit pointers; the three-item cases put whole interior
    # tiles -- staged through the buffer descriptor with a 32-bit box offset -- past 2^31: test_extent_plans.py checks it)
    out += [Big(R("conv3d_mfma_kernel<S=1,NT=2,TM=2,CK=8>", "f16x2", 64, 64, ITEM64, B=2), "full", 8.2),
            Big(R("conv3d_mfma_kernel<S=1,NT=2,TM=2,CK=8>", "f16x2", 64, 64, (12, 450, 1010), B=3), "full", 14.4),
            Big(R("conv3d_mfma_kernel<S=2,NT=2,TM=1,CK=8>", "f16x2", 32, 64, ITEM32, B=2, stride=2), "full", 3.6),
            Big(R("conv3d_mfma_kernel<S=2,NT=2,TM=1,CK=8>", "f16x2", 32, 64, (24, 450, 1010), B=3, stride=2), "full", 6.6)]
    # 6. transposed 64 -> 32: 1.02 GiB in and 4.09 GiB out with a short residual (kind 6; z-sliding in the fp16
    # modes); 2.05 GiB in and 8.18 GiB out without one (kind 1)
    out += [Big(R("deconv3d_zs_f16x2_mfma_kernel<NT=1>", "f16x2", 64, 32, (12, 177, 1010), B=2, stride=2, tr=1), "short", 12.8),
            Big(R("deconv3d_bf16x3_mfma_kernel<NT=1>", "bf16x3", 64, 32, (12, 177, 1010), B=2, stride=2, tr=1), "short", 12.8),
            Big(R("deconv3d_mfma_kernel<NT=1,CK=16>", "f16x2", 64, 32, (12, 177, 1010), B=4, stride=2, tr=1), None, 14.4)]
    # 7. the Cout = 1 heads: 2.04 and 3.90 GiB in
    for B, size in ((2, ITEM32), (3, (24, 450, 1010))):
        out += [Big(R("conv3d_cout1_zslide_kernel", "f16x2", 32, 1, size, B=B), None, 4.2),
                Big(R("conv3d_cout1_kernel<CK=8>", "f16x2", 32, 1, size, B=B, flags=CHUNKED), None, 4.2)]
    out += [Big(R("deconv3d_cout1_kernel", "f16x2", 32, 1, ITEM32, B=2, stride=2, tr=1), None, 3.1)]
    # (with two items no interior box of the transposed head starts past 2^31: a third case at 3.90 GiB)
    out += [Big(R("deconv3d_cout1_kernel", "f16x2", 32, 1, (24, 450, 1010), B=3, stride=2, tr=1), None, 6.0)]
    return out


BIG_CASES = _cases()


def big_id(big):
    r = big.row
    return "%s-%s-c%d-%s-b%d%s-%.1fGiB" % (r.name, r.mode, r.cin, "x".join(map(str, r.size)), r.B,
                                           "-f%x" % r.flags if r.flags else "", big.gib)


# ---------------------------------------------------------------------------------------- the window finder
def voxel_at(dims, C, byte):
    """(b, z, y, x) of the voxel of an fp32 NDHWC tensor (B, D, H, W, C) that holds byte offset ``byte``."""
    B, D, H, W = dims
    v = byte // (4 * C)
    assert 0 <= v < B * D * H * W, (dims, C, byte)
    return (v // (D * H * W), v // (H * W) % D, v // W % H, v % W)


def linear(dims, voxel):
    _, D, H, W = dims
    b, z, y, x = voxel
    return ((b * D + z) * H + y) * W + x


def window_around(dims, voxel, span):
    """The box of ``span`` voxels centred on ``voxel``, moved inside the volume: (b, (z0, z1), (y0, y1), (x0, x1))."""
    box = []
    for c, n, s in zip(voxel[1:], dims[1:], span):
        lo = min(max(c - s // 2, 0), max(n - s, 0))
        box.append((lo, min(lo + s, n)))
    return (voxel[0],) + tuple(box)


def find_window(dims, C, byte, span):
    """The voxel holding ``byte`` and the clipped window around it."""
    v = voxel_at(dims, C, byte)
    return v, window_around(dims, v, span)


def input_box(row, win):
    """The input voxels an output window reads, per axis (lo, hi) with hi exclusive, not yet clipped to the
    volume: k = 3, padding 1, stride ``row.stride``; transposed (k3, s2, p1, op1): output o reads inputs
    o // 2 and, for odd o, o // 2 + 1."""
    if row.tr:
        return tuple((o0 // 2, o1 // 2 + 1) for o0, o1 in win[1:])
    return tuple((o0 * row.stride - 1, (o1 - 1) * row.stride + 2) for o0, o1 in win[1:])


def to_output(row, voxel, which):
    """The output voxel whose window looks at ``voxel`` of the input ("x"), the output or the residual."""
    if which != "x":
        return voxel
    return (voxel[0],) + tuple(2 * c if row.tr else c // row.stride for c in voxel[1:])


def case_windows(big, seed=0):
    """[(label, window)] of a case, windows in output coordinates.  Labels: first, last, rand<i>, and
    <tensor>@2^<k> for every 2^31 / 2^32 / 2^33 byte boundary inside the input (x), the output (y) and the
    residual (r).  At least six windows: further random ones where a case crosses few boundaries."""
    row = big.row
    ydims = (row.B,) + y_dims(big)
    span = SPAN_COUT1 if row.cout == 1 else SPAN
    wins = [("first", window_around(ydims, (0, 0, 0, 0), span)),
            ("last", window_around(ydims, tuple(v - 1 for v in ydims), span))]
    tensors = [("y", ydims, row.cout)]
    if not row.vol:
        tensors.append(("x", (row.B,) + tuple(row.size), row.cin))
    if big.res:
        tensors.append(("r", (row.B,) + res_dims(big), row.cout))
    for which, dims, C in tensors:
        total = 4 * C * dims[0] * dims[1] * dims[2] * dims[3]
        for bound in BOUNDARIES:
            if bound < total:
                o = to_output(row, voxel_at(dims, C, bound), which)
                o = (o[0],) + tuple(min(c, n - 1) for c, n in zip(o[1:], ydims[1:]))      # the short residual's corner
                wins.append(("%s@2^%d" % (which, bound.bit_length() - 1), window_around(ydims, o, span)))
    rng = random.Random(1234 + seed)
    k = 0
    while k < 2 or len(wins) < 6:
        wins.append(("rand%d" % k, window_around(ydims, tuple(rng.randrange(n) for n in ydims), span)))
        k += 1
    return wins


def window_values(row, wins):
    return sum(row.cout * (w[1][1] - w[1][0]) * (w[2][1] - w[2][0]) * (w[3][1] - w[3][0]) for _, w in wins)


# ---------------------------------------------------------------------------------------- the windowed reference
def tensor_fetch(t):
    """fetch(b, box) of a (B, C, D, H, W) tensor on any device: the box (in-volume ranges) as float64 on the CPU."""
    def fetch(b, box):
        (z0, z1), (y0, y1), (x0, x1) = box
        return t[b:b + 1, :, z0:z1, y0:y1, x0:x1].cpu().double()
    return fetch


def volume_fetch(fL, fR):
    """fetch(b, box) of the concatenation volume of two (B, C, H, W) maps, never built whole: channels
    [left | right shifted by the plane's disparity d], the right half zero where x < d (no left mask)."""
    fL, fR = fL.cpu().double(), fR.cpu().double()
    C = fL.shape[1]

    def fetch(b, box):
        (z0, z1), (y0, y1), (x0, x1) = box
        out = torch.zeros(1, 2 * C, z1 - z0, y1 - y0, x1 - x0, dtype=torch.float64)
        out[0, :C] = fL[b, :, y0:y1, x0:x1].unsqueeze(1)
        for k, d in enumerate(range(z0, z1)):
            lo = max(x0, d)                                   # first column of the box with x - d >= 0
            if lo < x1:
                out[0, C:, k, :, lo - x0:] = fR[b, :, y0:y1, lo - d:x1 - d]
        return out
    return fetch


def padded_crop(row, in_dims, fetch, win):
    """The input box of an output window as float64 (1, Cin, ...), zeros where the box leaves the volume; and the box."""
    box = input_box(row, win)
    clipped = tuple((max(lo, 0), min(hi, n)) for (lo, hi), n in zip(box, in_dims))
    pad = []
    for (lo, hi), (clo, chi) in zip(reversed(box), reversed(clipped)):            # F.pad: last axis first
        pad += [clo - lo, hi - chi]
    return F.pad(fetch(win[0], clipped), pad), box


def windowed_reference(row, in_dims, fetch, w, sc, sh, fetch_res, relu, win):
    """float64 reference of one output window (1, Cout, dz, dy, dx): the input crop with its halo, zeros where the
    crop leaves the volume, torch's convolution, the folded scale / shift, the residual's window (the output is
    the common corner: same coordinates) and the ReLU after (1) or before (2) the addition."""
    crop, box = padded_crop(row, in_dims, fetch, win)
    wd = w.double().cpu()
    if row.tr:
        y = F.conv_transpose3d(crop, wd, stride=2, padding=1, output_padding=1)
        y = y[(slice(None), slice(None)) + tuple(slice(o0 - 2 * lo, o1 - 2 * lo)
                                                 for (o0, o1), (lo, _) in zip(win[1:], box))]
    else:
        y = F.conv3d(crop, wd, stride=row.stride)
    assert tuple(y.shape[2:]) == tuple(o1 - o0 for o0, o1 in win[1:]), (y.shape, win)
    y = y * sc.double().cpu().view(1, -1, 1, 1, 1) + sh.double().cpu().view(1, -1, 1, 1, 1)
    if relu == 2:
        y = y.relu()
    if fetch_res is not None:
        y = y + fetch_res(win[0], win[1:])
    return y.relu() if relu == 1 else y
