"""CPU: the extent guards of the convolution planner (make_plan in dsmnet_amd/csrc/conv3d.hip) and of
``dsm_basicblock2d_fwd``, one row on each side of every guard, and the two pieces of test machinery that
tests/test_large_extents_gpu.py relies on (tests/extents.py).

The kernels address memory with 32-bit quantities: buffer descriptors of ``unsigned`` extent, per-lane byte
offsets, an out-of-range marker at 2^31.  The host code switches kernels on byte extents accordingly; DESIGN.md
("Extent limits") lists the limits, and every line of that list names rows of this module:

* ``EXTENT_ROWS``: the largest extent that still passes and the first one that does not, with the exact plan name
  or DSM_ERR_UNSUPPORTED on each side.  Pointers are fake (16: aligned, never dereferenced); for a refused row
  ``dsm_conv3d_fwd`` must return what ``dsm_conv3d_plan`` does (it returns before any launch);
* ``costvolume.basicblock2d_ok`` (a Python mirror) / ``_split_kernel_layer`` (asks the plan) on the same rows;
* the window finder on the shapes of every GPU case, the windowed float64 reference against the full one.

The shapes are products of the prime factors of 2^k - 1: (1, 47, 178481) is 2^23 - 1 voxels, (1, 4095, 4097)
2^24 - 1, (31, 601, 1801) 2^25 - 1 -- one voxel short of the guard at 256 or 128 bytes per voxel."""
import ctypes

import pytest
import torch

from dsmnet_amd import _lib
from oracle import ops as OO
from tests import extents as E
from tests.helpers import seeded
from tests.test_conv_plans import CHUNKED, R, make_args, plan, row_args
from tests.test_wide2d_plans import precision

V23, V23_AT = (1, 47, 178481), (1, 2048, 4096)          # 2^23 - 1 | 2^23 voxels
V24, V24_AT = (1, 4095, 4097), (1, 4096, 4096)          # 2^24 - 1 | 2^24
V25, V25_AT = (31, 601, 1801), (2, 4096, 4096)          # 2^25 - 1 | 2^25
FP32_64 = "conv3d_mfma_kernel<S=1,NT=2,TM=2,CK=8>"
FP32_S2 = "conv3d_mfma_kernel<S=2,NT=2,TM=1,CK=8>"
FP32_32 = "conv3d_mfma_kernel<S=1,NT=1,TM=2,CK=16>"
UNSUPPORTED = -2                                        # DSM_ERR_UNSUPPORTED (include/dsmnet_hip.h)


def X(expect, mode, cin, cout, size, **kw):
    """A row: ``expect`` is the plan name (%s: the mode), or None where the arguments must be refused."""
    return (None if expect is None else (expect % mode if "%s" in expect else expect), mode, cin, cout, size, kw)


EXTENT_ROWS = []
for _m in ("f16x2", "bf16x3"):
    _zs = "deconv3d_zs_%s_mfma_kernel" if _m == "f16x2" else "deconv3d_%s_mfma_kernel"        # no zs_ form on bf16x3
    EXTENT_ROWS += [
        # 3-D 64 -> 64, stride 1 (256 B per voxel): split < 2^31 B <= fp32-input < 2^32 B <= refused
        X("conv3d_%s_mfma_kernel<NT=2,TM=2>", _m, 64, 64, V23), X(FP32_64, _m, 64, 64, V23_AT),
        X(FP32_64, _m, 64, 64, V24), X(None, _m, 64, 64, V24_AT),
        # 3-D 32 -> 64, stride 2 (128 B per voxel)
        X("conv3d_%s_mfma_kernel<S=2,NT=2,TM=1>", _m, 32, 64, V24, stride=2), X(FP32_S2, _m, 32, 64, V24_AT, stride=2),
        X(FP32_S2, _m, 32, 64, V25, stride=2), X(None, _m, 32, 64, V25_AT, stride=2),
        # transposed 64 -> 32 and 64 -> 64
        X(_zs + "<NT=1>", _m, 64, 32, V23, stride=2, tr=1), X("deconv3d_mfma_kernel<NT=1,CK=16>", _m, 64, 32, V23_AT, stride=2, tr=1),
        X("deconv3d_mfma_kernel<NT=1,CK=16>", _m, 64, 32, V24, stride=2, tr=1), X(None, _m, 64, 32, V24_AT, stride=2, tr=1),
        X(_zs + "<NT=2>", _m, 64, 64, V23, stride=2, tr=1), X("deconv3d_mfma_kernel<NT=2,CK=16>", _m, 64, 64, V23_AT, stride=2, tr=1),
        X("deconv3d_mfma_kernel<NT=2,CK=16>", _m, 64, 64, V24, stride=2, tr=1), X(None, _m, 64, 64, V24_AT, stride=2, tr=1),
        # z-sliding (kind 7): any total extent (2.04, 4.08 GiB in; 4.08 GiB in and 2.04 out) ...
        X("conv3d_zs_%s_mfma_kernel", _m, 32, 32, E.ITEM32, B=2), X("conv3d_zs_%s_mfma_kernel", _m, 32, 32, E.ITEM32, B=4),
        X("conv3d_zs_%s_mfma_kernel", _m, 64, 32, E.ITEM64, B=4),
        X("conv3d_zs_%s_mfma_kernel<vol>", _m, 64, 32, E.ITEM32, B=2, vol=1),
        X("conv3d_zs_%s_mfma_kernel<vol>", _m, 64, 32, E.ITEM32, B=4, vol=1),
        # ... while ONE input plane stays under 2^31 - 1 bytes: 2^31 - 128 | 2^31 at 32 inputs, 2^31 - 256 | 2^31 at 64
        X("conv3d_zs_%s_mfma_kernel", _m, 32, 32, V24), X(FP32_32, _m, 32, 32, V24_AT),
        X("conv3d_zs_%s_mfma_kernel", _m, 64, 32, V23), X(FP32_32, _m, 64, 32, V23_AT),
        # a virtual volume: 2 bytes per volume channel (the fp32 features of one side), and the right half's
        # descriptor is one feature plane PLUS the plane's shift of up to Di - 1 voxels: with two planes,
        # (2^24 - 1 + 1) voxels of 128 B reach 2^31, where the out-of-range marker would be a valid offset
        X("conv3d_zs_%s_mfma_kernel<vol>", _m, 64, 32, V24, vol=1), X(None, _m, 64, 32, (2, 4095, 4097), vol=1),
        X(None, _m, 64, 32, V24_AT, vol=1),
    ]
# the Cout = 1 heads (128 B per voxel): launched under 2^32 B, refused from there
for _kw in ({}, {"flags": CHUNKED}, {"stride": 2, "tr": 1}):
    _name = "deconv3d_cout1_kernel" if _kw.get("tr") else ("conv3d_cout1_kernel<CK=8>" if _kw else "conv3d_cout1_zslide_kernel")
    EXTENT_ROWS += [X(_name, "f16x2", 32, 1, V25, **_kw), X(None, "f16x2", 32, 1, V25_AT, **_kw)]
# the wide 2-D layers (kind 8): 2^31 B of input (3 * 2047 * 683 = 2^22 - 1 pixels of 512 B | 2^22), 2^31 - 1
# output elements (7 * 889 * 337 = 2^21 - 1 pixels of 1024 channels | 2^21)
EXTENT_ROWS += [
    X("conv2d_wide_f16x2_mfma_kernel<S=1,N=64,KS=1,units=34440>", "f16x2", 128, 256, (2047, 683), B=3),
    X(None, "f16x2", 128, 256, (1024, 1024), B=4),
    X("conv2d_wide_f16x2_mfma_kernel<S=1,N=64,KS=1,units=66752>", "f16x2", 16, 1024, (889, 337), B=7),
    X(None, "f16x2", 16, 1024, (1024, 1024), B=2),
]
# ... and their transposed mode (kind 9: backward-data of the stride-2 wide layers; ``out``: Ho x Wo, 2 Hi - 1 or 2 Hi),
# which has its own copy of the guard: 2^31 B of input (3 * 1025 * 341 = 2^20 - 1 pixels of 2048 B | 2^20), 2^31 - 1
# output elements (7 * 889 * 337 = 2^21 - 1 pixels of 1024 channels | 2^21)
EXTENT_ROWS += [
    X("deconv2d_wide_f16x2_mfma_kernel<N=64,KS=4,units=137760>", "f16x2", 512, 256, (1025, 341), B=3, out=(2050, 682)),
    X(None, "f16x2", 512, 256, (512, 512), B=4, out=(1024, 1024)),
    X("deconv2d_wide_f16x2_mfma_kernel<N=64,KS=1,units=66752>", "f16x2", 16, 1024, (445, 169), B=7, out=(889, 337)),
    X(None, "f16x2", 16, 1024, (512, 512), B=2, out=(1024, 1024)),
]
del _m, _zs, _kw, _name


def xrow_id(r):
    return "%s-%s-c%d-%d-%s-b%d" % (r[0] or "refused", r[1], r[2], r[3], "x".join(map(str, r[4])), r[5].get("B", 1)) + \
        "".join("-%s%s" % kv for kv in sorted(r[5].items()) if kv[0] != "B")


assert len({xrow_id(r) for r in EXTENT_ROWS}) == len(EXTENT_ROWS)


def build(mode, cin, cout, size, out=None, **kw):
    """The row's arguments; ``out``: a transposed wide 2-D request (kind 9), as tests/test_wide2d_train_reference.py
    builds it: one plane, stride 2, the output's extent given."""
    if out is None:
        return make_args(mode, cin, cout, size, **kw)
    a = make_args(mode, cin, cout, size, stride=2, tr=1, **kw)
    a.Do, a.Ho, a.Wo = 1, out[0], out[1]
    a.relu = 0
    assert 2 * a.Hi - 1 <= a.Ho <= 2 * a.Hi and 2 * a.Wi - 1 <= a.Wo <= 2 * a.Wi
    return a


def in_bytes(a):
    return 4 * a.B * a.Di * a.Hi * a.Wi * a.Cin


@pytest.mark.parametrize("row", EXTENT_ROWS, ids=xrow_id)
def test_each_side_of_an_extent_guard(hip_lib, row):
    from dsmnet_amd import costvolume as cv
    expect, mode, cin, cout, size, kw = row
    a = build(mode, cin, cout, size, **kw)
    rc, name = plan(hip_lib, a)
    assert (rc, name) == ((0, expect) if expect else (UNSUPPORTED, "")), (rc, name, in_bytes(a))
    if expect is None:
        assert hip_lib.dsm_conv3d_fwd(ctypes.byref(a), None) == UNSUPPORTED     # before any launch
        assert hip_lib.dsm_conv3d_workspace_bytes(ctypes.byref(a)) == 0
        return
    # the host layer hands x_amax to the layers _split_kernel_layer names: a plan on a kernel that scales its
    # fp16 operands (kinds 5 to 9: the mode is in the name) without it would fail the launch
    if mode == "f16x2":
        if "_f16x2_" in name:
            assert cv._split_kernel_layer(a), name
        if not cv._split_kernel_layer(a):
            a.x_amax = None
        assert plan(hip_lib, a) == (0, expect)


def test_the_rows_sit_on_the_guards():
    """Arithmetic of the table: within each pair the passing row is ONE voxel (or pixel, or plane shift) short."""
    def voxels(size, B=1):
        n = B
        for v in size:
            n *= v
        return n
    assert voxels(V23) == 2 ** 23 - 1 and voxels(V23_AT) == 2 ** 23
    assert voxels(V24) == 2 ** 24 - 1 and voxels(V24_AT) == 2 ** 24
    assert voxels(V25) == 2 ** 25 - 1 and voxels(V25_AT) == 2 ** 25
    assert voxels((2047, 683), 3) == 2 ** 22 - 1 and voxels((889, 337), 7) == 2 ** 21 - 1
    assert voxels((1025, 341), 3) == 2 ** 20 - 1 and voxels((512, 512), 4) == 2 ** 20           # kind 9, 2048 B per pixel
    assert (voxels(V24) + 2 - 1) * 128 == 2 ** 31                       # the virtual volume with two planes
    for B in (2, 4):
        assert E.nbytes(B, 32, E.ITEM32) == E.nbytes(B, 64, E.ITEM64) == B * 1095260160                 # 1.0200 GiB per item
    assert 2 ** 31 < E.nbytes(2, 32, E.ITEM32) < 2 ** 32 < E.nbytes(4, 32, E.ITEM32)


@pytest.mark.parametrize("C", [32, 64])
def test_basicblock2d_is_refused_at_2_gib_and_its_mirror_agrees(hip_lib, C):
    """``dsm_basicblock2d_fwd`` refuses 2^31 bytes of input (32-bit offsets, the out-of-range marker at 2^31);
    ``basicblock2d_ok`` is False for exactly those shapes, so the towers fall back to two launches instead of
    failing.  The launch side is asked for the refused shapes only (it returns before any launch)."""
    from dsmnet_amd import costvolume as cv
    pix = 2 ** 31 // (4 * C)                           # pixels of C channels in 2^31 bytes: 2^23 | 2^24
    under = (1, 4095, 4097) if C == 32 else (1, 47, 178481)
    assert under[0] * under[1] * under[2] == pix - 1
    shapes = [(under, True), ((8, 1024, pix // 8192), False), ((16, 1024, pix // 8192), False),
              ((2, 353, 1010), True)]
    with precision("f16x2"):
        old = cv.set_option("fuse_blocks", True)
        try:
            for (B, H, W), ok in shapes:
                x = torch.empty((B, C, H, W), device="meta")
                assert cv.basicblock2d_ok(x, C, C, 1, 1) == ok, (B, H, W)
                if not ok:
                    a = _lib.BasicBlock2dArgs()
                    a.x = a.y = a.w1_packed = a.w2_packed = a.x_amax = 16
                    a.B, a.H, a.W, a.C = B, H, W, C
                    a.precision = _lib.DSM_PREC_F16X2
                    assert hip_lib.dsm_basicblock2d_fwd(ctypes.byref(a), None) == UNSUPPORTED
        finally:
            cv.set_option("fuse_blocks", old)


# ------------------------------------------------------------------------------------- the GPU module's machinery
@pytest.mark.parametrize("big", E.BIG_CASES, ids=E.big_id)
def test_the_gpu_cases_name_their_plans_and_extents(hip_lib, big):
    row = big.row
    assert plan(hip_lib, row_args(row)) == (0, row.name)
    xb, yb = E.nbytes(row.B, row.cin, row.size), E.nbytes(row.B, row.cout, E.y_dims(big))
    assert max(xb if not row.vol else 0, yb) > 0.97 * 2 ** 31             # every case is about a large extent
    assert big.gib <= 28


@pytest.mark.parametrize("big", E.BIG_CASES, ids=E.big_id)
def test_the_window_finder_puts_windows_on_both_sides_of_every_boundary(big):
    """Shapes only.  Every case has its first / last / random windows, at least six in all, 20,000 values; and for
    every 2^31 / 2^32 / 2^33 boundary inside its input, output and residual a window which (for the input: whose
    halo box) holds the voxel that starts at the boundary and voxels before and after it."""
    row = big.row
    wins = E.case_windows(big)
    labels = [l for l, _ in wins]
    ydims = (row.B,) + E.y_dims(big)
    assert len(wins) >= 6 and E.window_values(row, wins) >= 20000
    assert labels[:2] == ["first", "last"] and sum(l.startswith("rand") for l in labels) >= 2
    assert wins[0][1][0] == 0 and all(lo == 0 for lo, _ in wins[0][1][1:])
    assert wins[1][1][0] == row.B - 1 and all(hi == n for (_, hi), n in zip(wins[1][1][1:], ydims[1:]))
    for _, (b, *box) in wins:
        assert 0 <= b < row.B and all(0 <= lo < hi <= n for (lo, hi), n in zip(box, ydims[1:]))
    tensors = {"y": (ydims, row.cout), "x": ((row.B,) + tuple(row.size), row.cin)}
    if big.res:
        tensors["r"] = ((row.B,) + E.res_dims(big), row.cout)
    if row.vol:
        del tensors["x"]                                 # the features are small: no boundary in the input
    want = set()
    for which, (dims, C) in tensors.items():
        total = 4 * C * dims[0] * dims[1] * dims[2] * dims[3]
        for bound in E.BOUNDARIES:
            if bound >= total:
                continue
            label = "%s@2^%d" % (which, bound.bit_length() - 1)
            want.add(label)
            win = dict(wins)[label]
            box = E.input_box(row, win) if which == "x" else win[1:]
            box = tuple((max(lo, 0), min(hi, n)) for (lo, hi), n in zip(box, dims[1:]))
            assert bound % (4 * C) == 0
            v = bound // (4 * C)                         # the first voxel past the boundary
            at = E.voxel_at(dims, C, bound)
            assert E.linear(dims, at) == v
            if which == "r" and big.res == "short":      # the residual's voxel may lie outside the output corner: nearest
                at = (at[0],) + tuple(min(c, n - 1) for c, n in zip(at[1:], ydims[1:]))
            else:
                assert at[0] == win[0] and all(lo <= c < hi for c, (lo, hi) in zip(at[1:], box)), (label, at, box)
            first = E.linear(dims, (win[0],) + tuple(lo for lo, _ in box))
            last = E.linear(dims, (win[0],) + tuple(hi - 1 for _, hi in box))
            assert first < v <= last, (label, first, v, last)
    assert {l for l in labels if "@" in l} == want
    # the cases together cross every boundary the issue lists
    if row.name.startswith("deconv3d_mfma"):
        assert {"y@2^31", "y@2^32", "y@2^33", "x@2^31"} <= want


def test_some_case_of_every_fp32_input_kernel_has_interior_tiles_past_2_gib():
    """The fp32-input kernels stage a tile whose halo box lies inside the volume through the buffer descriptor with a
    32-bit box offset, any other tile through 64-bit pointers.  For every such kernel among the cases, the input plane
    at which the last interior box of the last item starts (convolution: D - 3, stride 2: the last odd plane with two
    planes behind it, transposed: D - 2) must reach past 2^31 bytes: boxes with an offset of 2^31 and more exist."""
    names = {b.row.name for b in E.BIG_CASES
             if b.row.name.startswith(("conv3d_mfma", "conv3d_cout1", "deconv3d_mfma", "deconv3d_cout1"))}
    assert len(names) == 6, names
    for name in names:
        deep = []
        for r in (b.row for b in E.BIG_CASES if b.row.name == name):
            D = r.size[0]
            zb = D - 2 if r.tr else (D - 3 if r.stride == 1 else 2 * ((D - 2) // 2) - 1)
            plane = E.nbytes(1, r.cin, (1,) + tuple(r.size[1:]))
            deep.append(((r.B - 1) * D + zb + 1) * plane - 2 ** 31)
        assert max(deep) > 0, (name, deep)
        print(name, [v / 2 ** 20 for v in deep])


def test_find_window_returns_the_voxel_of_a_byte():
    dims, C = (2, 5, 7, 11), 32
    assert E.find_window(dims, C, 0, (3, 3, 3)) == ((0, 0, 0, 0), (0, (0, 3), (0, 3), (0, 3)))
    last = 4 * C * 2 * 5 * 7 * 11 - 1
    assert E.find_window(dims, C, last, (3, 3, 3)) == ((1, 4, 6, 10), (1, (2, 5), (4, 7), (8, 11)))
    v = (1, 2, 3, 4)
    byte = E.linear(dims, v) * 4 * C + 77
    assert E.find_window(dims, C, byte, (3, 4, 48)) == (v, (1, (1, 4), (1, 5), (0, 11)))


SMALL = [
    # (row, residual, relu): stride 1, stride 2 (odd and even sizes), transposed with the myadd_3d crop, one channel
    (R("s1", "f16x2", 16, 32, (5, 9, 13), B=2), "full", 1),
    (R("s2", "f16x2", 16, 32, (5, 10, 13), B=2, stride=2), "full", 2),
    (R("tr", "f16x2", 16, 32, (3, 5, 7), B=2, stride=2, tr=1), "short", 1),
    (R("tr", "f16x2", 16, 32, (3, 5, 7), B=1, stride=2, tr=1), None, 0),
    (R("c1", "f16x2", 16, 1, (4, 6, 9), B=1), None, 1),
]


@pytest.mark.parametrize("row,res,relu", SMALL, ids=[r[0].name + str(i) for i, r in enumerate(SMALL)])
def test_the_windowed_reference_equals_the_full_one(row, res, relu):
    """Windows at every face and corner of the volume, in the interior, and the whole output as one window."""
    from tests.test_conv_plans_gpu import reference, tensors
    big = E.Big(row, res, 0.0)
    x, w, sc, sh, _ = tensors(row, 300)
    rd = E.res_dims(big)
    r = None if rd is None else seeded(305, row.B, row.cout, *rd)
    full = reference(row, x, w, sc, sh, r, relu)
    ydims = (row.B,) + E.y_dims(big)
    assert tuple(full.shape[2:]) == ydims[1:]
    wins = [(b, (0, ydims[1]), (0, ydims[2]), (0, ydims[3])) for b in range(row.B)]
    corners = [(b, z, y, xx) for b in range(row.B) for z in (0, ydims[1] - 1) for y in (0, ydims[2] - 1)
               for xx in (0, ydims[3] - 1)]
    centre = (0,) + tuple(n // 2 for n in ydims[1:])
    wins += [E.window_around(ydims, v, (2, 3, 4)) for v in corners + [centre]]
    wins += [E.window_around(ydims, centre, (1, 1, 1)), E.window_around(ydims, centre, (3, 2, 5))]
    for win in wins:
        got = E.windowed_reference(row, row.size, E.tensor_fetch(x), w, sc, sh,
                                   None if r is None else E.tensor_fetch(r), relu, win)
        b, (z0, z1), (y0, y1), (x0, x1) = win
        assert (got - full[b:b + 1, :, z0:z1, y0:y1, x0:x1]).abs().max().item() <= 1e-12, win


def test_the_windowed_volume_equals_the_concatenation_volume():
    B, C, D, H, W = 2, 4, 6, 5, 9
    fL, fR = seeded(1, B, C, H, W), seeded(2, B, C, H, W)
    vol = OO.concat_volume(fL, fR, D, mask_left=False).double()
    fetch = E.volume_fetch(fL, fR)
    for box in [((0, D), (0, H), (0, W)), ((2, 5), (1, 4), (3, 8)), ((4, 6), (0, 2), (0, 3)), ((0, 1), (4, 5), (8, 9)),
                ((5, 6), (2, 5), (5, 9))]:
        for b in range(B):
            (z0, z1), (y0, y1), (x0, x1) = box
            assert torch.equal(fetch(b, box), vol[b:b + 1, :, z0:z1, y0:y1, x0:x1]), box
    row = R("vol", "f16x2", 2 * C, 32, (D, H, W), B=B, vol=1)
    from tests.test_conv_plans_gpu import reference
    w, sc, sh = seeded(3, 32, 2 * C, 3, 3, 3, scale=0.1), seeded(4, 32).abs() + 0.5, seeded(5, 32)
    full = reference(row, vol.float(), w, sc, sh, None, 1)
    win = (1, (3, 6), (2, 5), (0, 6))
    got = E.windowed_reference(row, row.size, fetch, w, sc, sh, None, 1, win)
    assert (got - full[1:2, :, 3:6, 2:5, 0:6]).abs().max().item() <= 1e-12
