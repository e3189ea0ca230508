"""CPU: the dispatch of ``dsm_conv3d_fwd`` (make_plan in dsmnet_amd/csrc/conv3d.hip), one table row per kernel
variant it can launch.

``dsm_conv3d_plan`` is host-only and shares its selection with the launch and with ``dsm_conv3d_workspace_bytes``
(one ``make_plan`` over one ``select_kernel``; the compiled variants are the lists of csrc/conv_common.hpp, from which the launch chains are
generated and which the plan consults), so a row that lands on a name here is a set of arguments whose launch
runs that kernel: tests/test_conv_plans_gpu.py imports ``CASES`` and launches every row against float64.  Pointers are fake addresses (16: aligned), never dereferenced.

* ``CASES``: every row names the exact variant its arguments must produce; natural thresholds of the planner have
  a row on each side, everything else is the smallest shape (a few ragged tiles) that reaches the name, through a
  flag field where a flag is the only small way in.
* a sweep over channel counts, geometry, precisions, flags and sizes collects every name the planner can produce:
  that set must equal the table's names (the sweep stops at 128 outputs: the wide, kind 8, names are pinned by
  tests/test_wide2d_plans.py; the mirror check adds wide points of its own).
* ``REFUSED``: argument sets whose variant is not compiled.  The plan must say DSM_ERR_UNSUPPORTED, as the launch
  does (before the variant lists were shared the plan answered OK with the name of a kernel that does not exist).
* the host layer's questions to the planner -- ``costvolume._split_kernel_layer`` (is the launch handed ``x_amax``),
  ``costvolume.conv2d_variant`` and ``blocks2d.fused_ok`` (is there a kernel for a 2-D layer) -- are answered by
  ``dsm_conv3d_plan`` itself, with stand-in addresses and on a copy of the struct; they agree with the plan on every
  point of the sweep, and the 2-D layers that have a kernel are pinned as a set."""
import collections
import ctypes
import itertools
import re

import pytest
import torch.nn as nn

from dsmnet_amd import _lib
from tests.test_wide2d_plans import FakeCudaMap, precision

A16 = 16
PREC = {"f16x2": (_lib.DSM_PREC_F16X2, 0), "f16": (_lib.DSM_PREC_F16, 0),
        "bf16x3": (_lib.DSM_PREC_F32, 0), "fp32": (_lib.DSM_PREC_F32, _lib.DSM_CONV_FP32_MFMA)}
SPLIT_MODES = ("bf16x3", "f16x2", "f16")
NO_NSPLIT, NO_ONCE, CHUNKED = _lib.DSM_CONV_NO_NSPLIT, _lib.DSM_CONV_NO_ONCE, _lib.DSM_CONV_COUT1_CHUNKED


def TM(t):
    return t << _lib.DSM_CONV_TM_SHIFT


# size: the input's (D, H, W) -- a 3-D layer -- or (H, W) -- a 2-D one (kd = 1).  tr: transposed (stride 2).
# flags: tuning bits of dsm_conv3d_args.flags on top of the mode's.  vol: the input is a virtual cost volume.
# grid: a persistent grid size to force as well (DSM_CONV_BLOCKS_SHIFT; it never changes the plan) where the
# kernel walks its tiles in a loop: smaller than the row's tile count, so that a workgroup takes several tiles.
Row = collections.namedtuple("Row", "name mode cin cout size B stride tr k dil flags vol grid")


def R(name, mode, cin, cout, size, B=1, stride=1, tr=0, k=3, dil=1, flags=0, vol=0, grid=0):
    return Row(name % mode if "%s" in name else name, mode, cin, cout, size, B, stride, tr, k, dil, flags, vol, grid)


CASES = [
    # ------------------------------------------------------------------ Cout = 1 heads (kinds 2, 3, 4; VALU)
    R("conv3d_cout1_zslide_kernel", "f16x2", 32, 1, (3, 9, 37), B=2),                  # Cin == 32
    R("conv3d_cout1_kernel<CK=8>", "bf16x3", 16, 1, (3, 9, 37)),                       # Cin != 32, below
    R("conv3d_cout1_kernel<CK=8>", "f16", 64, 1, (3, 9, 37), B=2),                     # ... and above
    R("conv3d_cout1_kernel<CK=8>", "fp32", 32, 1, (3, 9, 37), flags=CHUNKED),          # Cin == 32 by flag
    R("deconv3d_cout1_kernel", "fp32", 32, 1, (2, 5, 19), B=2, stride=2, tr=1),
    # ------------------------------------------------------------------ fp32-input MFMA, 3-D (kind 0)
    # big: B Do ceil(Ho / 8) ceil(Wo / 32) >= 1024 -- 32 * 8 * 4 = 1024 | 31 * 8 * 4 = 992
    R("conv3d_mfma_kernel<S=1,NT=1,TM=2,CK=16>", "fp32", 16, 32, (32, 60, 100)),
    R("conv3d_mfma_kernel<S=1,NT=1,TM=1,CK=16>", "fp32", 16, 32, (31, 60, 100), grid=96),
    R("conv3d_mfma_kernel<S=1,NT=1,TM=1,CK=16>", "fp32", 32, 32, (3, 7, 37), B=2),
    R("conv3d_mfma_kernel<S=1,NT=2,TM=2,CK=8>", "fp32", 16, 64, (3, 11, 37), B=2, flags=TM(2)),
    # tiles4 = B Do ceil(Ho / 4) ceil(Wo / 32) <= 64: one workgroup column per 32 outputs -- 4 * 4 * 4 | 5 * 4 * 4
    R("conv3d_mfma_kernel<S=1,NT=1,TM=1,CK=16>x2", "fp32", 16, 64, (4, 14, 100)),
    R("conv3d_mfma_kernel<S=1,NT=2,TM=1,CK=16>", "fp32", 16, 64, (5, 14, 100)),
    R("conv3d_mfma_kernel<S=1,NT=1,TM=1,CK=16>x4", "fp32", 16, 128, (3, 7, 37), B=2),
    # 128 outputs in the split modes: t4 <= 128 takes four split columns (below), 9 * 4 * 4 = 144 this kernel
    R("conv3d_mfma_kernel<S=1,NT=4,TM=1,CK=16>", "f16x2", 16, 128, (9, 14, 100)),
    R("conv3d_mfma_kernel<S=2,NT=1,TM=1,CK=8>", "f16", 16, 32, (5, 11, 67), B=2, stride=2),
    R("conv3d_mfma_kernel<S=2,NT=1,TM=1,CK=8>x2", "fp32", 16, 64, (7, 27, 199), stride=2),     # out 4 x 14 x 100: 64
    R("conv3d_mfma_kernel<S=2,NT=2,TM=1,CK=8>", "fp32", 16, 64, (9, 27, 199), stride=2),       # out 5 x 14 x 100: 80
    R("conv3d_mfma_kernel<S=2,NT=1,TM=1,CK=8>x4", "f16x2", 16, 128, (5, 11, 67), B=2, stride=2),
    R("conv3d_mfma_kernel<S=2,NT=4,TM=1,CK=8>", "f16", 16, 128, (9, 27, 199), stride=2, grid=24),
    # ------------------------------------------------------------------ fp32-input MFMA, 2-D (kind 0)
    # big: 2 * ceil(250 / 8) * ceil(500 / 32) = 2 * 32 * 16 = 1024 | 2 * 31 * 16 = 992
    R("conv2d_mfma_kernel<S=1,NT=1,TM=2,K=3,DIL=1>", "fp32", 16, 32, (250, 500), B=2),
    R("conv2d_mfma_kernel<S=1,NT=1,TM=1,K=3,DIL=1>", "fp32", 16, 32, (248, 500), B=2),
    R("conv2d_mfma_kernel<S=1,NT=1,TM=1,K=3,DIL=1>", "fp32", 32, 32, (11, 37), grid=2),
    R("conv2d_mfma_kernel<S=1,NT=2,TM=1,K=3,DIL=1>", "fp32", 16, 64, (11, 37), B=2),
    R("conv2d_mfma_kernel<S=1,NT=4,TM=1,K=3,DIL=1>", "fp32", 16, 128, (11, 37)),
    R("conv2d_mfma_kernel<S=1,NT=4,TM=1,K=3,DIL=2>", "fp32", 32, 128, (11, 37), B=2, dil=2),
    R("conv2d_mfma_kernel<S=2,NT=1,TM=1,K=3,DIL=1>", "f16x2", 16, 32, (21, 75), stride=2),
    R("conv2d_mfma_kernel<S=2,NT=2,TM=1,K=3,DIL=1>", "f16", 32, 64, (21, 75), B=2, stride=2),
    R("conv2d_mfma_kernel<S=1,NT=1,TM=1,K=1,DIL=1>", "f16x2", 32, 32, (11, 37), B=2, k=1),
    R("conv2d_mfma_kernel<S=1,NT=4,TM=1,K=1,DIL=1>", "f16", 64, 128, (11, 37), k=1),
    R("conv2d_mfma_kernel<S=2,NT=2,TM=1,K=1,DIL=1>", "f16x2", 64, 64, (21, 75), B=2, stride=2, k=1),
    # ------------------------------------------------------------------ transposed, fp32 input (kind 1)
    R("deconv3d_mfma_kernel<NT=1,CK=16>", "f16x2", 48, 32, (2, 5, 19), B=2, stride=2, tr=1),   # Cin % 32 != 0
    R("deconv3d_mfma_kernel<NT=2,CK=16>", "bf16x3", 16, 64, (2, 5, 19), stride=2, tr=1, grid=3),
    R("deconv3d_mfma_kernel<NT=2,CK=16>", "fp32", 32, 64, (2, 5, 19), B=2, stride=2, tr=1),    # Cin % 32 == 0 by flag
]
for _m in SPLIT_MODES:
    _f16 = _m != "bf16x3"
    CASES += [
        # -------------------------------------------------------------- z-sliding, 32 outputs (kind 7)
        R("conv3d_zs_%s_mfma_kernel", _m, 32, 32, (3, 11, 37), B=2, grid=3),           # Cin % 32 == 0 (48: below)
        R("conv3d_zs_%s_mfma_kernel<vol>", _m, 64, 32, (5, 9, 37), vol=1),
        # -------------------------------------------------------------- transposed split (kind 6)
        R("deconv3d_%s_mfma_kernel<NT=1>", _m, 32, 32, (2, 5, 19), B=2, stride=2, tr=1, grid=5),
        R("deconv3d_%s_mfma_kernel<NT=2>", _m, 96 if _f16 else 32, 64, (2, 5, 19), stride=2, tr=1),   # Cin % 64 != 0
        # -------------------------------------------------------------- split 3-D (kind 5)
        R("conv3d_%s_mfma_kernel<S=2,NT=2,TM=1>", _m, 16, 64, (5, 11, 67), B=2, stride=2, grid=4),
        # tiles16 = B Do ceil(Ho / 16) ceil(Wo / 32) >= 224 -- 14 * 2 * 8 | 13 * 2 * 8 (one mode; TM flag elsewhere)
        R("conv3d_%s_mfma_kernel<NT=1,TM=4>", _m, 16, 32, (14, 20, 250)) if _m == "f16x2" else
        R("conv3d_%s_mfma_kernel<NT=1,TM=4>", _m, 48, 32, (3, 19, 37), B=2, flags=TM(4)),
        R("conv3d_%s_mfma_kernel<NT=1,TM=2>", _m, 16, 32, (13, 20, 250)) if _m == "f16x2" else
        R("conv3d_%s_mfma_kernel<NT=1,TM=2>", _m, 48, 32, (3, 11, 37), B=2),           # Cin % 32 != 0: not z-sliding
        # tiles8 >= 192: 8-row tiles -- 2 * 8 * 3 * 4 = 192 | 15 * 3 * 4 = 180 (4-row tiles: 300 > 256, unsplit)
        R("conv3d_%s_mfma_kernel<NT=2,TM=2>", _m, 16, 64, (8, 20, 100), B=2) if _m == "f16x2" else
        R("conv3d_%s_mfma_kernel<NT=2,TM=2>", _m, 32, 64, (3, 11, 37), B=2, flags=TM(2)),
        R("conv3d_%s_mfma_kernel<NT=2,TM=1>", _m, 16, 64, (15, 20, 100)) if _m == "f16x2" else
        R("conv3d_%s_mfma_kernel<NT=2,TM=1>", _m, 32, 64, (3, 7, 37), B=2, flags=NO_NSPLIT),
        R("conv3d_%s_mfma_kernel<NT=1,TM=1>x2", _m, 16, 64, (3, 7, 37), B=2, grid=2),
        # 128 outputs: t4 <= 128 -- 8 * 4 * 4 (one mode); 9 * 4 * 4 is the fp32-input row above
        R("conv3d_%s_mfma_kernel<NT=1,TM=1>x4", _m, 16, 128, (8, 14, 100)) if _m == "f16x2" else
        R("conv3d_%s_mfma_kernel<NT=1,TM=1>x4", _m, 32, 128, (3, 7, 37), B=2),
        # -------------------------------------------------------------- split 2-D (kind 5, KZ = 1)
        # tiles16 >= 224: 2 * ceil(110 / 16) * ceil(500 / 32) = 2 * 7 * 16 | 2 * 6 * 16 = 192
        R("conv2d_%s_mfma_kernel<NT=1,TM=4,DIL=1>", _m, 16, 32, (110, 500), B=2) if _m == "f16x2" else
        R("conv2d_%s_mfma_kernel<NT=1,TM=4,DIL=1>", _m, 32, 32, (19, 37), B=2, flags=TM(4)),
        R("conv2d_%s_mfma_kernel<NT=1,TM=2,DIL=1>", _m, 16, 32, (96, 500), B=2) if _m == "f16x2" else
        R("conv2d_%s_mfma_kernel<NT=1,TM=2,DIL=1>", _m, 32, 32, (11, 37), B=2),
        # 64 outputs: tiles8 < 192 runs 4-row tiles in 2-D as in 3-D (the line does not look at kd)
        R("conv2d_%s_mfma_kernel<NT=2,TM=1,DIL=1>", _m, 16, 64, (11, 37), B=2, grid=2),
        R("conv2d_%s_mfma_kernel<NT=2,TM=2,DIL=1>", _m, 32, 64, (11, 37), B=2, flags=TM(2) | NO_NSPLIT),
        R("conv2d_%s_mfma_kernel<NT=1,TM=2,DIL=1>x2", _m, 16, 64, (11, 37), B=2, flags=TM(2), grid=1),
        R("conv2d_%s_mfma_kernel<NT=4,TM=2,DIL=1>", _m, 16, 128, (11, 37), B=2, flags=NO_NSPLIT),
        R("conv2d_%s_mfma_kernel<NT=2,TM=2,DIL=1>x2", _m, 32, 128, (11, 37), B=2),
        R("conv2d_%s_mfma_kernel<NT=4,TM=2,DIL=2>", _m, 16, 128, (11, 37), B=2, dil=2),
    ]
    if _f16:
        CASES += [
            R("deconv3d_zs_%s_mfma_kernel<NT=1>", _m, 64, 32, (2, 5, 19), B=2, stride=2, tr=1, grid=3),   # Cin % 64 == 0
            R("deconv3d_zs_%s_mfma_kernel<NT=2>", _m, 64, 64, (2, 5, 19), stride=2, tr=1),
            R("conv3d_%s_mfma_kernel<S=2,NT=2,TM=1>", _m, 32, 64, (5, 11, 67), stride=2, flags=NO_ONCE, grid=4),
            R("conv2d_%s_mfma_kernel<NT=1,TM=2,DIL=1>x2,once", _m, 64, 64, (11, 37), B=2, flags=TM(2)),   # Cin == 64
            R("conv2d_%s_mfma_kernel<NT=1,TM=2,DIL=1>x2", _m, 64, 64, (11, 37), flags=TM(2) | NO_ONCE),
        ]
    else:
        CASES += [R("conv2d_%s_mfma_kernel<NT=1,TM=2,DIL=1>x2", _m, 64, 64, (11, 37), flags=TM(2))]   # no `once` on bf16x3
# The 64-output 2-D window, natural (f16x2): tiles8 = 2 ceil(H / 8) ceil(250 / 32) -- H 82: 176 < 192, 4-row tiles;
# H 90: 192 and H 122: 256, two columns of 8-row tiles (`once` from 64 inputs exactly); H 130: 272, unsplit.
# The 3-D 4-row split: t4 = 2 * 8 * 4 * 4 = 256 in two columns, 13 * 5 * 4 = 260 unsplit.
CASES += [
    R("conv2d_f16x2_mfma_kernel<NT=2,TM=1,DIL=1>", "f16x2", 64, 64, (82, 250), B=2),
    R("conv2d_f16x2_mfma_kernel<NT=1,TM=2,DIL=1>x2,once", "f16x2", 64, 64, (90, 250), B=2),
    R("conv2d_f16x2_mfma_kernel<NT=1,TM=2,DIL=1>x2", "f16x2", 48, 64, (90, 250), B=2),
    R("conv2d_f16x2_mfma_kernel<NT=1,TM=2,DIL=1>x2", "f16x2", 80, 64, (122, 250), B=2),
    R("conv2d_f16x2_mfma_kernel<NT=2,TM=2,DIL=1>", "f16x2", 16, 64, (130, 250), B=2),
    R("conv2d_f16x2_mfma_kernel<NT=2,TM=2,DIL=1>x2", "f16x2", 16, 128, (122, 250), B=2),
    R("conv2d_f16x2_mfma_kernel<NT=4,TM=2,DIL=1>", "f16x2", 16, 128, (130, 250), B=2),
    R("conv3d_f16x2_mfma_kernel<NT=1,TM=1>x2", "f16x2", 16, 64, (8, 14, 100), B=2),
    R("conv3d_f16x2_mfma_kernel<NT=2,TM=1>", "f16x2", 16, 64, (13, 20, 100)),
]
del _m, _f16

# Arguments whose variant is not compiled: (mode, cin, cout, size, stride, k, dil, flags).  Stride 2 halves the size.
REFUSED = [("fp32", 16, 32 * nt, (11, 37), s, k, dil, 0) for s, nt, k, dil in [
    (1, 1, 1, 2), (1, 1, 3, 2), (1, 2, 1, 1), (1, 2, 1, 2), (1, 2, 3, 2), (1, 4, 1, 2),
    (2, 1, 1, 1), (2, 1, 1, 2), (2, 1, 3, 2), (2, 2, 1, 2), (2, 2, 3, 2),
    (2, 4, 1, 1), (2, 4, 1, 2), (2, 4, 3, 1), (2, 4, 3, 2)]]
REFUSED += [("bf16x3", 16, 128, (9, 14, 100), 1, 3, 1, TM(2))]      # 128 outputs, t4 = 144, forced 8-row tiles
REFUSED += [(m, 16, cout, (11, 37), 1, 3, 2, 0) for m in SPLIT_MODES for cout in (32, 64)]
assert len(REFUSED) == 22


def row_id(r):
    """The pytest id of a row, here and in the GPU module; DESIGN.md 3.2h names rows by it."""
    return "%s-%s-c%d-%s-b%d%s" % (r.name, r.mode, r.cin, "x".join(map(str, r.size)), r.B,
                                   "-f%x" % r.flags if r.flags else "")


assert len({row_id(r) for r in CASES}) == len(CASES)


def min_units(r):
    """A lower bound of the work units the row's kernel walks: 32 columns by 4 TM rows where the name carries TM,
    by at most 4 rows in the transposed kernels (deconv3d_mfma / split: 4, z-sliding: 2) and at most 8 in the
    z-sliding convolution (6 or 8), one plane deep, over the output -- the transposed kernels tile the input."""
    tm = [int(v) for v in re.findall(r"TM=(\d)", r.name)]
    ty = 4 * tm[0] if tm else (4 if r.name.startswith("deconv3d_") else 8)
    dims = r.size if r.tr else tuple((v - 1) // r.stride + 1 for v in r.size)
    d, h, w = dims if len(dims) == 3 else (1,) + tuple(dims)
    return r.B * d * -(-h // ty) * -(-w // 32)


def make_args(mode, cin, cout, size, B=1, stride=1, tr=0, k=3, dil=1, flags=0, vol=0):
    a = _lib.Conv3dArgs()
    a.x = a.w_packed = a.y = a.x_amax = A16
    a.B, a.Cin, a.Cout = B, cin, cout
    if len(size) == 2:
        a.Di, a.kd, a.k, a.dil = 1, 1, k, dil
        a.Hi, a.Wi = size
    else:
        a.Di, a.Hi, a.Wi = size
    a.Do, a.Ho, a.Wo = [2 * v if tr else (v - 1) // stride + 1 for v in (a.Di, a.Hi, a.Wi)]
    a.stride, a.transposed, a.relu = stride, tr, 1
    a.precision, fl = PREC[mode]
    a.flags = fl | flags
    a.vol_virtual = vol
    return a


def row_args(row):
    return make_args(row.mode, row.cin, row.cout, row.size, row.B, row.stride, row.tr, row.k, row.dil, row.flags,
                     row.vol)


def plan(hip_lib, a):
    buf = ctypes.create_string_buffer(96)
    rc = hip_lib.dsm_conv3d_plan(ctypes.byref(a), buf, 96)
    return rc, buf.value.decode()


SIZES_3D = [(1, 1, 1), (6, 12, 40), (12, 24, 80), (14, 64, 128), (24, 64, 128), (5, 9, 37), (48, 64, 128), (3, 8, 33),
            (4, 16, 64)]
SIZES_2D = [(1, 1), (24, 40), (96, 320), (190, 630), (12, 40), (64, 128), (7, 35), (250, 500)]


def sweep():
    """(args, what) over channel counts x geometry x precisions x flags x sizes: 3-D conv / strided / transposed,
    2-D with k, dilation and stride, forced tile heights, the A/B flags, a virtual volume, B = 1 and 2."""
    flagsets = [TM(t) | f for t in (0, 1, 2, 4) for f in (0, NO_NSPLIT, CHUNKED, NO_ONCE)]
    for mode, flags, cin, cout, B in itertools.product(PREC, flagsets, (16, 32, 48, 64, 128, 320), (1, 32, 64, 128),
                                                       (1, 2)):
        for (stride, tr), size in itertools.product(((1, 0), (2, 0), (2, 1)), SIZES_3D):
            for vol in ((0, 1) if stride == 1 and cout == 32 else (0,)):
                yield make_args(mode, cin, cout, size, B, stride, tr, flags=flags, vol=vol), \
                    (mode, flags, cin, cout, B, size, stride, tr, vol)
        if cout > 1:
            for k, dil, stride, size in itertools.product((1, 3), (1, 2), (1, 2), SIZES_2D):
                yield make_args(mode, cin, cout, size, B, stride, 0, k, dil, flags), \
                    (mode, flags, cin, cout, B, size, stride, k, dil)


@pytest.fixture(scope="module")
def swept(hip_lib):
    """name -> one argument set that produced it; and the (args, rc, name) list of the fp16 modes."""
    names, f16_points = {}, []
    for a, what in sweep():
        rc, name = plan(hip_lib, a)
        assert (rc == 0) == bool(name), what
        assert rc in (0, -2), (rc, what)
        if rc == 0:
            names.setdefault(name, what)
            if what[0] in ("f16x2", "f16"):
                f16_points.append((a, name, what))
    return names, f16_points


@pytest.mark.parametrize("row", CASES, ids=row_id)
def test_every_row_lands_on_the_variant_it_names(hip_lib, row):
    assert plan(hip_lib, row_args(row)) == (0, row.name)
    forced = row_args(row)
    forced.flags |= 7 << _lib.DSM_CONV_BLOCKS_SHIFT                     # a forced grid never changes the plan
    assert plan(hip_lib, forced) == (0, row.name)
    assert hip_lib.dsm_conv3d_workspace_bytes(ctypes.byref(row_args(row))) == 0


def test_a_forced_grid_is_smaller_than_the_tile_count():
    """Rows with ``grid`` are launched with that persistent grid as well (the GPU module): a workgroup must then
    walk several tiles, which needs fewer workgroups than tiles; every looping kernel family has such a row."""
    forced = [r for r in CASES if r.grid]
    for r in forced:
        assert 0 < r.grid < min_units(r), (row_id(r), min_units(r))
    families = {r.name.split("<")[0].replace(r.mode, "%s") for r in forced}
    assert families >= {"conv3d_mfma_kernel", "conv2d_mfma_kernel", "deconv3d_mfma_kernel", "conv3d_zs_%s_mfma_kernel",
                        "deconv3d_%s_mfma_kernel", "deconv3d_zs_%s_mfma_kernel", "conv3d_%s_mfma_kernel",
                        "conv2d_%s_mfma_kernel"}, families
    assert any("_%s_mfma_kernel<S=2" % r.mode in r.name for r in forced)            # the stride-2 split kernel


def test_the_design_table_lists_every_row():
    """one table line per name, its last column the id suffixes of the name's rows."""
    import os
    lines = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read().split("\n")
    for name in {r.name for r in CASES}:
        line = [ln for ln in lines if ln.startswith("| `%s` |" % name)]
        assert len(line) == 1, name
        want = "; ".join("`%s`" % row_id(r)[len(name) + 1:] for r in CASES if r.name == name)
        assert line[0].endswith("| %s |" % want), (name, want)


def test_the_table_has_a_row_for_every_name_the_planner_can_produce(swept):
    names, _ = swept
    table = {r.name for r in CASES}                # the sweep stops at 128 outputs: no wide (kind 8) name in it
    assert set(names) == table, (sorted(set(names) - table), sorted(table - set(names)))
    assert len(table) == 90


@pytest.mark.parametrize("mode,cin,cout,size,stride,k,dil,flags", REFUSED)
def test_a_variant_that_is_not_compiled_is_refused_by_the_plan(hip_lib, mode, cin, cout, size, stride, k, dil, flags):
    a = make_args(mode, cin, cout, size, 1, stride, 0, k, dil, flags)
    assert plan(hip_lib, a) == (-2, "")
    assert hip_lib.dsm_conv3d_workspace_bytes(ctypes.byref(a)) == 0


def test_split_kernel_layer_mirrors_the_plan(hip_lib, swept):
    """``_split_kernel_layer`` decides whether a launch is handed ``x_amax`` in the fp16 modes: False where the
    plan picks a split kernel fails the call (DSM_ERR_ARG), True where it does not wastes an absmax pass."""
    from dsmnet_amd import costvolume as cv
    _, points = swept
    assert len(points) > 10000
    # the sweep stops at 128 outputs: the wide layers (kind 8; tests/test_wide2d_plans.py pins their names) on top
    wide = [(make_args(mode, cin, cout, size, B, stride), (mode, cin, cout, B, size, stride))
            for mode, cin, cout, B, size, stride in itertools.product(("f16x2", "f16"), (128, 256), (256, 512, 1024),
                                                                      (1, 2), ((12, 40), (7, 35)), (1, 2))]
    points = points + [(a, plan(hip_lib, a)[1], what) for a, what in wide]
    assert sum(name.startswith("conv2d_wide_") for _, name, _ in points) == len(wide)
    for a, name, what in points:
        split = "_f16x2_" in name or "_f16_" in name
        assert cv._split_kernel_layer(a) == split, (name, what)


def test_split_kernel_layer_asks_with_a_copy_and_needs_no_x_amax(hip_lib):
    """The launch path asks before it has an ``x_amax``: the struct it hands over comes back untouched, and the
    answer is the one a stand-in maximum gives."""
    from dsmnet_amd import costvolume as cv
    for row in CASES:
        a, b = row_args(row), row_args(row)
        a.x_amax = None
        before = bytes(a)
        assert cv._split_kernel_layer(a) == cv._split_kernel_layer(b) == ("_f16x2_" in row.name or "_f16_" in row.name)
        assert bytes(a) == before and a.x_amax is None


def test_split_kernel_layer_is_false_for_a_refused_plan(hip_lib):
    from dsmnet_amd import costvolume as cv
    for mode, cin, cout, size, stride, k, dil, flags in REFUSED:
        a = make_args(mode, cin, cout, size, 1, stride, 0, k, dil, flags)
        assert plan(hip_lib, a)[0] == -2 and cv._split_kernel_layer(a) is False


@pytest.mark.parametrize("mode", list(PREC))
def test_fused_ok_and_the_variant_set_mirror_the_plan(hip_lib, mode):
    from dsmnet_amd import blocks2d, costvolume as cv
    ok_keys = set()
    with precision(mode):
        for cout, k, s, dil, cin in itertools.product((32, 64, 128), (1, 3), (1, 2), (1, 2), (16, 64)):
            conv = nn.Conv2d(cin, cout, k, s, padding=dil * (k - 1) // 2, dilation=dil)
            rcs = {plan(hip_lib, make_args(mode, cin, cout, size, B, s, 0, k, dil))[0]
                   for size in SIZES_2D for B in (1, 2)}
            assert len(rcs) == 1, (mode, cout, k, s, dil, rcs)              # no size decides whether a layer can run
            ok = blocks2d.fused_ok(conv, FakeCudaMap(1, cin, 12, 40))
            assert ok == (rcs == {0}), (mode, cin, cout, k, s, dil, ok, rcs)
            assert cv.conv2d_variant(cout, s, k, dil) == ok
            if ok:
                ok_keys.add((s, cout // 32, k, dil))
    # (stride, Cout / 32, k, dilation) of the 2-D layers that have a kernel, the same in every precision mode
    assert ok_keys == {(1, 1, 3, 1), (1, 2, 3, 1), (1, 4, 3, 1), (1, 4, 3, 2), (2, 1, 3, 1),
                       (2, 2, 3, 1), (1, 1, 1, 1), (1, 4, 1, 1), (2, 2, 1, 1)}
