"""CPU: the host-only plan queries (``dsm_corr1d_plan``, ``dsm_soft_argmin_{fwd,bwd}_plan``,
``dsm_concat_volume_{fwd,bwd}_plan``) send every case of the dispatch-coverage table to the branch the
table names, and the table reaches every branch the host code can take.

The tables below are the single source of the cases: tests/test_dispatch_gpu.py runs the same rows
against the float64 oracle on the GPU.  The plan queries share their selection code with the
launches (one ``pick_*`` function each in the .hip files), so a row that lands on a branch here is a
row whose parity test runs that branch's kernel.  Pointers are fake addresses (16: aligned, 20: one
float past a 16-byte boundary); a plan query never dereferences them."""
import collections

import pytest

from dsmnet_amd import _lib

A16, OFF4 = 16, 20          # fake device addresses: 16-byte aligned / offset by one float

# ------------------------------------------------------------------------------------ corr1d --
# shape (B, C, H, W) of fL and fR.  ``offset``: the inputs are contiguous views one float into a larger
# buffer (16-byte MISaligned although W % 4 == 0).
Corr = collections.namedtuple("Corr", "shape D s k offset plan")
CORR_CASES = [
    Corr((2, 16, 3, 72), 41, 1, 1, False, "tile<1,1>"),        # B = 2, ragged x-tile of 8 live columns, one channel group per quarter
    Corr((2, 48, 2, 24), 41, 1, 1, False, "tile<1,1>"),        # W < 64, D > W, three channel groups per quarter
    Corr((1, 32, 2, 128), 5, 1, 1, False, "tile<1,1>"),        # D < 12: one d-group lane row does all the work
    Corr((1, 16, 2, 68), 48, 1, 1, False, "tile<1,1>"),        # the four-wave / eight-wave boundary
    Corr((1, 16, 2, 68), 49, 1, 1, False, "tile<1,2>"),
    Corr((2, 48, 2, 200), 96, 1, 1, False, "tile<1,2>"),       # top of the tile kernel, B = 2, ragged W
    Corr((2, 48, 2, 200), 97, 1, 1, False, "fwd<1>vec"),
    Corr((2, 32, 3, 40), 7, 2, 3, False, "tile<2,1>+box3"),    # box3 at B = 2
    Corr((2, 64, 3, 160), 81, 2, 1, False, "tile<2,2>"),       # planes with shift >= W
    Corr((2, 64, 3, 160), 81, 2, 3, False, "tile<2,2>+box3"),
    Corr((1, 160, 2, 64), 81, 2, 1, False, "fwd<2>vec"),       # the window (160 KB) does not fit: five channel chunks
    Corr((1, 20, 3, 64), 41, 1, 1, False, "fwd<1>vec"),        # C % 16 != 0, partial chunk
    Corr((2, 40, 2, 68), 41, 1, 1, False, "fwd<1>vec"),
    Corr((1, 16, 2, 132), 128, 1, 1, False, "fwd<1>vec"),      # 16 d-groups: the 256-thread limit
    Corr((1, 16, 2, 132), 129, 1, 1, False, "generic"),
    Corr((1, 8, 2, 40), 200, 1, 1, False, "generic"),          # D > W through the generic kernel
    Corr((1, 8, 2, 30), 9, 2, 1, False, "fwd<2>scalar"),       # W % 4 != 0 at stride 2
    Corr((2, 16, 3, 72), 41, 1, 3, True, "fwd<1>scalar+box"),  # misaligned inputs: no 16-byte access anywhere
]
# A correlation kernel and the box filter that may follow it are separate launches (the filter reads
# the raw volume whichever kernel wrote it), so the reachable set is kernels x suffixes, and the table
# has to reach every member of each factor.
CORR_KERNELS = {"tile<1,1>", "tile<1,2>", "tile<2,1>", "tile<2,2>", "fwd<1>vec", "fwd<1>scalar",
                "fwd<2>vec", "fwd<2>scalar", "generic"}
CORR_SUFFIXES = {"", "+box3", "+box"}

# ------------------------------------------------------------------------------- soft-argmin --
# cost shape (B, 1, Dc, Hc, Wc); out size (D, H, W) or None (GCNet form, negate).
Sa = collections.namedtuple("Sa", "cshape osize negate align fwd bwd")
SA_CASES = [
    Sa((2, 1, 2, 4, 6), (3, 9, 13), False, False, "fwd<true,1>", "bwd_tile nseg=1"),      # upsampling, D < 4
    Sa((1, 1, 3, 4, 6), (6, 8, 12), False, False, "fwd<true,2>", "bwd_tile nseg=1"),      # upsampling, 4 <= D < 8
    Sa((2, 1, 6, 5, 9), None, True, False, "fwd<false,2>", "bwd_direct"),
    Sa((2, 1, 3, 5, 9), None, True, False, "fwd<false,1>", "bwd_direct"),
    Sa((1, 1, 9, 3, 5), None, True, False, "fwd<false,4>", "bwd_direct"),
    Sa((1, 1, 1, 3, 5), None, True, False, "fwd<false,1>", "bwd_direct"),                 # D = 1
    Sa((1, 1, 1, 3, 5), (1, 6, 10), False, False, "fwd<true,1>", "bwd_tile nseg=1"),      # D = 1, H and W x2
    Sa((2, 1, 4, 3, 5), (16, 12, 20), False, False, "up4<4>", "bwd_tile nseg=2"),         # Dc = 4: one plane per lane segment
    Sa((1, 1, 7, 4, 6), (28, 16, 24), False, False, "up4<4>", "bwd_tile nseg=2"),         # Dc = 7: the last segment is short
    Sa((1, 1, 5, 4, 6), (20, 16, 24), False, False, "up4<4>", "bwd_tile nseg=2"),         # Dc = 5: the last segment is empty
    Sa((1, 1, 6, 5, 9), (24, 5, 9), False, False, "up4<4>", "bwd_tile nseg=2"),           # D x4, H and W unchanged
    Sa((1, 1, 6, 5, 9), (24, 13, 30), False, False, "up4<4>", "bwd_tile nseg=2"),         # non-integer H, W scales
    Sa((2, 1, 13, 6, 70), (52, 24, 280), False, False, "up4<4>", "bwd_tile nseg=2"),      # 9 x 3 backward tiles, B = 2
    # the segment-count boundaries of the tiled adjoint (align_corners where D == 4 Dc would be the x4 head)
    Sa((1, 1, 5, 4, 6), (15, 8, 12), False, False, "fwd<true,4>", "bwd_tile nseg=1"),
    Sa((1, 1, 4, 4, 6), (16, 8, 12), False, True, "fwd<true,4>", "bwd_tile nseg=2"),
    Sa((1, 1, 24, 4, 6), (95, 8, 12), False, False, "fwd<true,4>", "bwd_tile nseg=2"),
    Sa((1, 1, 24, 4, 6), (96, 8, 12), False, True, "fwd<true,4>", "bwd_tile nseg=4"),
    Sa((1, 1, 25, 4, 6), (97, 8, 12), False, False, "fwd<true,4>", "bwd_tile nseg=4"),    # segments of 25, 25, 25, 22
    # down-sampling by 8 in H and W: sw = sh = 8, sd = 1, one segment of 8 disparities, so
    # cells = (31*8 + 3) * (7*8 + 3) * (7*1 + 3) = 251 * 59 * 10 = 148090 floats = 592 KB > 48 KB
    Sa((1, 1, 8, 40, 200), (8, 5, 25), False, False, "fwd<true,4>", "bwd_fallback"),
]
SA_FWD_NAMES = {"up4<4>", "fwd<true,4>", "fwd<true,2>", "fwd<true,1>", "fwd<false,4>", "fwd<false,2>", "fwd<false,1>"}
SA_BWD_NAMES = {"bwd_direct", "bwd_tile nseg=1", "bwd_tile nseg=2", "bwd_tile nseg=4", "bwd_fallback"}
# Not reachable, with the argument (pick_sa_fwd in csrc/soft_argmin.hip): the x4 head needs D == 4 Dc and
# Dc >= DS with DS = 4 for D >= 8, 2 for 4 <= D < 8, 1 for D < 4.  DS = 2 forces D = 4, Dc = 1 < 2; DS = 1
# forces D < 4, which is no multiple of four.  The two launches were removed from the host code.
SA_FWD_UNREACHABLE = {"up4<2>", "up4<1>"}

# ------------------------------------------------------------------------------ concat volume --
# mode: False / True = mask_left of concat_volume; "right" = concat_volume_right (forward only).
# plan None: the wrapper must refuse with ``error`` (a DSM_ERR_* code) and launch nothing.
Vol = collections.namedtuple("Vol", "shape D channels_last mode fwd bwd error")
VOL_CASES = [
    Vol((1, 64, 2, 40), 192, True, False, "ndhwc lds>64K", "ndhwc_bwd", 0),     # (64 + 191) * 68 * 4 = 69360 B of LDS
    Vol((1, 64, 2, 40), 192, True, True, "ndhwc lds>64K", "ndhwc_bwd", 0),
    Vol((1, 64, 2, 40), 192, True, "right", "ndhwc lds>64K", None, 0),
    Vol((1, 160, 2, 8), 192, True, True, None, "ndhwc_bwd", -2),                # (64 + 191) * 164 * 4 = 167280 B > 160 KB
    Vol((2, 8, 3, 37), 6, True, True, "ndhwc", "ndhwc_bwd", 0),
    Vol((1, 3, 2, 20), 5, False, True, "ncdhw vec", "ncdhw_bwd", 0),            # C % 4 != 0 is fine in NCDHW
    Vol((1, 3, 2, 20), 5, True, True, None, None, -2),                          # ... and refused in NDHWC
    Vol((1, 4, 30, 37), 3, False, False, "ncdhw scalar", "ncdhw_bwd", 0),       # H * W = 1110 > 1024: two y-blocks
    Vol((1, 4, 30, 37), 3, False, True, "ncdhw scalar", "ncdhw_bwd", 0),
]
VOL_FWD_NAMES = {"ndhwc", "ndhwc lds>64K", "ncdhw vec", "ncdhw scalar"}
VOL_BWD_NAMES = {"ndhwc_bwd", "ncdhw_bwd"}

# ------------------------------------------------------------------------- fused train-mode BN --
# (no kernel choice: the rows pin grid-stride loops and lane maps.)  y (B, C, D, H, W), residual
# spatial size or None.
Bn = collections.namedtuple("Bn", "C yshape rshape relu")
BN_CASES = [
    Bn(32, (1, 6, 48, 64), None, 1),              # 18432 voxels > 512 blocks * 32 voxel lanes: the reductions stride twice
    Bn(64, (2, 3, 40, 40), (3, 40, 40), 1),       # 9600 voxels > 512 * 16
    Bn(128, (2, 1, 9, 33), (1, 9, 33), 1),        # the towers' width, a 2-D view
    Bn(12, (2, 3, 7, 11), None, 1),               # 3 quads: 85 voxel lanes, thread 255 idle, quad_of by modulo
    Bn(4, (1, 2, 5, 9), (2, 5, 9), 2),
    Bn(256, (1, 2, 3, 5), None, 0),               # the widest the ABI takes: 4 voxel lanes, 512 sums by 256 threads
    Bn(64, (2, 4, 8, 20), (3, 7, 19), 1),         # cropped residual at B = 2
]
# the element-wise passes cap their grid at 4096 blocks when an absolute maximum is asked for: their
# index counts QUADS (out voxels * C / 4); 138240 voxels * 8 quads = 1105920 = 4320 blocks of 256
BN_CAP_CASE = Bn(32, (1, 9, 96, 160), (9, 96, 160), 1)


def _ptr(v):
    import ctypes
    return None if v is None else ctypes.c_void_p(v)


def corr_plan(hip_lib, case, fL=A16, fR=A16, out=A16, tmp=A16):
    from dsmnet_amd import costvolume as cv
    B, C, H, W = case.shape
    off = OFF4 - A16 if case.offset else 0
    return cv.corr1d_plan_name(_ptr(fL + off), _ptr(fR + off), _ptr(out), _ptr(tmp if case.k > 1 else None),
                               B, C, H, W, case.D, case.s, case.k)


def sa_dims(case):
    B, _, Dc, Hc, Wc = case.cshape
    D, H, W = (Dc, Hc, Wc) if case.osize is None else case.osize
    return B, Dc, Hc, Wc, D, H, W


def vol_plans(case):
    """(forward plan or error code, backward plan or error code or None when there is no backward)."""
    from dsmnet_amd import costvolume as cv
    B, C, H, W = case.shape
    mask = 2 if case.mode == "right" else int(case.mode)
    res = []
    for backward in (False, True):
        if backward and case.mode == "right":
            res.append(None)
            continue
        try:
            res.append(cv.concat_volume_plan_name(_ptr(A16), _ptr(A16), _ptr(A16), B, C, H, W, case.D, mask,
                                                  case.channels_last, backward))
        except _lib.DsmnetHipError as e:
            res.append(int(str(e).rsplit("code ", 1)[1].rstrip(")")))
    return res


@pytest.mark.parametrize("case", CORR_CASES, ids=lambda c: "%s-D%d-s%d-k%d" % ("x".join(map(str, c.shape)), c.D, c.s, c.k))
def test_corr1d_case_lands_on_its_branch(hip_lib, case):
    assert corr_plan(hip_lib, case) == case.plan


@pytest.mark.parametrize("case", SA_CASES, ids=lambda c: "%s-to-%s" % ("x".join(map(str, c.cshape[2:])), "x".join(map(str, c.osize or ("same",)))))
def test_soft_argmin_case_lands_on_its_branch(hip_lib, case):
    from dsmnet_amd import costvolume as cv
    dims = sa_dims(case)
    p = _ptr(A16)
    assert cv.soft_argmin_fwd_plan_name(p, p, p, *dims, negate=case.negate, align_corners=case.align) == case.fwd
    assert cv.soft_argmin_bwd_plan_name(p, p, p, p, p, *dims, negate=case.negate, align_corners=case.align) == case.bwd
    assert cv.soft_argmin_kernel_label(case.fwd) == ("soft_argmin_up4_kernel" if case.fwd == "up4<4>" else "soft_argmin_fwd_kernel")


@pytest.mark.parametrize("case", VOL_CASES, ids=lambda c: "%s-D%d-%s-%s" % ("x".join(map(str, c.shape)), c.D, "ndhwc" if c.channels_last else "ncdhw", c.mode))
def test_volume_case_lands_on_its_branch(hip_lib, case):
    fwd, bwd = vol_plans(case)
    assert fwd == (case.fwd if case.fwd is not None else case.error)
    if case.mode != "right":
        # (a refused forward never reaches its backward; the (1,160,2,8) gradient alone would be fine)
        assert bwd == (case.bwd if case.bwd is not None else case.error)


def test_the_table_reaches_every_branch(hip_lib):
    """Dropping a case, or a new branch in a ``pick_*`` function, fails here."""
    kernels, suffixes = set(), set()
    for c in CORR_CASES:
        name = corr_plan(hip_lib, c)
        k, plus, suffix = name.partition("+")
        kernels.add(k)
        suffixes.add(plus + suffix)
    assert kernels == CORR_KERNELS
    assert suffixes == CORR_SUFFIXES
    assert {c.fwd for c in SA_CASES} == SA_FWD_NAMES
    assert {c.bwd for c in SA_CASES} == SA_BWD_NAMES
    assert not (SA_FWD_UNREACHABLE & SA_FWD_NAMES)
    assert {c.fwd for c in VOL_CASES if c.fwd} == VOL_FWD_NAMES
    assert {c.bwd for c in VOL_CASES if c.bwd} == VOL_BWD_NAMES
    assert {c.error for c in VOL_CASES} == {0, -2}


def test_plan_names_cover_the_whole_argument_space(hip_lib):
    """Every name a plan query can write is in the sets above: a sweep over both sides of every threshold
    in the ``pick_*`` functions (D, C, W, stride, box size, alignment, scales) finds no other."""
    from dsmnet_amd import costvolume as cv
    p, q = _ptr(A16), _ptr(OFF4)
    seen_k, seen_s = set(), set()
    for D in (1, 11, 48, 49, 96, 97, 128, 129, 300):
        for C in (8, 16, 160, 400):
            for W in (30, 64):
                for s in (1, 2, 3):
                    for k in (1, 3, 5):
                        for fl, out in ((p, p), (q, p), (p, q)):
                            name = cv.corr1d_plan_name(fl, p, out, p if k > 1 else None, 1, C, 2, W, D, s, k)
                            kern, plus, suffix = name.partition("+")
                            seen_k.add(kern)
                            seen_s.add(plus + suffix)
    assert seen_k == CORR_KERNELS and seen_s == CORR_SUFFIXES
    fwd, bwd = set(), set()
    for Dc in (1, 2, 3, 4, 5, 8, 24, 48):
        for D in sorted({Dc, 2 * Dc, 4 * Dc, 4 * Dc - 1, 1, 3, 4, 7, 8, 15, 16, 95, 96}):
            for (Hc, Wc, H, W) in ((4, 6, 4, 6), (4, 6, 16, 24), (40, 200, 5, 25), (4, 6, 9, 13)):
                for align in (False, True):
                    for B in (1, 40000):
                        fwd.add(cv.soft_argmin_fwd_plan_name(p, p, p, B, Dc, Hc, Wc, D, H, W, False, align))
                        bwd.add(cv.soft_argmin_bwd_plan_name(p, p, p, p, p, B, Dc, Hc, Wc, D, H, W, False, align))
    assert fwd == SA_FWD_NAMES and bwd == SA_BWD_NAMES
    vf, vb = set(), set()
    for C in (4, 64):
        for D in (3, 192):
            for W in (37, 40):
                for cl in (False, True):
                    for vol in (p, q):
                        for backward, names in ((False, vf), (True, vb)):
                            try:
                                names.add(cv.concat_volume_plan_name(p, p, vol, 1, C, 2, W, D, 1, cl, backward))
                            except _lib.DsmnetHipError:
                                assert cl and vol is q          # NDHWC needs an aligned volume
    assert vf == VOL_FWD_NAMES and vb == VOL_BWD_NAMES


def test_plans_return_the_launch_error_codes(hip_lib):
    """A plan query refuses what the launch refuses, with the same code (tests/test_abi.py has the launch side)."""
    import ctypes
    null, one = None, ctypes.c_void_p(A16)
    buf = ctypes.create_string_buffer(96)
    assert hip_lib.dsm_corr1d_plan(null, null, null, null, 1, 1, 1, 1, 1, 1, 1, 0, buf, 96) == -1
    assert hip_lib.dsm_corr1d_plan(one, one, one, null, 1, 8, 4, 4, 4, 1, 2, 0, buf, 96) == -1   # even k
    assert hip_lib.dsm_corr1d_plan(one, one, one, null, 1, 8, 4, 4, 4, 1, 3, 0, buf, 96) == -1   # no tmp
    assert hip_lib.dsm_corr1d_plan(one, one, one, null, 1, 8, 4, 4, 4, 1, 1, 7, buf, 96) == -2   # dtype
    assert hip_lib.dsm_corr1d_plan(one, one, one, null, 1, 8, 4, 4, 4, 1, 1, 0, null, 96) == -1  # no buffer
    assert hip_lib.dsm_concat_volume_fwd_plan(one, one, one, 1, 8, 4, 4, 0, 1, 1, 0, buf, 96) == -1  # D = 0
    assert hip_lib.dsm_concat_volume_fwd_plan(one, one, one, 1, 8, 4, 4, 4, 1, 5, 0, buf, 96) == -1  # layout
    assert hip_lib.dsm_concat_volume_fwd_plan(one, one, one, 1, 6, 4, 4, 4, 1, 1, 0, buf, 96) == -2  # C % 4
    assert hip_lib.dsm_concat_volume_fwd_plan(one, one, one, 1, 8, 4, 4, 4, 2, 0, 0, buf, 96) == -2  # right-referenced NCDHW
    assert hip_lib.dsm_concat_volume_fwd_plan(one, one, ctypes.c_void_p(OFF4), 1, 8, 4, 4, 4, 1, 1, 0, buf, 96) == -4
    assert hip_lib.dsm_concat_volume_bwd_plan(ctypes.c_void_p(OFF4), one, one, 1, 8, 4, 4, 4, 1, 1, 0, buf, 96) == -4
    assert hip_lib.dsm_concat_volume_bwd_plan(one, one, one, 1, 252, 4, 4, 4, 1, 1, 0, buf, 96) == -2  # 2 C rows of LDS > 64 KB
    assert hip_lib.dsm_soft_argmin_fwd_plan(null, one, null, 1, 4, 4, 4, 4, 4, 4, 0, 0, 0, buf, 96) == -1
    assert hip_lib.dsm_soft_argmin_bwd_plan(one, one, null, one, one, 1, 4, 4, 4, 4, 4, 4, 0, 0, 0, buf, 96) == -1  # no stats
    assert hip_lib.dsm_soft_argmin_fwd_plan(one, one, null, 1, 4, 4, 4, 16, 8, 8, 0, 0, 0, buf, 96) == 0
    assert buf.value == b"up4<4>"


def test_bn_cases_reach_the_strided_loops():
    """The arithmetic behind the BN rows: which of them make the capped grids stride (csrc/bn3d.hip:
    512 blocks of 256 / (C / 4) voxel lanes in the reductions; 4096 blocks of 256 quads in the passes that
    report an absolute maximum)."""
    def vox(c):
        n = 1
        for v in c.yshape:
            n *= v
        return n
    strided = [c for c in BN_CASES if vox(c) > 512 * (256 // (c.C // 4))]
    assert [c.C for c in strided] == [32, 64]
    assert {c.C for c in BN_CASES} >= {4, 12, 128, 256}
    assert 256 % (12 // 4) != 0                                      # idle threads at C = 12
    assert any(c.rshape and c.yshape[0] > 1 and tuple(c.rshape) != tuple(c.yshape[1:]) for c in BN_CASES)
    quads = vox(BN_CAP_CASE) * (BN_CAP_CASE.C // 4)
    assert quads > 4096 * 256 and vox(BN_CAP_CASE) == 138240
