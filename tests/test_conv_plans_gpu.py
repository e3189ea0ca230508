"""GPU parity of every kernel variant ``dsm_conv3d_fwd`` can launch: one launch per row of the plan table of
tests/test_conv_plans.py (``CASES``), through ``conv3d_block`` / ``conv2d_block``, against torch's float64
convolution on the CPU with the folded scale / shift, the (cropped) residual and the ReLU.

* the name: the launch is timed by a ``LaunchTimer``, which asks ``dsm_conv3d_plan`` with the very argument struct
  (real pointers, the wrapper's own flags and maxima) that is launched -- it must be the row's name, exactly;
* the band: the fp32-input kernels (names without a split mode) hold 2e-4 absolute on unit data with He-scaled
  weights (tests/test_conv3d_gpu.py, test_conv2d_gpu.py); the split, z-sliding and transposed-split kernels hold
  the (max, rms) pairs of their mode (tests/test_zs_gpu.py ``LIMITS``, from tests/test_f16_gpu.py), relative to the
  largest output / the output's rms, grown by sqrt(Cin / 64) on 3-D rows as there and not at all on 2-D rows;
* ``y_amax``: in the fp16 modes every launch to 32 or more channels reports max |y| exactly, whichever kernel the
  row lands on (the fp32-input ones included) -- the next layer scales its fp16 operands by it;
* a row with ``grid`` is launched a second time with that persistent grid forced (fewer workgroups than tiles:
  tests/test_conv_plans.py checks it): the same bits;
* the last test of the module holds the set of launched names against the table's."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ops as OO
from tests.helpers import maxerr, seeded
from tests.test_conv3d_gpu import TOL
from tests.test_conv_plans import CASES, SPLIT_MODES, row_id
from tests.test_f16_gpu import errors, precision
from tests.test_zs_gpu import LIMITS

pytestmark = pytest.mark.gpu

LAUNCHED = set()
F16_MODES = ("f16x2", "f16")


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


def is_split(row):
    return any("_%s_" % m in row.name for m in SPLIT_MODES)


def tensors(row, seed):
    """Unit data and He-scaled weights (fan-out, as the fp32 parity tests scale them), scale / shift of a folded
    BatchNorm.  A virtual-volume row draws the two feature maps and builds the volume for the reference."""
    three_d = len(row.size) == 3
    taps = 27 if three_d else row.k * row.k
    kshape = (3, 3, 3) if three_d else (row.k, row.k)
    wshape = ((row.cin, row.cout) if row.tr else (row.cout, row.cin)) + kshape
    w = seeded(seed + 1, *wshape, scale=(2.0 / (taps * row.cout)) ** 0.5)
    sc, sh = seeded(seed + 2, row.cout).abs() + 0.5, seeded(seed + 3, row.cout)
    if row.vol:
        D, H, W = row.size
        fL, fR = seeded(seed, row.B, row.cin // 2, H, W), seeded(seed + 4, row.B, row.cin // 2, H, W)
        return OO.concat_volume(fL, fR, D, mask_left=False), w, sc, sh, (fL, fR)
    return seeded(seed, row.B, row.cin, *row.size), w, sc, sh, None


def reference(row, x, w, sc, sh, res, relu):
    xd, wd = x.double(), w.double()
    if len(row.size) == 2:
        y = F.conv2d(xd, wd, None, row.stride, row.dil * (row.k - 1) // 2, row.dil)
    elif row.tr:
        y = F.conv_transpose3d(xd, wd, stride=2, padding=1, output_padding=1)
    else:
        y = F.conv3d(xd, wd, stride=row.stride, padding=1)
    view = (1, -1) + (1,) * (y.dim() - 2)
    y = y * sc.double().view(view) + sh.double().view(view)
    if relu == 2:
        y = y.relu()
    if res is not None:
        crop = (slice(None), slice(None)) + tuple(slice(0, n) for n in res.shape[2:])
        y = y[crop] + res.double()
    return y.relu() if relu == 1 else y


def out_size(row):
    return tuple(2 * v if row.tr else (v - 1) // row.stride + 1 for v in row.size)


def launch(cv, row, x, w, sc, sh, res, relu, feats=None, grid=0, record=True):
    """One launch in the row's mode and flags; the name its plan gives the launched arguments must be the row's.
    ``record``: count the name for the last test of this module (other modules that borrow the helper do not)."""
    from dsmnet_amd import _lib
    three_d = len(row.size) == 3
    if three_d:
        packed = cv.pack_conv3d_weight(w.cuda(), bool(row.tr))
        if feats is not None:
            both = torch.cat(feats, 0).cuda().contiguous(memory_format=torch.channels_last)
            xin = cv.VirtualVolume(both, row.size[0], False)
        else:
            xin = x.cuda()
    else:
        packed = cv.pack_conv2d_weight(w.cuda())
        xin = x.cuda().contiguous(memory_format=torch.channels_last)
    r = None if res is None else res.cuda()
    timer = cv.LaunchTimer()
    old = cv.set_option("conv_flags", row.flags | (grid << _lib.DSM_CONV_BLOCKS_SHIFT))
    cv.set_timer(timer)
    try:
        with precision(cv, row.mode):
            if three_d:
                y = cv.conv3d_block(xin, packed, row.cout, sc.cuda(), sh.cuda(), r, row.stride, bool(row.tr), relu)
            else:
                y = cv.conv2d_block(xin, packed, row.cout, sc.cuda(), sh.cuda(), r, row.stride, relu, row.k, row.dil)
    finally:
        cv.set_timer(None)
        cv.set_option("conv_flags", old)
    torch.cuda.synchronize()
    names = [rec[0] for rec in timer.records if rec[0] != "absmax_kernel"]
    assert names == [row.name], names
    if record:
        LAUNCHED.add(row.name)
    return y


def check_band(row, y, want):
    assert tuple(y.shape) == tuple(want.shape)
    if not is_split(row):
        err = maxerr(y, want)
        print("ERR %s %s abs %.3e (<= %.1e)" % (row.name, row.mode, err, TOL))
        assert err <= TOL, err
    else:
        emax, erms = errors(y, want)
        grow = max(1.0, row.cin / 64.0) ** 0.5 if len(row.size) == 3 else 1.0
        lmax, lrms = LIMITS[row.mode][0] * grow, LIMITS[row.mode][1] * grow
        print("ERR %s %s max %.3e (<= %.2e) rms %.3e (<= %.2e)" % (row.name, row.mode, emax, lmax, erms, lrms))
        assert emax <= lmax and erms <= lrms, (emax, erms)


def check_amax(row, y):
    if row.mode in F16_MODES and row.cout >= 32:
        assert y._dsm_amax.item() == y.abs().max().item()


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: row_id(CASES[i]))
def test_every_row_against_float64(cv, i):
    """Ragged last tiles come with the table's sizes; the transposed rows add a residual one shorter than the
    output in z, y and x (myadd_3d: the output is the common corner), every third other row a full-size one;
    ReLU after the add (1) or before it (2)."""
    row = CASES[i]
    x, w, sc, sh, feats = tensors(row, 1000 + 10 * i)
    osz = out_size(row)
    res = None
    if row.tr:
        res = seeded(1005 + 10 * i, row.B, row.cout, *(max(1, v - 1) for v in osz))
    elif i % 3 == 0:
        res = seeded(1005 + 10 * i, row.B, row.cout, *osz)
    relu = 2 if res is not None and i % 2 else 1
    want = reference(row, x, w, sc, sh, res, relu)
    y = launch(cv, row, x, w, sc, sh, res, relu, feats)
    check_band(row, y, want)
    check_amax(row, y)
    if row.grid:
        z = launch(cv, row, x, w, sc, sh, res, relu, feats, grid=row.grid)
        assert torch.equal(z, y)
        check_amax(row, z)


# the fp16-mode rows to 32 or more channels that are a few tiles large: every kernel family is among them, the
# fp32-input kernels that such a row lands on (1x1, stride 2, 128 outputs) included
AMAX_ROWS = [i for i, r in enumerate(CASES) if r.mode in F16_MODES and r.cout >= 32 and not r.vol and
             r.B * r.cin * torch.Size(r.size).numel() <= 1 << 20]


@pytest.mark.parametrize("i", AMAX_ROWS, ids=lambda i: row_id(CASES[i]))
def test_y_amax_of_a_negative_maximum(cv, i):
    """No ReLU, one channel shifted far below zero: the largest magnitude is a negative value."""
    row = CASES[i]
    x, w, sc, sh, _ = tensors(row, 5000 + 10 * i)
    sh[row.cout // 2] = -1000.0
    y = launch(cv, row, x, w, sc, sh, None, 0)
    amax = y._dsm_amax.item()
    assert amax == y.abs().max().item() and y.min().item() == -amax and amax > 900.0


@pytest.mark.parametrize("i", AMAX_ROWS, ids=lambda i: row_id(CASES[i]))
def test_y_amax_of_a_maximum_in_the_ragged_last_tile(cv, i):
    """The residual puts the largest value on the last voxel of the last image's last channel: the corner of the
    partial tile in every direction."""
    row = CASES[i]
    x, w, sc, sh, _ = tensors(row, 7000 + 10 * i)
    res = seeded(7005 + 10 * i, row.B, row.cout, *out_size(row))
    res.view(-1)[-1] = 1000.0
    y = launch(cv, row, x, w, sc, sh, res, 1)
    amax = y._dsm_amax.item()
    assert amax == y.abs().max().item() and amax == y.cpu().reshape(-1)[-1].item() and amax > 900.0


def test_every_name_of_the_table_was_launched():
    """Runs last: the rows above launched every variant the table names (test_conv_plans.py proves that the table
    names every variant the planner can produce, the wide kernels of test_wide2d_gpu.py aside)."""
    assert LAUNCHED == {r.name for r in CASES}, sorted({r.name for r in CASES} - LAUNCHED)
