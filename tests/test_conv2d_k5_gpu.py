"""GPU: the 5x5 stride-2 2-D layers (Cout 128 / 256; dsmnet_amd/csrc/conv_wide2d.hpp with K = 5) against float64
``F.conv2d(stride=2, padding=2)`` + bias (+ ReLU) on the CPU, their determinism and ``y_amax``.

Bands (tests/test_f16_gpu.py, as tests/test_wide2d_gpu.py uses them): f16x2 -- max <= 1.5e-6 of the largest
output, rms <= 6e-7 of the output rms; f16 -- max <= 3e-3, rms <= 6e-4.  K = 25 Cin is at most 3,200 here
(9,216 in the wide suite)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import seeded
from tests.test_wide2d_gpu import F16_MAX, F16_RMS, F16X2_MAX, F16X2_RMS, cv, errors, options  # noqa: F401 (cv: fixture)

pytestmark = pytest.mark.gpu

# (B, Cin, H, W), Cout, input scale
CASES = [
    ((1, 64, 10, 14), 128, 1.0),       # even H and W: the 5x5 window leaves the map on one side only
    ((2, 16, 7, 11), 128, 1e-6),       # one chunk, batch 2, odd extents; tiny inputs
    ((1, 128, 1, 1), 256, 1.0),        # only the centre tap sees data
    ((1, 64, 9, 67), 128, 1e4),        # a 34-wide output row crosses a 32-pixel M-tile; large inputs
    ((1, 48, 30, 330), 256, 1.0),      # a 15 x 165 output: several column blocks and row blocks, Cin % 32 != 0
    ((1, 128, 3, 5), 256, 1.0),        # the map is smaller than the window in both directions
]
# share of the reference that ReLU clips, computed on the CPU when the cases were chosen
CLIPPED = [0.480, 0.498, 0.492, 0.490, 0.501, 0.455]


@functools.lru_cache(maxsize=None)
def case_data(i):
    """(x, w, bias, float64 conv + bias before the activation) of CASES[i]: computed once, never modified.
    The bias has the spread of the convolution's output, so that ReLU clips about half the outputs with a
    different share in every channel."""
    shape, cout, xs = CASES[i]
    cin = shape[1]
    x = seeded(800 + i, *shape, scale=xs)
    w = seeded(900 + i, cout, cin, 5, 5, scale=(2.0 / (25 * cin)) ** 0.5)
    pre = F.conv2d(x.double(), w.double(), stride=2, padding=2)
    b = (seeded(1000 + i, cout).double() * pre.std()).float()
    return x, w, b, pre + b.double().view(1, -1, 1, 1)


def run_case(cv, i, relu, mode="f16x2", flags=0):
    x, w, b, _ = case_data(i)
    _, cout, _ = CASES[i]
    with options(cv, conv_precision=mode, conv_flags=flags):
        xg = x.cuda().contiguous(memory_format=torch.channels_last)
        return cv.conv2d_block(xg, cv.pack_conv2d_weight(w.cuda()), cout, torch.ones(cout, device="cuda"), b.cuda(),
                               stride=2, relu=relu, k=5)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("mode", ["f16x2", "f16"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_parity_against_float64(cv, i, mode, relu):
    ref = case_data(i)[3]
    ref = ref.relu() if relu else ref
    if relu:
        clipped = (ref == 0).double().mean().item()
        assert 0.3 <= clipped <= 0.7 and abs(clipped - CLIPPED[i]) < 5e-4, clipped
    (B, _, H, W), cout, _ = CASES[i]
    y = run_case(cv, i, relu, mode)
    assert tuple(y.shape) == (B, cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1) == tuple(ref.shape)
    assert y.is_contiguous(memory_format=torch.channels_last)
    emax, erms = errors(y, ref)
    print("case %d %s relu=%d: max %.2e rms %.2e" % (i, mode, relu, emax, erms))
    lim = (F16X2_MAX, F16X2_RMS) if mode == "f16x2" else (F16_MAX, F16_RMS)
    assert emax <= lim[0] and erms <= lim[1], (emax, erms)


@pytest.mark.parametrize("i", [0, 3, 4])
def test_the_same_call_twice_gives_identical_bits(cv, i):
    a, b = run_case(cv, i, 1), run_case(cv, i, 1)
    assert torch.equal(a, b)


# case 0 (4 chunks: 1 .. 4 ranges, 63 is clamped to 4); case 4 (3 chunks; a grid of 3 workgroups walks the units)
@pytest.mark.parametrize("i,ks,grid", [(0, 1, 0), (0, 2, 0), (0, 4, 0), (0, 63, 0), (4, 3, 0), (4, 0, 3)])
def test_forced_splits_and_grids_stay_inside_the_band(cv, i, ks, grid):
    from dsmnet_amd import _lib
    flags = (ks << _lib.DSM_CONV_KSPLIT_SHIFT) | (grid << _lib.DSM_CONV_BLOCKS_SHIFT)
    ref = case_data(i)[3].relu()
    y = run_case(cv, i, 1, flags=flags)
    emax, erms = errors(y, ref)
    print("case %d ks=%d grid=%d: max %.2e rms %.2e" % (i, ks, grid, emax, erms))
    assert emax <= F16X2_MAX and erms <= F16X2_RMS, (emax, erms)
    assert torch.equal(y, run_case(cv, i, 1, flags=flags))


def raw_launch(cv, i, y_amax, flags=0):
    """``dsm_conv3d_fwd`` with a caller-owned ``y_amax`` slot."""
    from dsmnet_amd import _lib
    x, w, b, _ = case_data(i)
    (B, cin, H, W), cout, _ = CASES[i]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xg = x.cuda().contiguous(memory_format=torch.channels_last)
    packed, bias = cv.pack_conv2d_weight(w.cuda()), b.cuda()
    assert packed.numel() * 4 == 16 + cin * cout * 25 * 4
    y = torch.empty((B, cout, Ho, Wo), device="cuda").contiguous(memory_format=torch.channels_last)
    xa = cv.absmax(xg)
    a = _lib.Conv3dArgs()
    a.x, a.w_packed, a.y, a.shift = xg.data_ptr(), packed.data_ptr(), y.data_ptr(), bias.data_ptr()
    a.B, a.Cin, a.Cout = B, cin, cout
    a.Di, a.Hi, a.Wi, a.Do, a.Ho, a.Wo = 1, H, W, 1, Ho, Wo
    a.stride, a.relu, a.kd, a.k, a.dil = 2, 1, 1, 5, 1
    a.flags = flags
    a.precision, a.x_amax, a.y_amax = _lib.DSM_PREC_F16X2, xa.data_ptr(), y_amax.data_ptr()
    nws = _lib.load().dsm_conv3d_workspace_bytes(ctypes.byref(a))
    ws = torch.empty(max(nws // 4, 4), device="cuda")
    a.workspace, a.workspace_bytes = ws.data_ptr(), nws
    _lib.check(_lib.load().dsm_conv3d_fwd(ctypes.byref(a), cv._stream()), "dsm_conv3d_fwd")
    torch.cuda.synchronize()
    return y


# case 0 with one K-range (the kernel's own epilogue folds the maximum) and split (the reduce pass does), case 4
@pytest.mark.parametrize("i,ks", [(0, 1), (0, 0), (4, 0)])
def test_y_amax(cv, i, ks):
    from dsmnet_amd import _lib
    flags = ks << _lib.DSM_CONV_KSPLIT_SHIFT
    slot = torch.zeros(1, device="cuda")
    y = raw_launch(cv, i, slot, flags)
    assert slot.item() == y.abs().max().item() > 0
    big = torch.full((1,), 2.0 * y.abs().max().item(), device="cuda")
    want = big.item()
    raw_launch(cv, i, big, flags)
    assert big.item() == want                    # a slot that already holds more is left alone
    y2 = run_case(cv, i, 1, flags=flags)         # and the host wrapper hands the maximum to the next layer
    assert y2._dsm_amax.item() == y2.abs().max().item()


def test_pack_refuses_other_5x5_layers(cv):
    with pytest.raises(ValueError):
        cv.pack_conv2d_weight(torch.zeros(64, 64, 5, 5, device="cuda"))
    with pytest.raises(ValueError):
        cv.pack_conv2d_weight(torch.zeros(256, 105, 5, 5, device="cuda"))
