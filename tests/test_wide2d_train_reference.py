"""CPU: training through the wide 3x3 layers (``costvolume.wide_conv2d_relu``) -- what the GPU tests of
tests/test_wide2d_train_gpu.py rest on, and the host side of the dispatch.

1. Quarter rule (tests/test_bwd_ranges_reference.py): torch's fp32 CPU autograd of relu(conv2d(x, w, b))
   against float64 autograd stays below a quarter of the tightest gradient bound used on the GPU (1e-4), with
   the mask of the fp32 forward.
2. The restatement the GPU tests use for the transposed launch: conv_transpose2d(g, w, stride 2, padding 1,
   output_padding 1) cropped == conv2d(zero-interleaved g, flipped transposed w, padding 1), in float64.
3. Plan, workspace, option and dispatch of the new path (host only: fake 16-byte-aligned addresses)."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dsmnet_amd import _lib
from tests import wide2d_train_cases as T
from tests.test_wide2d_plans import PREC, plan

A16 = 16


# ------------------------------------------------------------------------------------ 1. quarter rule --
@pytest.mark.parametrize("key", T.IDS)
def test_fp32_autograd_is_within_a_quarter_of_the_gradient_bound(key):
    x, w, b, pre, cot = T.case_data(key)
    stride = T.CASES[key][2]
    clipped = (pre <= 0).double().mean().item()
    assert 0.3 <= clipped <= 0.7, clipped
    xf, wf, bf = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = F.relu(F.conv2d(xf, wf, bf, stride=stride, padding=1))
    dx, dw, db = torch.autograd.grad(y, [xf, wf, bf], cot)
    mask = y.detach() > 0
    flipped = (mask != (pre > 0)).sum().item()
    gx, gw, gb = T.grads64(key, mask)
    ex, ew, eb = T.rel(dx, gx), T.rel(dw, gw), T.rel(db, gb)
    print("%s: clipped %.3f, fp32 mask differs from float64 in %d entries; fp32 CPU autograd vs float64 "
          "dX %.2e dW %.2e db %.2e" % (key, clipped, flipped, ex, ew, eb))
    lim = min(T.TOL.values()) / 4
    assert ex <= lim and ew <= lim and eb <= lim, (ex, ew, eb)


# ----------------------------------------------------------------------------- 2. restatement identity --
@pytest.mark.parametrize("key", T.STRIDE2)
def test_transposed_convolution_equals_the_convolution_of_the_zero_interleaved_map(key):
    (B, cin, H, W), cout, _ = T.CASES[key]
    x, w, b, pre, cot = T.case_data(key)
    g = (cot.double() * (pre > 0).double())
    assert 2 * g.shape[2] - 1 <= H <= 2 * g.shape[2] and 2 * g.shape[3] - 1 <= W <= 2 * g.shape[3]
    a = F.conv_transpose2d(g, w.double(), stride=2, padding=1, output_padding=1)[..., :H, :W]
    z = F.conv2d(T.zero_interleave(g, H, W), w.double().flip(2, 3).transpose(0, 1), padding=1)
    assert a.shape == z.shape == (B, cin, H, W)
    assert (a - z).abs().max().item() <= 1e-12 * a.abs().max().item()
    assert (a - T.grads64(key, pre > 0)[0]).abs().max().item() <= 1e-12 * a.abs().max().item()


def test_the_shapes_put_block_origins_on_odd_rows_and_columns():
    """E and F exist for the parity of the ABSOLUTE coordinate: the dx launch of E has a second M-block that
    begins at an odd row, that of F column blocks that begin at odd columns."""
    R, CW, nby, nbx = T.geometry_s1(22, 36)
    assert nby >= 2 and any((by * R) % 2 for by in range(nby)), (R, CW, nby, nbx)
    R, CW, nby, nbx = T.geometry_s1(21, 75)
    assert nbx >= 2 and any((bx * CW) % 2 for bx in range(nbx)), (R, CW, nby, nbx)


# ---------------------------------------------------------------------------------- 3. plan and option --
def dx_args(key, mode, dil=1, stride=2, cout=None, flags=0):
    """The backward-data request of CASES[key]: input = the layer's output gradient, output = the layer's x."""
    (B, cin, H, W), co, _ = T.CASES[key]
    Hg, Wg = T.out_size(key)
    a = _lib.Conv3dArgs()
    a.x = a.w_packed = a.y = a.x_amax = A16
    a.B, a.Cin, a.Cout = B, co, cin if cout is None else cout
    a.Di, a.Hi, a.Wi, a.Do, a.Ho, a.Wo = 1, Hg, Wg, 1, H, W
    a.stride, a.transposed, a.relu = stride, 1, 0
    a.kd, a.k, a.dil = 1, 3, dil
    a.precision, fl = PREC[mode]
    a.flags = fl | flags
    return a


def test_the_option_exists_is_off_and_rejects_a_bad_environment_value(monkeypatch):
    from dsmnet_amd import costvolume as cv
    assert cv.get_option("wide_conv2d_train") is False
    assert cv.set_option("wide_conv2d_train", True) is False
    assert cv.set_option("wide_conv2d_train", False) is True
    monkeypatch.setenv("DSM_WIDE_CONV2D_TRAIN", "2")
    with pytest.raises(ValueError):
        cv._env_flag("DSM_WIDE_CONV2D_TRAIN", False)
    monkeypatch.setenv("DSM_WIDE_CONV2D_TRAIN", "1")
    assert cv._env_flag("DSM_WIDE_CONV2D_TRAIN", False) is True


@pytest.mark.parametrize("key", T.STRIDE2)
def test_plan_of_the_transposed_request(hip_lib, key):
    from dsmnet_amd import costvolume as cv
    for mode in ("f16x2", "f16"):
        a = dx_args(key, mode)
        rc, name = plan(hip_lib, a)
        assert rc == 0 and name.startswith("deconv2d_wide_%s_mfma_kernel<" % mode), (rc, name)
        assert cv._split_kernel_layer(a)                                     # the launch needs x_amax
        ks = int(name.split("KS=")[1].split(",")[0])
        ws = hip_lib.dsm_conv3d_workspace_bytes(ctypes.byref(a))
        assert ws == (4 * ks * a.B * a.Ho * a.Wo * a.Cout if ks > 1 else 0), (name, ws)
        a.x_amax = None
        assert plan(hip_lib, a) == (-1, "")
    for mode in ("bf16x3", "fp32"):
        assert plan(hip_lib, dx_args(key, mode)) == (-2, "")


def test_plan_refuses_every_other_transposed_2d_request(hip_lib):
    from dsmnet_amd import costvolume as cv
    for a in (dx_args("B", "f16x2", cout=384), dx_args("B", "f16x2", dil=2), dx_args("B", "f16x2", stride=1),
              dx_args("B", "f16x2", cout=64), dx_args("B", "f16x2", cout=128)):
        assert plan(hip_lib, a) == (-2, ""), (a.Cout, a.dil, a.stride)
        assert hip_lib.dsm_conv3d_workspace_bytes(ctypes.byref(a)) == 0
        assert not cv._split_kernel_layer(a) or a.Cout in (64, 128)
    a = dx_args("B", "f16x2")
    a.k = 1
    assert plan(hip_lib, a) == (-2, "")
    a = dx_args("B", "f16x2")
    a.Ho -= 1                                                                # 2 Hi - 2: no stride-2 source of Hi rows
    assert plan(hip_lib, a) == (-2, "")
    a = dx_args("B", "f16x2")
    a.Ho = 2 * a.Hi + 1                                                      # more than the natural size: refused alike
    assert plan(hip_lib, a) == (-2, "")
    a = dx_args("B", "f16x2")
    a.residual, a.Dr, a.Hr, a.Wr = A16, 1, a.Ho, a.Wo
    assert plan(hip_lib, a) == (-2, "")


def test_a_forced_split_shows_in_the_plan_and_the_workspace(hip_lib):
    a = dx_args("D", "f16x2", flags=5 << _lib.DSM_CONV_KSPLIT_SHIFT)        # Cin = 1024: 64 chunks, at least 8 ranges
    rc, name = plan(hip_lib, a)
    assert rc == 0 and "KS=8," in name, name
    a = dx_args("B", "f16x2", flags=7 << _lib.DSM_CONV_KSPLIT_SHIFT)        # Cin = 512: 32 chunks
    rc, name = plan(hip_lib, a)
    assert rc == 0 and "KS=7," in name, name
    assert hip_lib.dsm_conv3d_workspace_bytes(ctypes.byref(a)) == 4 * 7 * a.B * a.Ho * a.Wo * a.Cout


def test_the_backward_entry_point_is_bound(hip_lib):
    assert hip_lib.dsm_bias_relu_bwd.argtypes[6] is ctypes.c_long
    assert hip_lib.dsm_abi_version() == 7
    # argument checks run before any launch: no device is touched
    assert hip_lib.dsm_bias_relu_bwd(None, A16, A16, None, None, None, 8, 256, None) == -1
    assert hip_lib.dsm_bias_relu_bwd(A16, 2 * A16, 3 * A16, 4 * A16, None, None, 8, 256, None) == -1   # db without ws
    assert hip_lib.dsm_bias_relu_bwd(A16, 2 * A16, A16, None, None, None, 8, 256, None) == -1          # g is gy
    assert hip_lib.dsm_bias_relu_bwd(A16, 2 * A16, 3 * A16, None, None, None, 8, 254, None) == -2      # C % 4
    assert hip_lib.dsm_bias_relu_bwd(A16, 2 * A16 + 4, 3 * A16, None, None, None, 8, 256, None) == -4  # alignment


class FakeCudaMap(object):
    """What the dispatch looks at: an fp32 CUDA tensor's type, shape and requires_grad, without a GPU."""
    is_cuda, dtype, requires_grad = True, torch.float32, False

    def __init__(self, *shape):
        self.shape = torch.Size(shape)


TAKEN = [(256, 256, 1, 3), (256, 512, 2, 3), (512, 512, 1, 3), (512, 512, 2, 3), (512, 1024, 2, 3), (1024, 1024, 1, 3)]
REFUSED = [(105, 256, 2, 5), (145, 256, 2, 3), (1025, 512, 1, 3), (128, 256, 1, 3), (256, 128, 1, 3), (256, 384, 1, 3)]


@pytest.fixture
def routes(monkeypatch):
    """Conv2dReLU.forward with both ends replaced: which path does a layer take?"""
    from dsmnet_amd import costvolume as cv
    monkeypatch.setattr(cv, "wide_conv2d_relu", lambda x, w, b, s: ("wide_train", s))
    monkeypatch.setattr(nn.Sequential, "forward", lambda self, x: ("stock", None))
    old = (cv.set_option("wide_conv2d_train", True), cv.set_option("conv_precision", "f16x2"),
           cv.set_option("wide_conv2d", False))
    yield cv
    cv.set_option("wide_conv2d_train", old[0])
    cv.set_option("conv_precision", old[1])
    cv.set_option("wide_conv2d", old[2])


def _layer(cin, cout, s, k, bias=True, act=None):
    from dsmnet_amd.models.util_conv import Conv2dReLU
    return Conv2dReLU(nn.Conv2d(cin, cout, k, s, padding=(k - 1) // 2, bias=bias), act or nn.ReLU(inplace=True))


def test_conv2drelu_takes_the_new_path_exactly_where_every_gradient_has_a_kernel(routes):
    cv = routes
    for cin, cout, s, k in TAKEN:
        assert _layer(cin, cout, s, k)(FakeCudaMap(1, cin, 12, 40)) == ("wide_train", s), (cin, cout, s, k)
    for cin, cout, s, k in REFUSED:
        assert _layer(cin, cout, s, k)(FakeCudaMap(1, cin, 12, 40))[0] == "stock", (cin, cout, s, k)
    x = FakeCudaMap(1, 256, 12, 40)
    assert _layer(256, 256, 1, 3, bias=False)(x)[0] == "stock"
    assert _layer(256, 256, 1, 3, act=nn.LeakyReLU(0.1))(x)[0] == "stock"
    assert _layer(256, 256, 1, 3)(FakeCudaMap(1, 256, 12, 2040))[0] == "stock"          # the size limits of _wide_ok
    # 256 -> 1024 at 700 x 1000: the forward fits 32-bit offsets, the output gradient backward-data reads does not
    assert _layer(256, 1024, 1, 3)(FakeCudaMap(1, 256, 700, 1000))[0] == "stock"
    assert _layer(256, 1024, 1, 3)(FakeCudaMap(1, 256, 500, 1000))[0] == "wide_train"
    with torch.no_grad():
        assert _layer(256, 256, 1, 3)(x)[0] == "stock"
    frozen = _layer(256, 256, 1, 3)
    for p in frozen.parameters():
        p.requires_grad_(False)
    assert frozen(x)[0] == "stock"                                                      # nothing requires grad
    for mode in ("bf16x3", "fp32"):
        cv.set_option("conv_precision", mode)
        assert _layer(256, 256, 1, 3)(x)[0] == "stock"
    cv.set_option("conv_precision", "f16")
    assert _layer(256, 256, 1, 3)(x)[0] == "wide_train"
    cv.set_option("wide_conv2d_train", False)
    for wide in (False, True):                       # with the option off nothing changes, whatever wide_conv2d says
        cv.set_option("wide_conv2d", wide)
        assert _layer(256, 256, 1, 3)(x)[0] == "stock"


def test_pack_cache_makes_one_pack_per_weight_version_and_drops_it_with_the_weight(monkeypatch):
    """The contract of tests/test_folded_caches.py for the forward and gradient packs of a wide layer."""
    import gc
    from dsmnet_amd import blocks3d, costvolume as cv
    calls = []
    monkeypatch.setattr(cv, "pack_conv2d_weight", lambda w: calls.append(tuple(w.shape)) or w.clone())
    w = nn.Parameter(torch.randn(8, 4, 3, 3))
    ent = cv._wide_pack_entry(w)
    first = cv._wide_pack(ent, w, "forward")
    assert cv._wide_pack(cv._wide_pack_entry(w), w, "forward") is first and len(calls) == 1      # the second forward
    grad = cv._wide_pack(cv._wide_pack_entry(w), w, "gradient")
    assert calls[-1] == (4, 8, 3, 3) and torch.equal(grad, w.detach().flip(2, 3).transpose(0, 1))
    assert cv._wide_pack(ent, w, "gradient") is grad and len(calls) == 2
    with torch.no_grad():
        w.mul_(2.0)                                  # an optimizer step bumps the version
    assert cv._wide_pack(cv._wide_pack_entry(w), w, "forward") is not first and len(calls) == 3
    blocks3d.invalidate_folded_caches()              # a graph replay: the epoch
    cv._wide_pack(cv._wide_pack_entry(w), w, "forward")
    assert len(calls) == 4
    key = id(w)
    assert key in cv._WIDE_PACKS
    del w, ent
    gc.collect()
    assert key not in cv._WIDE_PACKS
