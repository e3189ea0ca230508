"""GPU: every kernel family that takes its precision from dsmnet_amd/csrc/split_core.hpp, in each mode that
reaches it, against the PER-ELEMENT bound of tests/split_bound.py -- max(|y - float64| / bound) <= 1 over all
outputs -- on inputs with a loud and a quiet part, where ``max|err| / max|ref|`` sees nothing
(tests/test_split_bound.py shows on the CPU that this yardstick catches a lost low term and flushed subnormals).

Rows (the smallest shapes that leave partial tiles), each asserting its plan first:
  conv_split 3-D   64 -> 64 s1, 32 -> 64 s2 (all modes), 64 -> 32 transposed (bf16x3)        (2, ., 5, 9, 37)
  conv_split 2-D   128 -> 128, dilation 2                                                    (2, 128, 17, 33)
  conv_zs          32 -> 32 s1 on (2, 32, 5, 11, 53); the virtual volume of (2, 32, 11, 53) maps, D = 14
  deconv_zs        64 -> 32                                                                  (1, 64, 5, 6, 35)
  wide 3x3         48 -> 256 s1 (2, 48, 7, 11); 256 -> 512 s2 (1, 256, 7, 11) and its backward-data launch
  5x5 s2           16 -> 128                                                                 (1, 16, 9, 21)
  basicblock2d     C = 32, 64 with skip and ReLU, and the same with an identity first layer  (2, C, 13, 37)
  weight gradients 3-D 32 -> 32 s1, 32 -> 64 s2 (1, ., 5, 9, 37); 2-D 64 -> 64 (2, 64, 13, 37)
Classes (split_bound.make_input, all on the ``relu_like`` base): G Gaussian, O4 / O6 one element x 1e4 (interior)
/ x 1e6 (last ragged tile), Q half the columns 2^-18 below the rest, L sign * exp(3 |n|), C one channel x 2^12,
Z all zero but one element, Wt one weight tap x 1e3; for the weight gradients the class goes to X ("X-..") or to
the gradient G ("G-..").  f16x2 runs every class, f16 and bf16x3 run G, O6 and Q.  Every case prints its ratio
as ``CONTRACT <row> <class> <mode> <ratio>`` (DESIGN.md 3.2a keeps the measured table).

Range edges (one conv_zs and one wide row, max |x| exactly 2^-48, 2^75 and 2^-70) and PSMNet under a rescaling
that leaves the network unchanged are at the end."""
import functools
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

from tests import split_bound as SB
from tests.helpers import seeded

pytestmark = pytest.mark.gpu
CL = torch.channels_last
ALL, F16S, BF = ("f16x2", "f16", "bf16x3"), ("f16x2", "f16"), ("bf16x3",)
SOME = ("G", "O6", "Q")                                  # the classes of the f16 and bf16x3 modes


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


@contextmanager
def precision(cv, mode):
    old = cv.set_option("conv_precision", mode)
    try:
        yield
    finally:
        cv.set_option("conv_precision", old)


def plan_name(cv, mode, B, cin, cout, isz, osz, stride=1, transposed=0, kd=3, k=3, dil=1, vol=0):
    from dsmnet_amd import _lib
    a = _lib.Conv3dArgs()
    a.x = a.w_packed = a.y = a.x_amax = 16
    a.B, a.Cin, a.Cout = B, cin, cout
    a.Di, a.Hi, a.Wi = isz
    a.Do, a.Ho, a.Wo = osz
    a.stride, a.transposed, a.relu, a.kd, a.k, a.dil, a.vol_virtual = stride, transposed, 0, kd, k, dil, vol
    a.precision = {"f16x2": _lib.DSM_PREC_F16X2, "f16": _lib.DSM_PREC_F16, "bf16x3": 0}[mode]
    return cv.conv3d_plan_name(a)


def ksplit_of(name):
    return int(name.split("KS=")[1].split(",")[0].rstrip(">"))


def report(row, cls, mode, r):
    print("CONTRACT %s %s %s %.3f" % (row, cls, mode, r))


def finite_and_amax(y, cls, mode):
    assert torch.isfinite(y).all()
    if cls in ("O4", "O6") and mode != "bf16x3":
        assert y._dsm_amax.item() == y.abs().max().item()


def params(rows, classes=SB.CLASSES):
    """(row, class, mode): f16x2 on every class, the other modes of the row on G, O6 and Q."""
    out = []
    for row, spec in rows.items():
        for mode in spec["modes"]:
            for cls in classes:
                if mode == "f16x2" or cls.split("-")[-1] in SOME:
                    out.append(pytest.param(row, cls, mode, id="%s-%s-%s" % (row, cls, mode)))
    return out


# ------------------------------------------------------------------ forward layers: one launch, one bound --
# kind: c3 Conv3d, t3 ConvTranspose3d (k3 s2 p1 op1), c2 Conv2d; K: products that can be non-zero per output
FWD = {
    "split3d_64_64_s1": dict(kind="c3", shape=(2, 64, 5, 9, 37), cout=64, stride=1, modes=ALL, plan="conv3d_%s_mfma_kernel<"),
    "split3d_32_64_s2": dict(kind="c3", shape=(2, 32, 5, 9, 37), cout=64, stride=2, modes=ALL, plan="conv3d_%s_mfma_kernel<"),
    "split3d_64_32_tr": dict(kind="t3", shape=(2, 64, 5, 9, 37), cout=32, stride=2, modes=BF, plan="deconv3d_%s_mfma_kernel<"),
    "split2d_128_d2": dict(kind="c2", shape=(2, 128, 17, 33), cout=128, stride=1, dil=2, modes=ALL, plan="conv2d_%s_mfma_kernel<"),
    "zs_32_32": dict(kind="c3", shape=(2, 32, 5, 11, 53), cout=32, stride=1, modes=ALL, plan="conv3d_zs_%s_mfma_kernel"),
    "zs_virtual": dict(kind="vol", shape=(4, 32, 11, 53), D=14, cout=32, stride=1, modes=ALL, plan="conv3d_zs_%s_mfma_kernel<vol>"),
    "deconv_zs_64_32": dict(kind="t3", shape=(1, 64, 5, 6, 35), cout=32, stride=2, modes=F16S, plan="deconv3d_zs_%s_mfma_kernel<"),
    "wide_48_256_s1": dict(kind="wide", shape=(2, 48, 7, 11), cout=256, stride=1, modes=F16S, plan="conv2d_wide_%s_mfma_kernel<S=1,"),
    "wide_256_512_s2": dict(kind="wide", shape=(1, 256, 7, 11), cout=512, stride=2, modes=F16S, plan="conv2d_wide_%s_mfma_kernel<S=2,"),
    # backward-data of the row above: the input is that layer's output gradient (1, 512, 4, 6), the output its x
    "wide_256_512_s2_dx": dict(kind="wide_tr", shape=(1, 512, 4, 6), cout=256, out=(7, 11), stride=2, modes=F16S,
                               plan="deconv2d_wide_%s_mfma_kernel<"),
    "k5_16_128": dict(kind="k5", shape=(1, 16, 9, 21), cout=128, stride=2, modes=F16S, plan="conv2d_k5_%s_mfma_kernel<S=2,"),
}


def geometry(spec):
    """(conv as a function of float64 (input, weight), weight shape, the weight's Cout axis, K)."""
    kind, cin, cout, s = spec["kind"], spec["shape"][1], spec["cout"], spec["stride"]
    if kind == "c3":
        return (lambda a, b: F.conv3d(a, b, stride=s, padding=1)), (cout, cin, 3, 3, 3), 0, 27 * cin
    if kind == "vol":
        return (lambda a, b: F.conv3d(a, b, padding=1)), (cout, 2 * cin, 3, 3, 3), 0, 27 * 2 * cin
    if kind == "t3":
        return ((lambda a, b: F.conv_transpose3d(a, b, stride=2, padding=1, output_padding=1)), (cin, cout, 3, 3, 3), 1,
                8 * cin)
    if kind == "c2":
        d = spec["dil"]
        return (lambda a, b: F.conv2d(a, b, padding=d, dilation=d)), (cout, cin, 3, 3), 0, 9 * cin
    if kind == "wide":
        return (lambda a, b: F.conv2d(a, b, stride=s, padding=1)), (cout, cin, 3, 3), 0, 9 * cin
    if kind == "wide_tr":
        Ho, Wo = spec["out"]                              # the weight is the forward layer's (Cout_fwd = cin here)
        return ((lambda a, b: F.conv_transpose2d(a, b, stride=2, padding=1, output_padding=1)[:, :, :Ho, :Wo]),
                (cin, cout, 3, 3), 1, 4 * cin)
    if kind == "k5":
        return (lambda a, b: F.conv2d(a, b, stride=2, padding=2)), (cout, cin, 5, 5), 0, 25 * cin
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def fwd_case(row, cls):
    """Inputs and the float64 terms of one (row, class): computed once, shared by the modes, never modified."""
    spec = FWD[row]
    seed = 7000 + 100 * sorted(FWD).index(row)
    conv, wshape, cout_axis, K = geometry(spec)
    fan = K if spec["kind"] not in ("t3", "wide_tr") else wshape[1] * (27 if spec["kind"] == "t3" else 9)
    w = seeded(seed + 1, *wshape, scale=(2.0 / fan) ** 0.5)
    x, w = SB.make_input(cls, seed, spec["shape"], w)
    c = dict(x=x, w=w, K=K, x_amax=x.abs().max().item(), scale=None, shift=None, res=None, relu=1)
    operand = x
    if spec["kind"] == "vol":                            # x: both views' maps; the layer multiplies the volume
        from oracle import ops as OO
        operand = OO.concat_volume(x[:2], x[2:], spec["D"], mask_left=True)
    t = SB.conv_terms(operand, w, conv, cout_axis)
    cout = spec["cout"]
    if spec["kind"] in ("c3", "t3", "c2", "vol"):         # folded BN, skip, ReLU: the towers' and the trunk's form
        c["scale"], c["shift"] = seeded(seed + 2, cout).abs() + 0.5, seeded(seed + 3, cout) * 0.2
        if spec["kind"] != "vol":
            c["res"] = seeded(seed + 4, *t["pre"].shape)
    elif spec["kind"] in ("wide", "k5"):                  # bias with the spread of the output + ReLU
        c["scale"] = torch.ones(cout)
        c["shift"] = (seeded(seed + 3, cout).double() * t["pre"].std()).float()
    else:
        c["relu"] = 0                                    # the backward-data launch has no epilogue
    c["t"] = t
    return c


def fwd_plan(cv, row, mode):
    spec = FWD[row]
    shape, cout, s, kind = spec["shape"], spec["cout"], spec["stride"], spec["kind"]
    if kind in ("c3", "t3"):
        name = plan_name(cv, mode, shape[0], shape[1], cout, shape[2:], cv.conv3d_out_size(shape[2:], s, kind == "t3"), s,
                         int(kind == "t3"))
    elif kind == "vol":
        vs = (spec["D"],) + tuple(shape[2:])
        name = plan_name(cv, mode, shape[0] // 2, 2 * shape[1], cout, vs, vs, vol=1)
    elif kind == "wide_tr":
        name = plan_name(cv, mode, shape[0], shape[1], cout, (1,) + tuple(shape[2:]), (1,) + tuple(spec["out"]), 2, 1, kd=1)
    else:
        osz = (1, (shape[2] - 1) // s + 1, (shape[3] - 1) // s + 1)
        name = plan_name(cv, mode, shape[0], shape[1], cout, (1,) + tuple(shape[2:]), osz, s, kd=1, k=5 if kind == "k5" else 3,
                         dil=spec.get("dil", 1))
    want = spec["plan"] % mode
    assert name.startswith(want) and (name == want or want[-1] in "<,"), (name, want)
    return name


def fwd_run(cv, row, c):
    spec = FWD[row]
    kind, cout, s = spec["kind"], spec["cout"], spec["stride"]
    g = lambda v: None if v is None else v.cuda()        # noqa: E731
    x, w = c["x"].cuda(), c["w"].cuda()
    if kind in ("c3", "t3"):
        return cv.conv3d_block(x, cv.pack_conv3d_weight(w, kind == "t3"), cout, g(c["scale"]), g(c["shift"]), g(c["res"]),
                               s, kind == "t3", c["relu"])
    if kind == "vol":
        both = x.contiguous(memory_format=CL)
        return cv.conv3d_block(cv.VirtualVolume(both, spec["D"], True), cv.pack_conv3d_weight(w, False), cout,
                               g(c["scale"]), g(c["shift"]), relu=c["relu"])
    x = x.contiguous(memory_format=CL)
    if kind == "wide_tr":
        return cv.conv2d_transposed_block(x, cv.pack_conv2d_weight(w.flip(2, 3).transpose(0, 1).contiguous()), cout, spec["out"])
    return cv.conv2d_block(x, cv.pack_conv2d_weight(w), cout, g(c["scale"]), g(c["shift"]), g(c["res"]), stride=s,
                           relu=c["relu"], k=5 if kind == "k5" else 3, dilation=spec.get("dil", 1))


@pytest.mark.parametrize("row,cls,mode", params(FWD))
def test_forward_layers_hold_the_per_element_bound(cv, row, cls, mode):
    c = fwd_case(row, cls)
    with precision(cv, mode):
        name = fwd_plan(cv, row, mode)
        y = fwd_run(cv, row, c)
    ks = ksplit_of(name) if "KS=" in name else 1
    ref, bound = SB.bound_from_terms(c["t"], mode, SB.n_forward(mode, c["K"], ks), c["x_amax"], c["w"].abs().max().item(),
                                     c["scale"], c["shift"], c["res"])
    assert tuple(y.shape) == tuple(ref.shape)
    r = SB.ratio(y, ref.relu() if c["relu"] else ref, bound)
    report(row, cls, mode, r)
    finite_and_amax(y, cls, mode)
    assert r <= 1.0, r


# ----------------------------------------------------------------------------- the fused BasicBlock (2-D) --
# "_id": the first layer is the identity (centre tap 1, scale 1, shift 0), so the SECOND layer's split sees
# relu(class) itself and E1 is one layer's bound on |x|, not on a 9 C-term sum: the propagated term no longer
# swamps the second layer's own bound, and a fault in the intermediate's split (per-tile scale, subnormal
# residuals) shows.  The bound is the same formula, nothing in it knows about the identity.
BLOCKS = {"basicblock_32": dict(C=32, modes=F16S), "basicblock_64": dict(C=64, modes=F16S),
          "basicblock_32_id": dict(C=32, modes=F16S, identity=True), "basicblock_64_id": dict(C=64, modes=F16S, identity=True)}


@functools.lru_cache(maxsize=None)
def block_case(row, cls):
    C = BLOCKS[row]["C"]
    seed = 8000 + 100 * C
    w1 = seeded(seed + 1, C, C, 3, 3, scale=(2.0 / (9 * C)) ** 0.5)
    w2 = seeded(seed + 2, C, C, 3, 3, scale=(2.0 / (9 * C)) ** 0.5)
    x, w1 = SB.make_input(cls, seed, (2, C, 13, 37), w1)
    s1, h1 = seeded(seed + 3, C).abs() + 0.5, seeded(seed + 4, C)
    if BLOCKS[row].get("identity"):
        w1 = torch.zeros(C, C, 3, 3)
        w1[torch.arange(C), torch.arange(C), 1, 1] = 1.0
        s1, h1 = torch.ones(C), torch.zeros(C)
        if cls == "Wt":                                  # the loud tap goes to the second layer's weights
            w2 = SB.make_input(cls, seed, (2, C, 13, 37), w2)[1]
    s2, h2 = seeded(seed + 5, C).abs() + 0.5, seeded(seed + 6, C)
    return dict(x=x, w1=w1, w2=w2, s1=s1, h1=h1, s2=s2, h2=h2)


@functools.lru_cache(maxsize=None)
def block_bound(row, cls, mode):
    c, C = block_case(row, cls), BLOCKS[row]["C"]
    n = SB.n_forward(mode, 9 * C)
    return SB.chain_bound(c["x"], c["w1"], c["w2"], lambda a, b: F.conv2d(a, b, padding=1), mode, n, n,
                          c["x"].abs().max().item(), c["s1"], c["h1"], c["s2"], c["h2"], res=c["x"])


@pytest.mark.parametrize("row,cls,mode", params(BLOCKS))
def test_the_fused_block_holds_the_propagated_bound(cv, row, cls, mode):
    c, C = block_case(row, cls), BLOCKS[row]["C"]
    timer = cv.LaunchTimer()
    with precision(cv, mode):
        cv.set_timer(timer)
        try:
            y = cv.basicblock2d(c["x"].cuda().contiguous(memory_format=CL), cv.pack_conv2d_weight(c["w1"].cuda()),
                                c["s1"].cuda(), c["h1"].cuda(), cv.pack_conv2d_weight(c["w2"].cuda()), c["s2"].cuda(),
                                c["h2"].cuda(), relu=True, skip=True)
        finally:
            torch.cuda.synchronize()
            cv.set_timer(None)
    launched = [k for k in timer.summary() if k != "absmax_kernel"]          # the maximum of x, then the block alone
    assert launched == ["basicblock2d_%s_mfma_kernel<C=%d>" % (mode, C)], timer.summary()
    ref, bound = block_bound(row, cls, mode)
    r = SB.ratio(y, ref.relu(), bound)
    report(row, cls, mode, r)
    finite_and_amax(y, cls, mode)
    assert r <= 1.0, r


# -------------------------------------------------------------------------------------- weight gradients --
# TY: G rows per tile of wgrad_split_kernel (conv3d_bwd.hip: 3-D S = 1 -> 4, S = 2 -> 1; 2-D S = 1 -> 8)
WGRAD = {
    "wgrad3d_32_32_s1": dict(shape=(1, 32, 5, 9, 37), cg=32, stride=1, TY=4, modes=ALL, label="conv3d_wgrad_%s_kernel<S=1,32x32>"),
    "wgrad3d_32_64_s2": dict(shape=(1, 32, 5, 9, 37), cg=64, stride=2, TY=1, modes=ALL, label="conv3d_wgrad_%s_kernel<S=2,32x64>"),
    "wgrad2d_64_64": dict(shape=(2, 64, 13, 37), cg=64, stride=1, TY=8, modes=ALL, label="conv2d_wgrad_kernel"),
}
WGRAD_CLASSES = ("G",) + tuple("%s-%s" % (o, k) for o in "XG" for k in ("O4", "O6", "Q", "L", "C", "Z"))


@functools.lru_cache(maxsize=None)
def wgrad_case(row, cls):
    spec = WGRAD[row]
    seed = 9000 + 100 * sorted(WGRAD).index(row)
    shape, cg, s = spec["shape"], spec["cg"], spec["stride"]
    gshape = (shape[0], cg) + tuple((v - 1) // s + 1 for v in shape[2:])
    who, _, k = cls.rpartition("-")
    x = SB.make_input(k if who == "X" else "G", seed, shape)[0]
    g = SB.make_input(k if who == "G" else "G", seed + 1, gshape)[0]
    wsize = (cg, shape[1]) + (3,) * (len(shape) - 2)
    grad = torch.nn.grad.conv3d_weight if len(shape) == 5 else torch.nn.grad.conv2d_weight
    # (X, G) in the places of (x, w): the "output channel" of the sum over voxels is G's, axis 0 of dW
    t = SB.conv_terms(x, g, lambda a, b: grad(a, wsize, b, stride=s, padding=1), cout_axis=1, out_axis=0)
    return dict(x=x, g=g, t=t)


def wgrad_n(row, mode):
    spec = WGRAD[row]
    shape, cg, s, TY = spec["shape"], spec["cg"], spec["stride"], spec["TY"]
    og = [(v - 1) // s + 1 for v in shape[2:]]
    Dg = og[0] if len(og) == 3 else 1
    tiles = shape[0] * Dg * -(-og[-2] // TY) * -(-og[-1] // 32)
    pairs = (shape[1] // 32) * (cg // 32)
    return SB.n_wgrad(mode, tiles, TY, min(max(256 // pairs, 1), tiles), len(og) == 2)


@pytest.mark.parametrize("row,cls,mode", params(WGRAD, WGRAD_CLASSES))
def test_weight_gradients_hold_the_per_element_bound(cv, row, cls, mode):
    spec, c = WGRAD[row], wgrad_case(row, cls)
    timer = cv.LaunchTimer()
    with precision(cv, mode):
        cv.set_timer(timer)
        try:
            if len(spec["shape"]) == 5:
                dw = cv._wgrad(cv.to_channels_last_3d(c["x"].cuda()), cv.to_channels_last_3d(c["g"].cuda()),
                               spec["shape"][1], spec["cg"], spec["stride"])
            else:
                dw = cv._wgrad2d(c["x"].cuda().contiguous(memory_format=CL), c["g"].cuda().contiguous(memory_format=CL),
                                 spec["stride"], 1)
        finally:
            torch.cuda.synchronize()
            cv.set_timer(None)
    label = spec["label"] % mode if "%s" in spec["label"] else spec["label"]
    assert label in timer.summary(), timer.summary()
    ref, bound = SB.bound_from_terms(c["t"], mode, wgrad_n(row, mode), c["x"].abs().max().item(), c["g"].abs().max().item())
    r = SB.ratio(dw, ref, bound)
    report(row, cls, mode, r)
    assert torch.isfinite(dw).all()
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------- range edges --
# The supported range of a tensor's maximum is [2^-48, 2^76) (include/dsmnet_hip.h at DSM_PREC_F16X2): inside it
# the clamp of the exponent rule never binds below (2^-48 -> e = 60) and the scaled maximum stays under fp16's
# 65504 above (2^75 2^-60 = 2^15).  Below it the scaled values sink towards fp16's subnormals: the floor of the
# bound, taken with the CLAMPED exponent, says by how much -- the result degrades, it is never NaN.
@pytest.mark.parametrize("target", [2.0 ** -48, 2.0 ** 75, 2.0 ** -70], ids=["2^-48", "2^75", "2^-70"])
@pytest.mark.parametrize("row", ["zs_32_32", "wide_48_256_s1"])
def test_range_edges(cv, row, target):
    base = fwd_case(row, "G")
    x = SB.with_max(base["x"], target)
    assert x.abs().max().item() == target
    conv, _, cout_axis, K = geometry(FWD[row])
    c = dict(base, x=x, scale=None, shift=None, res=None)
    t = SB.conv_terms(x, c["w"], conv, cout_axis)
    with precision(cv, "f16x2"):
        name = fwd_plan(cv, row, "f16x2")
        y = fwd_run(cv, row, c)
    ks = ksplit_of(name) if "KS=" in name else 1
    ref, bound = SB.bound_from_terms(t, "f16x2", SB.n_forward("f16x2", K, ks), target, c["w"].abs().max().item())
    r = SB.ratio(y, ref.relu(), bound)
    rel = (y.double().cpu() - ref.relu()).abs().max().item() / ref.abs().max().item()
    report(row, "max=%s" % ("2^%d" % round(torch.tensor(target).log2().item())), "f16x2", r)
    print("   max|err| / max|ref| = %.2e" % rel)
    assert torch.isfinite(y).all() and y.abs().max().item() > 0
    assert r <= 1.0, r


# ------------------------------------------------------- PSMNet under a rescaling that changes nothing --
# conv + BN + ReLU -> conv: BN weight and bias of one output channel x s, the next layer's weights for that input
# channel / s, s = 2^12 -- exact in every fold (a power of two), and ReLU commutes with a positive scale: the
# function, and so the reference's golden, is the same.  Only the state dict changes.  What does change is the
# maximum the next layer's fp16 split is scaled by: every other channel now sits 2^-12 below it.
#   firstconv[0] -> firstconv[2] (models/psmnet/submodule.py:69-74): feeds the fused block;
#   dres0[0] -> dres0[2] (stackhourglass.py:73-76): feeds conv_zs.
SITES = {"firstconv": ("feature_extraction.firstconv.0.1", "feature_extraction.firstconv.2.0.weight"),
         "dres0": ("dres0.0.1", "dres0.2.0.weight")}
RESCALE, CHANNEL = 2.0 ** 12, 3
_runs = {}


def psmnet_run(cv, golden_e2e, mode, site):
    """The three heads of the golden checkpoint (rescaled at ``site``, or as it is: None) in ``mode``; run once."""
    if (mode, site) not in _runs:
        from tests.golden.make_goldens import images
        from tests.helpers import golden_state
        from dsmnet_amd.models import model_create_by_name
        sd, cfg = golden_state(golden_e2e, "psmnet")
        if site is not None:
            bn, nxt = SITES[site]
            sd = {k: v.clone() for k, v in sd.items()}
            sd[bn + ".weight"][CHANNEL] *= RESCALE
            sd[bn + ".bias"][CHANNEL] *= RESCALE
            sd[nxt][:, CHANNEL] /= RESCALE
        imL, imR = images(cfg["image_seed"], *cfg["hw"])
        m = model_create_by_name("psmnet", 192)
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        with precision(cv, mode), torch.no_grad():
            _runs[mode, site] = [p.detach().clone() for p in m(imL.cuda(), imR.cuda())[1]]
    return _runs[mode, site]


@pytest.mark.parametrize("site", sorted(SITES))
def test_psmnet_is_unchanged_by_an_exact_rescaling_of_one_channel(cv, golden_e2e, site):
    names = ("pred3", "pred2", "pred1")
    plain, scaled = psmnet_run(cv, golden_e2e, "bf16x3", None), psmnet_run(cv, golden_e2e, "bf16x3", site)
    same = all(torch.equal(a, b) for a, b in zip(plain, scaled))
    print("%s x 2^12, bf16x3: %s" % (site, "bit-identical to the unrescaled run" if same else "NOT bit-identical"))
    for name, a, b in zip(names, plain, scaled):
        d = (a - b).abs().max().item()
        print("   bf16x3 %s: %.2e px from the unrescaled run" % (name, d))
        assert d <= 1e-5, (name, d)
    f_plain, f_scaled = psmnet_run(cv, golden_e2e, "f16x2", None), psmnet_run(cv, golden_e2e, "f16x2", site)
    # the rescaled channel is alive: the f16x2 split of the next layer's input really is scaled differently
    assert not all(torch.equal(a, b) for a, b in zip(f_plain, f_scaled))
    for name, p, q in zip(names, f_scaled, f_plain):
        print("   f16x2 %s: %.2e px from its unrescaled run" % (name, (p - q).abs().max().item()))
    for name, p in zip(names, f_scaled):
        err = golden_e2e.compare("e2e.psmnet." + name, p, 1e-3)
        print("   f16x2 %s: %.2e px from the golden" % (name, err))
