"""GPU parity: gradients of the 3-D convolution blocks (bwd-data on the forward kernels with
re-packed weights, bwd-weight on the voxel-reduction MFMA kernel) against torch's CPU autograd,
and a PSMNet trunk training step against the oracle's autograd (BASELINE config #5 in fp32).

Tolerances: gradients are sums over up to 1e5 voxels of O(1) products in fp32 with atomics
(order varies): 1e-3 relative to the largest gradient entry."""
import pytest
import torch
import torch.nn.functional as F

from oracle import models as OM
from oracle import ops as OO
from tests.golden.make_goldens import randomise_bn
from tests.helpers import maxerr, seeded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


@pytest.mark.parametrize("cin,cout,stride,transposed,shape,bias", [
    (32, 32, 1, False, (1, 6, 12, 40), False), (64, 32, 1, False, (1, 5, 9, 33), True),
    (64, 64, 1, False, (2, 3, 7, 35), False),
    (32, 64, 2, False, (1, 6, 12, 40), False), (64, 64, 2, False, (1, 5, 9, 37), True),
    (64, 64, 2, True, (1, 3, 6, 20), False), (64, 32, 2, True, (1, 3, 5, 33), True),
    (32, 1, 1, False, (1, 5, 9, 37), False),
    (32, 1, 2, True, (1, 4, 7, 19), True),          # GCNet's head l37 (gcnet.py:63): ADVICE r1
])
def test_conv3d_function_gradients(cv, cin, cout, stride, transposed, shape, bias):
    B, D, H, W = shape
    x = seeded(1, B, cin, D, H, W).requires_grad_(True)
    wshape = (cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3)
    w = seeded(2, *wshape, scale=0.1).requires_grad_(True)
    b = seeded(3, cout, scale=0.1).requires_grad_(True) if bias else None
    if transposed:
        ref = F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)
    else:
        ref = F.conv3d(x, w, b, stride=stride, padding=1)
    cot = seeded(4, *ref.shape)
    grads = torch.autograd.grad(ref, [t for t in (x, w, b) if t is not None], cot)
    xg = x.detach().cuda().requires_grad_(True)
    wg = w.detach().cuda().requires_grad_(True)
    bg = b.detach().cuda().requires_grad_(True) if bias else None
    y = cv.conv3d(xg, wg, bg, stride, transposed)
    assert maxerr(y, ref) <= 2e-4
    got = torch.autograd.grad(y, [t for t in (xg, wg, bg) if t is not None], cot.cuda())
    for name, g, r in zip(("dx", "dw", "db"), got, grads):
        tol = 1e-3 * max(1.0, r.abs().max().item())
        assert g.shape == r.shape, name
        assert maxerr(g, r) <= tol, "%s: %.3e > %.3e" % (name, maxerr(g, r), tol)


class _SignLog(object):
    """Records the sign pattern of every tensor that enters a ReLU (as CPU bool masks)."""

    def __init__(self):
        self.masks = []

    def wrap(self, fn):
        def relu(x, *a, **k):
            self.masks.append((x.detach() > 0).cpu())
            return fn(x, *a, **k)
        return relu


def _trunk_step_errors(seed, hw=(16, 40), d4=8, batch=1):
    """One train-mode trunk + heads step on a seeded input: relative max-abs error of every
    checked gradient against the oracle's CPU autograd, and the number of ReLU inputs whose SIGN
    differs between the two implementations.

    The backward of a ReLU network is discontinuous: an activation within rounding distance of zero
    can take the other side in the two implementations, and then the gradients legitimately differ
    by what that unit carries.  The discontinuity is REMOVED here instead of budgeted for (ADVICE
    r02): the product runs first and records the sign pattern of every ReLU input; the oracle's
    trunk then runs with those masks forced (y = x * mask_k in place of its k-th F.relu -- the same
    function wherever the signs agree, and the same derivative everywhere).  What is left is
    arithmetic: summation order and the products' precision.

    The oracle runs in float64.  Its fp32 CPU autograd is not accurate enough to judge the product at
    GRAD_TOL: at the config #5 shape, with the same masks, its weight gradients lie up to 2e-3 (relative
    to the largest entry) from its own float64 result -- classif3.0.0.weight, summed over 1.6e6 voxels
    with heavy cancellation -- and by how much depends on the host's thread count."""
    import torch.nn.functional as TF
    from dsmnet_amd import blocks3d
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd.models import model_create_by_name
    sd = randomise_bn(OM.init_state("psmnet", 0), 41)
    OM.apply_head_scale("psmnet", sd, 0.05)
    fl, fr = seeded(seed, batch, 32, *hw), seeded(seed + 1, batch, 32, *hw)
    size = (4 * d4, 4 * hw[0], 4 * hw[1])
    keys = ["dres0.0.0.weight", "dres0.0.1.weight", "dres1.2.0.weight", "dres2.conv1.0.0.weight",
            "dres2.conv5.0.weight", "dres3.conv6.0.weight", "dres4.conv2.1.bias",
            "classif1.2.weight", "classif3.0.0.weight"]
    # product first: forward with the sign pattern of every ReLU input recorded
    m = model_create_by_name("psmnet", 192)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    gfl, gfr = fl.cuda().requires_grad_(True), fr.cuda().requires_grad_(True)
    glog = _SignLog()
    # the product's train-mode blocks are fused (BatchNorm + add + ReLU in one kernel): the sign
    # pattern of the ReLU's input is read off the block's output (out > 0 <=> input > 0)
    blocks3d._TRAIN_RELU_HOOK[0] = lambda out, mode, residual: glog.masks.append((out.detach() > 0).cpu())
    orig_t = torch.relu
    torch.relu = glog.wrap(orig_t)                 # (DSM_TRAIN_BN=stock: blocks3d calls torch.relu)
    try:
        gc = m.regularise(cv.concat_volume(gfl, gfr, d4, True))
    finally:
        torch.relu = orig_t
        blocks3d._TRAIN_RELU_HOOK[0] = None
    loss = sum(cv.soft_argmin(c, size).mean() for c in gc)
    assert len(glog.masks) == 21, len(glog.masks)
    params = dict(m.named_parameters())
    ggr = torch.autograd.grad(loss, [params[k] for k in keys] + [gfl, gfr])
    # oracle: leaves that require grad; its k-th ReLU takes the product's k-th mask
    osd = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k
               else v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    ofl, ofr = fl.double().requires_grad_(True), fr.double().requires_grad_(True)
    n = OM.Net(osd, training=True)
    state = {"k": 0, "flips": 0, "units": 0}

    def forced_relu(x, *a, **k):
        mask = glog.masks[state["k"]]
        assert mask.shape == x.shape, (state["k"], mask.shape, x.shape)
        state["k"] += 1
        state["flips"] += int(((x.detach() > 0) != mask).sum())
        state["units"] += mask.numel()
        return x * mask.to(x.dtype)

    orig = TF.relu
    TF.relu = forced_relu                          # the oracle's trunk calls F.relu
    try:
        costs = OM.psmnet_trunk(n, OO.concat_volume(ofl, ofr, d4, True))
    finally:
        TF.relu = orig
    assert state["k"] == 21
    oloss = sum(OO.soft_argmin(c, size).mean() for c in costs)
    ogr = torch.autograd.grad(oloss, [osd[k] for k in keys] + [ofl, ofr])
    assert abs(loss.item() - oloss.item()) <= 1e-3 * max(1.0, abs(oloss.item()))
    for a, b in zip(gc, costs):                                   # train-mode forward: tight
        assert maxerr(a, b) <= 2e-5 * b.abs().max().item()
    # running statistics were updated as nn.BatchNorm3d does
    assert maxerr(m.dres0[0][1].running_mean, osd["dres0.0.1.running_mean"]) <= 1e-4
    errs = {k: maxerr(g, r) / max(r.abs().max().item(), 1e-6)
            for k, g, r in zip(keys + ["fL", "fR"], ggr, ogr)}
    return errs, state["flips"], state["units"]


GRAD_TOL = 1e-4      # relative to the largest entry of each gradient, same ReLU masks on both sides


def _check_gradients(errs, flips, units):
    """With the ReLU masks forced the gradients must agree to GRAD_TOL (measured ~3e-6: summation
    order and the products' precision).  The flip count stays as a sanity line of its own: rounding
    noise flips a ReLU input only when it lies within ~1e-6 of zero relative to the layer's scale --
    at most a few per million units (measured 330 of 4.6e8 at the config #5 shape)."""
    worst = max(errs.values())
    print("gradients vs the mask-forced oracle: worst relative error %.2e; %d of %d ReLU inputs had "
          "the other sign in the oracle's own forward" % (worst, flips, units))
    assert worst <= GRAD_TOL, "worst %.3e (flips=%d): %r" % (worst, flips, errs)
    assert flips <= 16 + 3e-6 * units, "too many sign flips (%d of %d) for rounding noise" % (flips, units)


def test_psmnet_trunk_training_step_vs_oracle(hip_lib):
    """Train-mode forward + backward through the whole 3-D trunk and the three fused heads:
    parameter and input gradients against the oracle's CPU autograd, on three seeds.

    The forward agrees to ~3e-6 on every input; the oracle's backward runs with the product's ReLU
    masks forced (see _trunk_step_errors), so every gradient must agree to GRAD_TOL on every seed."""
    for seed in (81, 71, 101):
        errs, flips, units = _trunk_step_errors(seed)
        _check_gradients(errs, flips, units)


def test_psmnet_trunk_training_step_at_config5_shape(hip_lib):
    """BASELINE config #5's own 1/4-resolution shape, one pair: features (1,32,135,240), D/4 = 48
    (540x960, D=192).  The odd sizes exercise the crop of ``myadd_3d`` on every level
    (135 -> 68 -> 34 -> 68 -> 136 vs 135; stackhourglass.py:10-20) in forward AND backward.
    Gradients against the oracle's CPU autograd with the product's ReLU masks forced: GRAD_TOL."""
    errs, flips, units = _trunk_step_errors(91, hw=(135, 240), d4=48)
    _check_gradients(errs, flips, units)


def test_psmnet_trunk_training_step_batch_2_odd_sizes(hip_lib):
    """Two pairs, features (2,32,15,38), D/4 = 7: every ``myadd_3d`` crop in forward and backward
    (7 -> 4 -> 2 -> 4 -> 8 vs 7; 15 -> 8 -> 4 -> 8 -> 16 vs 15; 38 -> 19 -> 10 -> 20 vs 19) with a batch
    boundary inside every kernel's work list.  Same bound and flip budget as at batch 1."""
    errs, flips, units = _trunk_step_errors(61, hw=(15, 38), d4=7, batch=2)
    _check_gradients(errs, flips, units)


def _gcnet_step_errors(seed, batch=2, hw=(21, 42), d2=12):
    """``_trunk_step_errors`` for GCNet: 3-D trunk (models/gcnet.py:65-101) + the transposed 32 -> 1 head
    ``l37`` + soft-argmin of the negated cost, in train mode, on a seeded 1/2-resolution feature pair.

    GCNet's blocks end in their own ReLU and add the skip AFTER it (``relu == RELU_BEFORE_ADD``), so the
    sign of the ReLU's input is not ``out > 0`` there: it is ``out > residual`` on the cropped corner the
    output covers.  Outside that corner the transposed convolution's values are dropped by the crop and
    carry no gradient: the oracle keeps its own sign there.  A positive value that the addition absorbs
    (relu(y) + r == r in fp32) reads as a flip and is counted by the flip budget.
    Sizes: (12,21,42) -> (6,11,21) -> (3,6,11) -> (2,3,6) -> (1,2,3) and back up through
    (2,4,6) / (4,6,12) / (6,12,22) / (12,22,42): every skip addition crops."""
    import torch.nn.functional as TF
    from dsmnet_amd import blocks3d
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd.models import model_create_by_name
    sd = randomise_bn(OM.init_state("gcnet", 0), 43)
    OM.apply_head_scale("gcnet", sd, 0.05)
    fl, fr = seeded(seed, batch, 32, *hw), seeded(seed + 1, batch, 32, *hw)
    keys = ["layer3d.l19.0.weight", "layer3d.l22.0.weight", "layer3d.l32.0.weight",      # stride 1
            "layer3d.l21.0.weight", "layer3d.l30.0.weight",                              # stride 2
            "layer3d.l33.0.weight", "layer3d.l34.0.weight", "layer3d.l36.0.weight",      # transposed + skip
            "layer3d.l35.1.weight", "layer3d.l36.1.bias",                                # BN before a ReLU + add
            "layer3d.l37.weight"]      # (l37.bias: the soft-argmin is shift invariant, its gradient is 0)
    m = model_create_by_name("gcnet", 2 * d2)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    gfl, gfr = fl.cuda().requires_grad_(True), fr.cuda().requires_grad_(True)
    glog = _SignLog()

    def hook(out, mode, res=None):
        out = out.detach()
        if mode == blocks3d.RELU_BEFORE_ADD and res is not None:
            d, h, w = out.shape[2:]
            glog.masks.append((out > res.detach()[:, :, :d, :h, :w]).cpu())
        else:
            glog.masks.append((out > 0).cpu())

    blocks3d._TRAIN_RELU_HOOK[0] = hook
    orig_t = torch.relu
    torch.relu = glog.wrap(orig_t)                 # (DSM_TRAIN_BN=stock: blocks3d calls torch.relu)
    try:
        gcost = m.layer3d.cost(cv.concat_volume(gfl, gfr, d2, False))
    finally:
        torch.relu = orig_t
        blocks3d._TRAIN_RELU_HOOK[0] = None
    loss = cv.soft_argmin(gcost, None, negate=True).mean()
    assert len(glog.masks) == 18, len(glog.masks)
    params = dict(m.named_parameters())
    ggr = torch.autograd.grad(loss, [params[k] for k in keys] + [gfl, gfr])
    osd = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k
               else v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    ofl, ofr = fl.double().requires_grad_(True), fr.double().requires_grad_(True)
    n = OM.Net(osd, training=True)
    state = {"k": 0, "flips": 0, "units": 0}

    def forced_relu(x, *a, **k):
        mask = glog.masks[state["k"]]
        state["k"] += 1
        own = x.detach() > 0
        assert mask.shape[:2] == x.shape[:2] and all(a <= b for a, b in zip(mask.shape[2:], x.shape[2:]))
        d, h, w = mask.shape[2:]
        state["flips"] += int((own[:, :, :d, :h, :w] != mask).sum())
        state["units"] += mask.numel()
        own[:, :, :d, :h, :w] = mask               # outside the skip's corner: no gradient, own sign
        return x * own.to(x.dtype)

    orig = TF.relu
    TF.relu = forced_relu                          # the oracle's trunk calls F.relu
    try:
        ocost = OM.gcnet_trunk(n, OO.concat_volume(ofl, ofr, d2, False))
    finally:
        TF.relu = orig
    assert state["k"] == 18
    oloss = OO.soft_argmin(ocost, None, negate=True).mean()
    ogr = torch.autograd.grad(oloss, [osd[k] for k in keys] + [ofl, ofr])
    assert tuple(gcost.shape) == tuple(ocost.shape) == (batch, 1, 2 * d2, 2 * hw[0], 2 * hw[1])
    assert abs(loss.item() - oloss.item()) <= 1e-3 * max(1.0, abs(oloss.item()))
    assert maxerr(gcost, ocost) <= 2e-5 * ocost.abs().max().item()
    errs = {k: maxerr(g, r) / max(r.abs().max().item(), 1e-6)
            for k, g, r in zip(keys + ["fL", "fR"], ggr, ogr)}
    return errs, state["flips"], state["units"]


def test_gcnet_trunk_training_step_vs_oracle(hip_lib):
    """GCNet's backward against the oracle's float64 autograd with the product's ReLU masks forced: the
    only user of ReLU-before-add in the BatchNorm backward and of the transposed Cout = 1 head.  Batch 2,
    odd sizes; weights of stride-1, stride-2 and transposed layers with skip, BN parameters, ``l37``, and
    both feature inputs at GRAD_TOL."""
    errs, flips, units = _gcnet_step_errors(83)
    print({k: "%.1e" % v for k, v in errs.items()})
    _check_gradients(errs, flips, units)


def test_psmnet_full_training_step(hip_lib):
    """BASELINE config #5 in miniature (fp32, 1 GPU): PSMNet in train mode, 256x512, D=192:
    forward with batch-statistics BN, smooth-L1 loss on the three heads, backward through the
    HIP trunk and the stock-torch towers, one SGD step; every parameter receives a finite
    gradient and the loss on the same pair goes down."""
    from dsmnet_amd import sharding
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(0)
    m = model_create_by_name("psmnet", 192).cuda().train()
    for i in (1, 2, 3):                                   # sane logit scale for a random init
        with torch.no_grad():
            getattr(m, "classif%d" % i)[2].weight.mul_(1e-3)
    g = torch.Generator().manual_seed(5)
    left = torch.rand(1, 3, 256, 512, generator=g).cuda()
    right = torch.roll(left, -6, dims=3)
    target = torch.full((1, 256, 512), 6.0, device="cuda")
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)

    def step():
        opt.zero_grad()
        _, preds = m(left, right)
        loss = sum(w * F.smooth_l1_loss(p, target) for w, p in zip((1.0, 0.7, 0.5), preds))
        loss.backward()
        return loss

    l0 = step()
    missing = [n for n, p in m.named_parameters() if p.grad is None]
    assert not missing, missing[:5]
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    assert sharding.allreduce_gradients(m.parameters(), world=1) == 0    # single process: no-op
    opt.step()
    l1 = step()
    assert torch.isfinite(l0) and torch.isfinite(l1)
    assert l1.item() < l0.item(), (l0.item(), l1.item())


def _config5_batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    left = torch.rand(B, 3, 540, 960, generator=g)
    right = torch.roll(left, -9, dims=3)
    disp = torch.full((B, 1, 540, 960), 9.0)
    disp[:, :, :, :9] = 0
    return torch.cat([left, right, disp], 1).cuda()


def test_config5_psmnet_train_step_540x960_four_pairs(hip_lib):
    """BASELINE config #5 at its real per-GPU shape: ``train.train_step`` on PSMNet, 540x960,
    D=192, 4 pairs on one GPU (the share of batch 32 over 8 GPUs; the gradient all-reduce of
    the other 7 is covered by the world-size-2 gloo tests).  fp32, as the reference computes
    (stackhourglass.py:124); tests/test_train_f16_gpu.py runs the same step in the fp16 mode of
    config #5.  Checks: the volume convolution (4,64,48,135,240) = 1.59 GB runs on the z-sliding
    kernel (32-bit offsets per input plane), every parameter gets a finite gradient, the loss is finite
    and decreases over Adam steps on the same batch, peak memory is reported."""
    import ctypes
    from dsmnet_amd import _lib, costvolume as cv, train
    from dsmnet_amd.models import model_create_by_name
    a = _lib.Conv3dArgs()
    a.B, a.Cin, a.Cout = 4, 64, 32
    a.Di, a.Hi, a.Wi = 48, 135, 240
    a.Do, a.Ho, a.Wo = 48, 135, 240
    a.stride, a.transposed, a.relu = 1, 0, 0
    a.x = a.w_packed = a.y = 16                       # the plan looks at shapes only
    assert "conv3d_zs_" in cv.conv3d_plan_name(a), cv.conv3d_plan_name(a)
    torch.manual_seed(0)
    model = model_create_by_name("psmnet", 192).cuda()
    for i in (1, 2, 3):
        with torch.no_grad():
            getattr(model, "classif%d" % i)[2].weight.mul_(1e-3)
    lossfun = train.losses("supervised", model.count_levels, 0)
    lossfun.Weight_Adjust_levels(0)
    opt = train.make_optimizer(model, lr=1e-3)
    batch = _config5_batch(4, 11)
    torch.cuda.reset_peak_memory_stats()
    losses = [train.train_step(model, opt, lossfun, batch)[0] for _ in range(3)]
    assert all(l == l and abs(l) < 1e6 for l in losses), losses
    assert losses[-1] < losses[0], losses
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print("config #5 step: losses %s, peak memory %.1f GiB" % (["%.4f" % l for l in losses], peak))
    assert peak < 200.0


def test_gcnet_train_step(hip_lib):
    """One supervised step through GCNet: the transposed 32 -> 1 head ``l37``
    (gcnet.py:63,98) has its own backward kernels; every parameter gets a finite gradient and
    the loss goes down."""
    from dsmnet_amd import train
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(0)
    model = model_create_by_name("gcnet", 64).cuda()
    with torch.no_grad():
        model.layer3d.l37.weight.mul_(0.05)
    lossfun = train.losses("supervised", model.count_levels, 0)
    lossfun.Weight_Adjust_levels(0)
    opt = train.make_optimizer(model, lr=1e-3)
    g = torch.Generator().manual_seed(3)
    left = torch.rand(1, 3, 64, 128, generator=g)
    right = torch.roll(left, -5, dims=3)
    disp = torch.full((1, 1, 64, 128), 5.0)
    batch = torch.cat([left, right, disp], 1).cuda()
    losses = [train.train_step(model, opt, lossfun, batch)[0] for _ in range(4)]
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert losses[-1] < losses[0], losses


@pytest.mark.parametrize("stride,shape", [(1, (1, 6, 12, 40)), (2, (1, 5, 9, 37))])
def test_wgrad_exact_fp32_kernel_option(cv, stride, shape):
    """``conv_fp32`` (DSM_CONV_FP32_MFMA in the wgrad flags) keeps the fp32-input MFMA weight-gradient
    kernel; both kernels agree with the fp64 reference."""
    B, D, H, W = shape
    x = seeded(1, B, 32, D, H, W)
    w = seeded(2, 64, 32, 3, 3, 3, scale=0.1).requires_grad_(True)
    ref = F.conv3d(x.double(), w.double(), None, stride=stride, padding=1)
    cot = seeded(4, *ref.shape)
    (gref,) = torch.autograd.grad(ref, [w], cot.double())
    got = {}
    for exact in (False, True):
        old = cv.set_option("conv_fp32", exact)
        try:
            wg = w.detach().cuda().requires_grad_(True)
            y = cv.conv3d(x.cuda(), wg, None, stride, False)
            (got[exact],) = torch.autograd.grad(y, [wg], cot.cuda())
        finally:
            cv.set_option("conv_fp32", old)
    tol = 1e-3 * max(1.0, gref.abs().max().item())
    assert maxerr(got[False], gref.float()) <= tol and maxerr(got[True], gref.float()) <= tol
