"""GPU parity of every dispatch branch of corr1d, soft-argmin, the concatenation volume / relayout
and the fused train-mode BN against the float64 oracle (``oracle.ops`` is dtype-generic; BN: float64
torch as in tests/test_bn3d_gpu.py).  The cases are the tables of tests/test_dispatch_plans.py, which
pins on the CPU the branch each row takes; here each row first asks the plan query about the REAL
device pointers, so the kernel that runs is the one the row is named after.

Inputs are float32-representable draws handed to the oracle as float64; cotangents likewise.  Every
comparison is a maximum over the whole tensor.  Tolerances are the suite's existing ones
(test_corr1d_vs_oracle, test_softargmin_vs_oracle, test_volume_vs_oracle, test_bn_add_relu3d_vs_torch)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ops as OO
from dsmnet_amd import _lib
from tests.helpers import maxerr, seeded
from tests import test_dispatch_plans as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


def _ids(fmt):
    return lambda c: fmt(c)


def _offset_view(t):
    """``t`` on the device as a contiguous view one float into a larger buffer: 16-byte misaligned."""
    buf = torch.empty(t.numel() + 5, device="cuda", dtype=torch.float32)
    start = 1 + ((16 - buf.data_ptr() % 16) % 16) // 4          # buffer base aligned or not: land on +4 bytes
    v = buf[start:start + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ------------------------------------------------------------------------------------ corr1d --
@pytest.mark.parametrize("case", T.CORR_CASES,
                         ids=_ids(lambda c: "%s-D%d-s%d-k%d-%s" % ("x".join(map(str, c.shape)), c.D, c.s, c.k, c.plan)))
def test_corr1d_branch_vs_float64_oracle(cv, case):
    fL, fR = seeded(7, *case.shape), seeded(8, *case.shape)
    dL, dR = fL.double().requires_grad_(True), fR.double().requires_grad_(True)
    ref = OO.corr1d(dL, dR, case.D, case.s, case.k)
    cot = seeded(9, *ref.shape)
    rL, rR = torch.autograd.grad(ref, (dL, dR), cot.double())
    gl = (_offset_view(fL) if case.offset else fL.cuda()).requires_grad_(True)
    gr = (_offset_view(fR) if case.offset else fR.cuda()).requires_grad_(True)
    B, C, H, W = case.shape
    # out and tmp are fresh allocations of the wrapper (the caching allocator hands out 512-byte multiples)
    scratch = torch.empty(4, device="cuda")
    assert cv.corr1d_plan_name(gl, gr, scratch, scratch if case.k > 1 else None, B, C, H, W, case.D, case.s,
                               case.k) == case.plan
    out = cv.corr1d(gl, gr, case.D, case.s, case.k)
    gL, gR = torch.autograd.grad(out, (gl, gr), cot.cuda())
    errs = maxerr(out, ref), maxerr(gL, rL), maxerr(gR, rR)
    print("corr1d %s: out %.3e dL %.3e dR %.3e" % ((case.plan,) + errs))
    # 3e-4 absolute (test_corr1d_vs_oracle).  |out| <= 44, |g| <= 47 at these shapes and seeds; the float32
    # oracle on the CPU is within 5.8e-6 (forward) and 1.6e-5 (gradients) of the float64 one: about 20x margin
    # over fp32 re-association
    assert errs[0] <= 3e-4
    assert errs[1] <= 3e-4 and errs[2] <= 3e-4


# ------------------------------------------------------------------------------- soft-argmin --
@pytest.mark.parametrize("case", T.SA_CASES,
                         ids=_ids(lambda c: "%s-to-%s-%s" % ("x".join(map(str, c.cshape)), "x".join(map(str, c.osize or ("same",))), c.fwd)))
def test_soft_argmin_branch_vs_float64_oracle(cv, case):
    c = seeded(31, *case.cshape, scale=2.0)
    dc = c.double().requires_grad_(True)
    ref = OO.soft_argmin(dc, case.osize, case.negate, case.align)
    cot = seeded(32, *ref.shape)
    (rg,) = torch.autograd.grad(ref, dc, cot.double())
    g = c.cuda().requires_grad_(True)
    dims = T.sa_dims(case)
    assert cv.soft_argmin_fwd_plan_name(g, g, g, *dims, negate=case.negate, align_corners=case.align) == case.fwd
    assert cv.soft_argmin_bwd_plan_name(g, g, g, g, g, *dims, negate=case.negate, align_corners=case.align) == case.bwd
    out = cv.soft_argmin(g, case.osize, case.negate, case.align)
    (gg,) = torch.autograd.grad(out, g, cot.cuda())
    assert out.shape == ref.shape and gg.shape == rg.shape
    e_out, e_g, gmax = maxerr(out, ref), maxerr(gg, rg), rg.abs().max().item()
    print("soft_argmin %s / %s: disp %.3e dcost %.3e (|g|max %.3e)" % (case.fwd, case.bwd, e_out, e_g, gmax))
    # 1e-3 px and 1e-3 max(1, |g|max) (test_softargmin_vs_oracle).  Measured on the CPU, the float32 oracle is
    # within 4.1e-5 px / 4.6e-5 of the float64 one over these rows (the largest at D = 97); at the down-sampling
    # fallback row (8x40x200 -> 8x5x25, |g|max = 0.64) it is within 7.5e-7 px / 6.2e-8: the existing bound
    # keeps more than 20x margin everywhere, nothing wider is needed.
    assert e_out <= 1e-3
    assert e_g <= 1e-3 * max(1.0, gmax)


def test_soft_argmin_timer_label_follows_the_plan(cv):
    """The launch label the timer records is the kernel the host code picks: D x4 with H, W unchanged is
    the x4 head, and D == 4 Dc with Dc < 4 is not."""
    timer = cv.LaunchTimer()
    cv.set_timer(timer)
    try:
        cv.soft_argmin(seeded(1, 1, 1, 6, 5, 9).cuda(), (24, 5, 9))
        cv.soft_argmin(seeded(1, 1, 1, 3, 5, 9).cuda(), (12, 10, 18))
        cv.soft_argmin(seeded(1, 1, 1, 6, 5, 9).cuda(), (24, 10, 18), align_corners=True)
    finally:
        cv.set_timer(None)
    torch.cuda.synchronize()
    assert [r[0] for r in timer.records] == ["soft_argmin_up4_kernel", "soft_argmin_fwd_kernel", "soft_argmin_fwd_kernel"]


# ------------------------------------------------------------------------------ concat volume --
@pytest.mark.parametrize("case", T.VOL_CASES,
                         ids=_ids(lambda c: "%s-D%d-%s-%s" % ("x".join(map(str, c.shape)), c.D, "ndhwc" if c.channels_last else "ncdhw", c.mode)))
def test_volume_branch_vs_float64_oracle(cv, case):
    fL, fR = seeded(11, *case.shape), seeded(12, *case.shape)
    B, C, H, W = case.shape
    if case.fwd is None:                                       # refused by the host code: a clean error, no launch
        torch.cuda.synchronize()
        with pytest.raises(_lib.DsmnetHipError, match=r"dsm_concat_volume_fwd failed: .*\(code %d\)" % case.error):
            cv.concat_volume(fL.cuda(), fR.cuda(), case.D, bool(case.mode), case.channels_last)
        torch.cuda.synchronize()                               # and nothing faulted behind it
        return
    if case.mode == "right":
        got = cv.concat_volume_right(fL.cuda(), fR.cuda(), case.D)
        assert got.is_contiguous(memory_format=torch.channels_last_3d)
        assert torch.equal(got.cpu().double(), OO.concat_volume_right(fL.double(), fR.double(), case.D))
        return
    dL, dR = fL.double().requires_grad_(True), fR.double().requires_grad_(True)
    ref = OO.concat_volume(dL, dR, case.D, case.mode)
    cot = seeded(13, *ref.shape)
    rL, rR = torch.autograd.grad(ref, (dL, dR), cot.double())
    gl, gr = fL.cuda().requires_grad_(True), fR.cuda().requires_grad_(True)
    vol = cv.concat_volume(gl, gr, case.D, case.mode, case.channels_last)
    fmt = torch.channels_last_3d if case.channels_last else torch.contiguous_format
    assert vol.is_contiguous(memory_format=fmt)
    assert cv.concat_volume_plan_name(gl, gr, vol, B, C, H, W, case.D, case.mode, case.channels_last) == case.fwd
    assert torch.equal(vol.detach().cpu().double(), ref.detach())          # data movement: bit-exact
    gL, gR = torch.autograd.grad(vol, (gl, gr), cot.cuda())
    print("volume %s: dL %.3e dR %.3e" % (case.fwd, maxerr(gL, rL), maxerr(gR, rR)))
    assert maxerr(gL, rL) <= 1e-4 and maxerr(gR, rR) <= 1e-4


def test_relayout_second_channel_block_ragged(cv):
    """(B, C, S) <-> (B, S, C) with C = 80 (a second, partial 64-channel block), S = 105 (a partial
    64-voxel block) and B = 2, against ``permute`` on the raw memory: bit-exact both ways."""
    x = seeded(3, 2, 80, 3, 5, 7).cuda()
    cl = cv.to_channels_last_3d(x)
    assert cl.is_contiguous(memory_format=torch.channels_last_3d) and cl.shape == x.shape
    raw = torch.as_strided(cl, (2, 3, 5, 7, 80), (105 * 80, 35 * 80, 7 * 80, 80, 1))
    assert torch.equal(raw, x.permute(0, 2, 3, 4, 1))
    back = cv.to_contiguous_3d(cl)
    assert back.is_contiguous() and back.data_ptr() != cl.data_ptr() and torch.equal(back, x)


# ------------------------------------------------------------------------- fused train-mode BN --
def _bn_reference(y, gamma, beta, res, rm, rv, relu, momentum, eps):
    out = F.batch_norm(y, rm, rv, gamma, beta, True, momentum, eps)
    if relu == 2:
        out = out.relu()
    if res is not None:
        d, h, w = (min(a, b) for a, b in zip(out.shape[2:], res.shape[2:]))
        out = out[:, :, :d, :h, :w] + res[:, :, :d, :h, :w]
    if relu == 1:
        out = out.relu()
    return out


def _bn_parity(cv, case):
    C, (B, Dy, Hy, Wy), rshape, relu = case
    y = (seeded(1, B, C, Dy, Hy, Wy) * 1.7 + 0.3).double().requires_grad_(True)
    gamma = (seeded(2, C).abs() + 0.5).double().requires_grad_(True)
    beta = seeded(3, C).double().requires_grad_(True)
    res = seeded(4, B, C, *rshape).double().requires_grad_(True) if rshape else None
    rm, rv = seeded(5, C).double(), seeded(6, C).abs().double() + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    want = _bn_reference(y, gamma, beta, res, rm, rv, relu, 0.1, 1e-5)
    cot = seeded(7, *want.shape).double()
    grads = torch.autograd.grad(want, [t for t in (y, gamma, beta, res) if t is not None], cot)

    yg = y.detach().float().cuda().requires_grad_(True)
    gg, bg = gamma.detach().float().cuda().requires_grad_(True), beta.detach().float().cuda().requires_grad_(True)
    rg = res.detach().float().cuda().requires_grad_(True) if res is not None else None
    rmg, rvg = rm0.float().cuda(), rv0.float().cuda()
    out = cv.bn_add_relu3d(yg, gg, bg, rg, rmg, rvg, relu, 0.1, 1e-5)
    assert tuple(out.shape) == tuple(want.shape)
    e = maxerr(out, want)
    print("bn C=%d %s: out %.3e (|out|max %.3e) rm %.3e rv %.3e" % (C, (B, Dy, Hy, Wy), e, want.abs().max().item(),
                                                                     maxerr(rmg, rm), maxerr(rvg, rv)))
    assert e <= 2e-5 * max(1.0, want.abs().max().item())
    assert maxerr(rmg, rm) <= 1e-5 and maxerr(rvg, rv) <= 1e-5
    got = torch.autograd.grad(out, [t for t in (yg, gg, bg, rg) if t is not None], cot.float().cuda())
    for name, g, r in zip(("dy", "dgamma", "dbeta", "dres"), got, grads):
        assert g.shape == r.shape, name
        tol = 5e-5 * max(1.0, r.abs().max().item())
        print("   %s %.3e (bound %.3e)" % (name, maxerr(g, r), tol))
        assert maxerr(g, r) <= tol, "%s: %.3e > %.3e" % (name, maxerr(g, r), tol)
    return out


@pytest.mark.parametrize("case", T.BN_CASES, ids=_ids(lambda c: "C%d-%s" % (c.C, "x".join(map(str, c.yshape)))))
def test_bn_grid_strides_and_widths_vs_float64_torch(cv, case):
    _bn_parity(cv, case)


def test_bn_apply_grid_cap_under_amax_scope(cv):
    """f16x2 inside ``amax_scope``: the apply and backward-apply launches get an absolute-maximum slot and
    1105920 quads, so their grids are capped at 4096 blocks and every thread walks a second element;
    the slot must hold exactly max |out|."""
    old = cv.set_option("conv_precision", "f16x2")
    try:
        with cv.amax_scope(torch.device("cuda", torch.cuda.current_device())):
            out = _bn_parity(cv, T.BN_CAP_CASE)
            assert cv.needs_amax() and out._dsm_amax.numel() == 1
            assert out._dsm_amax.item() == out.detach().abs().max().item()
    finally:
        cv.set_option("conv_precision", old)
