"""GPU: ``dsm_warp_abs_error_bwd`` / ``WarpAbsErrorFunction`` (csrc/warp.hip) against float64 CPU autograd
through the oracle's ``imwarp`` (utils/imwrap.py:37-72) and ``abs`` (models/iresnet.py:169-170).

The gradients of bilinear sampling and of ``abs`` jump where the sample position is an integer or ``L == v``;
the inputs are constructed to stay clear of both (sample position ``k + f`` with ``f`` in [0.1, 0.9],
``|L - v| >= 0.1``), so no element is left out of any comparison.  The bound is not a fixed number: the stock
fp32 GPU path (``models.iresnet.imwrap_BCHW`` + ``abs`` under autograd) runs on the same inputs, its worst error
against float64 relative to the reference tensor's maximum is measured, and the new path gets 4x that with a
floor of 2e-6 (an fp32 sum of a handful of terms taken in another order).  Both figures are printed."""
import functools

import pytest
import torch

from oracle import models as OM
from tests.helpers import seeded

pytestmark = pytest.mark.gpu

SEED = 11
FLOOR = 2e-6
# (B, C, H, W), source (H0, W0) or None for the map's own size
SHAPES = [((2, 5, 9, 33), None), ((1, 32, 6, 70), None), ((1, 4, 20, 31), (24, 40)), ((1, 8, 2, 2), None),
          ((1, 9, 3, 300), None)]


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


def _delt(seed):
    torch.manual_seed(seed)
    return float(1e-4 * (torch.rand(1)[0] + 0.1))          # the draw imwrap_BCHW makes (:70)


def _disp_for(ix_t, W, W0):
    """The disparity that puts pixel x's sample at ``ix_t``: ix = (x - disp) * W0 / (W0 - 1) - 0.5."""
    x = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    return (x - (ix_t + 0.5) * (W0 - 1) / W0).float()


@functools.lru_cache(maxsize=None)
def case(idx, rowwise=False):
    """fp32 inputs (L, R, disp, g) and the float64 reference (gL, gR, gdisp, gR of the plain warp, gdisp of the
    plain warp, sign).  ``rowwise``: one sample position per row (every pixel of a row scatters into the same two
    columns)."""
    (B, C, H, W), src = SHAPES[idx] if idx >= 0 else (((1, 8, 4, 300), None))
    H0, W0 = src or (H, W)
    gen = torch.Generator().manual_seed(100 + idx)
    kshape = (B, 1, H, 1) if rowwise else (B, 1, H, W)
    k = torch.randint(-3, W0 + 2, kshape, generator=gen).double()
    f = 0.1 + 0.8 * torch.rand(kshape, generator=gen, dtype=torch.float64)
    disp = _disp_for((k + f).expand(B, 1, H, W), W, W0)
    R = seeded(200 + idx, B, C, H0, W0)
    g = seeded(300 + idx, B, C, H, W)
    torch.manual_seed(SEED)
    with torch.no_grad():
        v = OM.imwarp(R.double(), disp.double())
    sgn = torch.where(torch.rand(v.shape, generator=gen) < 0.5, -1.0, 1.0).double()
    L = (v + sgn * (0.1 + torch.rand(v.shape, generator=gen, dtype=torch.float64))).float()
    Ld, Rd, dd = (t.double().requires_grad_(True) for t in (L, R, disp))
    torch.manual_seed(SEED)
    ref = torch.autograd.grad((Ld - OM.imwarp(Rd, dd)).abs(), [Ld, Rd, dd], g.double())
    torch.manual_seed(SEED)
    ref_plain = torch.autograd.grad(OM.imwarp(Rd, dd), [Rd, dd], g.double())
    sign = torch.sign(L.double() - v)
    assert (L.double() - v).abs().min().item() >= 0.09
    return (L, R, disp, g), ref + ref_plain + (sign,)


def rel(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def stock(L, R, disp, g, plain=False):
    """The training path of the parent commit on the GPU in fp32."""
    from dsmnet_amd.models.iresnet import imwrap_BCHW
    Lc, Rc, dc = (t.cuda().requires_grad_(True) for t in (L, R, disp))
    torch.manual_seed(SEED)
    v = imwrap_BCHW(Rc, dc)
    if plain:
        return torch.autograd.grad(v, [Rc, dc], g.cuda())
    return torch.autograd.grad(torch.abs(Lc - v), [Lc, Rc, dc], g.cuda())


def new(cv, L, R, disp, g, needs=(True, True, True)):
    ins = [None if t is None else t.cuda().requires_grad_(n) for t, n in zip((L, R, disp), needs)]
    out = cv.warp_abs_error(ins[0], ins[1], ins[2], _delt(SEED))
    want = [t for t in ins if t is not None and t.requires_grad]
    grads = iter(torch.autograd.grad(out, want, g.cuda()))
    return out, [next(grads) if (t is not None and t.requires_grad) else None for t in ins]


def check(tag, got, stk, ref):
    """Bound = max(4 x the stock fp32 path's measured error, FLOOR), both relative to max |ref|."""
    e_stock, e_new = rel(stk, ref), rel(got, ref)
    print("%s: stock fp32 vs fp64 %.3e, new vs fp64 %.3e (of max |ref| = %.3e)"
          % (tag, e_stock, e_new, ref.abs().max().item()))
    assert e_new <= max(4 * e_stock, FLOOR), (tag, e_new, e_stock)


@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_gradients_match_float64_autograd(cv, idx):
    (L, R, disp, g), (rL, rR, rd, rR_plain, rd_plain, sign) = case(idx)
    sL, sR, sd = stock(L, R, disp, g)
    _, (gL, gR, gd) = new(cv, L, R, disp, g)
    assert torch.equal(gL.cpu(), (g.double() * sign).float())
    assert rel(gL, rL) == 0.0
    check("shape %s gR" % (SHAPES[idx],), gR, sR, rR)
    check("shape %s gdisp" % (SHAPES[idx],), gd, sd, rd)
    # the disparity gradient is exercised (on the 2 x 2 map most of k in [-3, 4) is out of bounds)
    assert (rd != 0).double().mean().item() > (0.5 if disp.shape[3] > 2 else 0.0)
    # the plain warp (L = None)
    pR, pd = stock(L, R, disp, g, plain=True)
    _, (_, gR, gd) = new(cv, None, R, disp, g)
    check("shape %s plain gR" % (SHAPES[idx],), gR, pR, rR_plain)
    check("shape %s plain gdisp" % (SHAPES[idx],), gd, pd, rd_plain)
    # one gradient at a time: the NULL-pointer paths; the written ones do not depend on what else is asked for
    _, (a, b, only_d) = new(cv, L, R, disp, g, needs=(False, False, True))
    assert a is None and b is None
    check("shape %s gdisp alone" % (SHAPES[idx],), only_d, sd, rd)
    _, (a, only_R, c) = new(cv, L, R, disp, g, needs=(False, True, False))
    assert a is None and c is None
    check("shape %s gR alone" % (SHAPES[idx],), only_R, sR, rR)


def test_a_whole_row_scatters_into_two_columns(cv):
    (L, R, disp, g), (rL, rR, rd, _, _, sign) = case(-1, rowwise=True)
    sL, sR, sd = stock(L, R, disp, g)
    _, (gL, gR, gd) = new(cv, L, R, disp, g)
    assert torch.equal(gL.cpu(), (g.double() * sign).float())
    check("contention gR", gR, sR, rR)
    check("contention gdisp", gd, sd, rd)


def test_wild_disparities_give_finite_gradients_and_exact_zeros(cv):
    """|d| up to ~100 px on a 20-px-wide map: most pixels have every tap out of bounds."""
    shape = (1, 3, 16, 20)
    L, R, g = seeded(1, *shape), seeded(2, *shape), seeded(4, *shape)
    disp = seeded(3, 1, 1, 16, 20) * 40
    out, (gL, gR, gd) = new(cv, L, R, disp, g)
    for t in (gL, gR, gd):
        assert bool(torch.isfinite(t).all())
    outside = (out.detach().cpu() == L.abs()).all(dim=1, keepdim=True)        # v == 0 in every channel
    assert 0.5 < outside.double().mean().item() < 1.0
    assert bool((gd.cpu()[outside] == 0).all())
    assert torch.equal(gL.cpu()[outside.expand(shape)], (g * torch.sign(L))[outside.expand(shape)])
    # with every pixel out of bounds nothing reaches R either
    far = torch.full((1, 1, 16, 20), 1000.0)
    _, (_, gR, gd) = new(cv, L, R, far, g)
    assert bool((gR == 0).all()) and bool((gd == 0).all())


def test_train_forward_is_the_eval_forward(cv):
    (L, R, disp, g), _ = case(0)
    out, _ = new(cv, L, R, disp, g)
    assert out.requires_grad
    with torch.no_grad():
        want = cv.warp_abs_error(L.cuda(), R.cuda(), disp.cuda(), _delt(SEED))
    assert torch.equal(out.detach(), want)


def test_gR_does_not_accumulate_eagerly_or_in_a_replayed_graph(cv):
    (L, R, disp, g), (rL, rR, rd, _, _, sign) = case(0)
    sL, sR, sd = stock(L, R, disp, g)
    _, first = new(cv, L, R, disp, g)
    _, second = new(cv, L, R, disp, g)                       # a fresh graph: nothing carried over
    check("second backward gR", second[1], sR, rR)
    assert torch.equal(first[0], second[0]) and torch.equal(first[2], second[2])
    ins = [t.cuda().requires_grad_(True) for t in (L, R, disp)]
    gc, delt = g.cuda(), _delt(SEED)

    def step():
        out = cv.warp_abs_error(ins[0], ins[1], ins[2], delt)
        return torch.autograd.grad(out, ins, gc)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seen.append([o.clone() for o in outs])
    check("second replay gR", seen[1][1], sR, rR)           # not twice the gradient
    assert rel(seen[1][1], first[1].double().cpu()) <= max(4 * rel(sR, rR), FLOOR)
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][2], seen[1][2])
    assert torch.equal(seen[1][0], first[0]) and torch.equal(seen[1][2], first[2])


def test_argument_checks_under_autograd(cv):
    R = torch.zeros(1, 4, 8, 8, device="cuda", requires_grad=True)
    with pytest.raises(ValueError):
        cv.warp_abs_error(None, R, torch.zeros(1, 2, 8, 8, device="cuda", requires_grad=True), 1e-5)
    with pytest.raises(ValueError):
        cv.warp_abs_error(torch.zeros(1, 3, 8, 8, device="cuda", requires_grad=True), R,
                          torch.zeros(1, 1, 8, 8, device="cuda"), 1e-5)
    with pytest.raises(RuntimeError):
        cv.warp_abs_error(None, torch.zeros(1, 4, 8, 8, requires_grad=True), torch.zeros(1, 1, 8, 8), 1e-5)
