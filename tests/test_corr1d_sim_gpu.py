"""GPU: the cosine similarity of Corr1d and the tiled data gradient against the float64 restatement
(tests/corr1d_sim_oracle.py, pinned to the reference by tests/golden/golden_corr_sim.npz).  The rows are
``tests.test_corr1d_sim.SIM_CASES``; each test first asks the plan queries about the REAL device pointers, so the
kernels that run are the ones the row names.

Tolerances.
* Forward, absolute: ``(C + 16 + k^2) * 2^-23``, a priori: |out| <= 1; after Cauchy-Schwarz the fp32 dot product
  contributes gamma_C, each squared norm gamma_C / 2 on its inverse root, plus a few ulps for the root, the
  division and the products, and k^2 additions of the box filter.
* Gradients: measured against the REFERENCE, not the kernel: the restatement runs in float32 on the CPU on the
  same inputs; its largest deviation from float64, divided by the largest float64 gradient entry, times 8 is
  the bound (kernel and float32 CPU path sum in different orders inside the same a-priori bound).  Measured
  float32-CPU deviations over the rows (torch 2.10, x86-64): 0.9e-7 .. 3.8e-7 of the largest entry (dL),
  1.1e-7 .. 3.5e-7 (dR); the degenerate case 5.9e-8 / 7.0e-8 / 1.1e-7 on the three clamped pixels and 1.5e-7 / 1.6e-7
  on the rest; the figure depends on the CPU and its thread count (on the MI355X host 1.1e-7 .. 3.7e-7), which is
  why it is measured in the run and not written down as a constant.  The kernels measured 1.2e-7 .. 3.8e-7 (dL)
  and 0.8e-7 .. 4.8e-7 (dR) there, 0.4 .. 1.8 x the float32-CPU figure of the same row, and 0.3 .. 1.05 x on the
  clamped pixels (profiles/corr1d_sim.md has the table)."""
import ctypes

import pytest
import torch
import torch.nn as nn

from oracle import ops as OO
from dsmnet_amd import _lib
from tests import corr1d_sim_oracle as CS
from tests import test_corr1d_sim as S
from tests.helpers import maxerr, seeded
from tests.test_dispatch_gpu import _offset_view

pytestmark = pytest.mark.gpu
EPS = 1e-8


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


_REFS = {}


def reference(case):
    """Inputs, cotangent, the float64 restatement and the float32-CPU deviation of a row: computed once, shared,
    never written to."""
    key = S.case_id(case)
    if key not in _REFS:
        fL, fR = seeded(7, *case.shape), seeded(8, *case.shape)
        B, C, H, W = case.shape
        cot = seeded(9, B, case.D, H, W)
        out, gL, gR = CS.with_grads(fL.double(), fR.double(), cot.double(), case.D, case.s, case.k, EPS)
        _, hL, hR = CS.with_grads(fL, fR, cot, case.D, case.s, case.k, EPS)
        dev = ((hL.double() - gL).abs().max().item() / gL.abs().max().item(),
               (hR.double() - gR).abs().max().item() / gR.abs().max().item())
        _REFS[key] = (fL, fR, cot, out, gL, gR, dev)
    return _REFS[key]


def fwd_tol(C, k):
    return (C + 16 + k * k) * 2.0 ** -23


def device_inputs(case, fL, fR):
    gl = (_offset_view(fL) if case.offset else fL.cuda()).requires_grad_(True)
    gr = (_offset_view(fR) if case.offset else fR.cuda()).requires_grad_(True)
    return gl, gr


def check_plans(cv, case, sim, gl, gr, cot):
    """The plan queries on the real pointers (out, raw, inv, dfL, dfR and the workspace are fresh allocations of
    the wrapper: the caching allocator hands out 512-byte multiples)."""
    B, C, H, W = case.shape
    sc = torch.empty(4, device="cuda")
    cos = sim == "cosine"
    fwd = cv.corr1d_sim_fwd_plan_name(gl, gr, sc, sc if case.k > 1 else None, sc if cos else None, B, C, H, W,
                                      case.D, case.s, case.k, sim)
    bwd = cv.corr1d_sim_bwd_plan_name(cot, gl, gr, sc if cos else None, sc if cos else None, sc, sc,
                                      sc if (case.k > 1 or cos) else None, B, C, H, W, case.D, case.s, case.k, sim)
    assert (fwd, bwd) == S.expected(case, sim)


@pytest.mark.parametrize("case", S.SIM_CASES, ids=S.case_id)
def test_cosine_row_vs_float64_restatement(cv, case):
    fL, fR, cot, ref, rL, rR, dev = reference(case)
    gl, gr = device_inputs(case, fL, fR)
    gcot = cot.cuda()
    check_plans(cv, case, "cosine", gl, gr, gcot)
    out = cv.corr1d(gl, gr, case.D, case.s, case.k, sim="cosine", eps=EPS)
    gL, gR = torch.autograd.grad(out, (gl, gr), gcot)
    e_out = maxerr(out, ref)
    e_L, e_R = maxerr(gL, rL) / rL.abs().max().item(), maxerr(gR, rR) / rR.abs().max().item()
    print("cosine %s / %s: out %.3e (tol %.3e)  dL %.3e (float32 CPU %.3e)  dR %.3e (float32 CPU %.3e)"
          % (S.expected(case, "cosine") + (e_out, fwd_tol(case.shape[1], case.k), e_L, dev[0], e_R, dev[1])))
    assert torch.isfinite(out).all() and torch.isfinite(gL).all() and torch.isfinite(gR).all()
    assert e_out <= fwd_tol(case.shape[1], case.k)
    assert e_L <= 8 * dev[0] and e_R <= 8 * dev[1]


def test_cosine_degenerate_vectors(cv):
    """Two zero feature vectors and one shorter than eps (the golden's degenerate case, (k, s, D) = (1, 1, 9)):
    finite everywhere, the forward at the a-priori tolerance, and the gradients in two groups so that the 1e8
    entries of the clamped pixels do not hide the rest: every clamped pixel relative to its own largest entry,
    all other pixels relative to their own maximum.  Bounds as in the row test: 8 x the float32-CPU deviation of
    the same group."""
    fL, fR = CS.make_degenerate(seeded(41, 2, 16, 3, 24), seeded(42, 2, 16, 3, 24))
    cot = seeded(43, 2, 9, 3, 24)
    ref, rL, rR = CS.with_grads(fL.double(), fR.double(), cot.double(), 9, 1, 1, EPS)
    _, hL, hR = CS.with_grads(fL, fR, cot, 9, 1, 1, EPS)
    gl, gr = fL.cuda().requires_grad_(True), fR.cuda().requires_grad_(True)
    out = cv.corr1d(gl, gr, 9, 1, 1, sim="cosine", eps=EPS)
    gL, gR = torch.autograd.grad(out, (gl, gr), cot.cuda())
    assert torch.isfinite(out).all() and torch.isfinite(gL).all() and torch.isfinite(gR).all()
    assert maxerr(out, ref) <= fwd_tol(16, 1)
    assert out[0, :, 0, 3].abs().max().item() == 0.0 and out[0, 0, 1, 5].item() == 0.0
    assert rL.abs().max().item() > 1e7
    got = {"L": gL.double().cpu(), "R": gR.double().cpu()}
    want, f32 = {"L": rL, "R": rR}, {"L": hL.double(), "R": hR.double()}
    rest = {k: torch.ones(2, 3, 24, dtype=torch.bool) for k in "LR"}
    for side, b, y, x in CS.DEGENERATE_PIXELS:
        w = want[side][b, :, y, x]
        scale = w.abs().max().item()
        err = (got[side][b, :, y, x] - w).abs().max().item() / scale
        dev = (f32[side][b, :, y, x] - w).abs().max().item() / scale
        print("clamped pixel %s(%d,%d,%d): scale %.3e err %.3e float32 CPU %.3e" % (side, b, y, x, scale, err, dev))
        assert scale > 1e6 and err <= 8 * dev
        rest[side][b, y, x] = False
    for side in "LR":
        m = rest[side][:, None].expand(2, 16, 3, 24)
        scale = want[side][m].abs().max().item()
        err = (got[side][m] - want[side][m]).abs().max().item() / scale
        dev = (f32[side][m] - want[side][m]).abs().max().item() / scale
        print("other pixels d%s: scale %.3e err %.3e float32 CPU %.3e" % (side, scale, err, dev))
        assert err <= 8 * dev


@pytest.mark.parametrize("case", S.SIM_CASES, ids=S.case_id)
def test_dot_through_the_sim_entry_is_bit_identical(cv, hip_lib, case):
    """The templated kernels' DSM_SIM_DOT instantiations are the kernels of ``dsm_corr1d_fwd``."""
    fL, fR = reference(case)[:2]
    gl, gr = device_inputs(case, fL, fR)
    B, C, H, W = case.shape
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    outs = []
    for entry in ("old", "sim"):
        out = torch.full((B, case.D, H, W), float("nan"), device="cuda")
        tmp = torch.full_like(out, float("nan")) if case.k > 1 else None
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if entry == "old":
            rc = hip_lib.dsm_corr1d_fwd(p(gl), p(gr), p(out), p(tmp), B, C, H, W, case.D, case.s, case.k, 0, st)
        else:
            assert cv.corr1d_sim_fwd_plan_name(gl, gr, out, tmp, None, B, C, H, W, case.D, case.s, case.k, "dot") == case.fwd
            rc = hip_lib.dsm_corr1d_sim_fwd(p(gl), p(gr), p(out), p(tmp), None, B, C, H, W, case.D, case.s, case.k,
                                            _lib.DSM_SIM_DOT, 0.0, 0, st)
        assert rc == 0
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("case", [c for c in S.SIM_CASES if "bwd_tile" in c.bwd], ids=S.case_id)
def test_tiled_dot_backward_vs_float64_oracle(cv, case):
    """``corr1d_tiled_bwd`` on: the dot-product gradients of every eligible row at the bound of
    test_corr1d_branch_vs_float64_oracle (3e-4 absolute, same seeds), twice with the same bits."""
    fL, fR, cot = reference(case)[:3]
    dL, dR = fL.double().requires_grad_(True), fR.double().requires_grad_(True)
    rL, rR = torch.autograd.grad(OO.corr1d(dL, dR, case.D, case.s, case.k), (dL, dR), cot.double())
    gl, gr = device_inputs(case, fL, fR)
    gcot = cot.cuda()
    check_plans(cv, case, "dot", gl, gr, gcot)
    old = cv.set_option("corr1d_tiled_bwd", True)
    try:
        runs = []
        for _ in range(2):
            out = cv.corr1d(gl, gr, case.D, case.s, case.k)
            runs.append(torch.autograd.grad(out, (gl, gr), gcot))
    finally:
        cv.set_option("corr1d_tiled_bwd", old)
    errs = maxerr(runs[0][0], rL), maxerr(runs[0][1], rR)
    print("tiled dot backward %s: dL %.3e dR %.3e" % ((case.bwd,) + errs))
    assert errs[0] <= 3e-4 and errs[1] <= 3e-4
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_cosine_forward_and_backward_replay_from_a_graph(cv):
    case = S.SIM_CASES[9]                      # (2,64,3,160) D 81 s 2 k 3: every launch of the op
    assert (case.k, case.s, case.bwd) == (3, 2, "box3+bwd_tile<2>")
    fL, fR, cot = reference(case)[:3]
    gl, gr, gcot = fL.cuda().requires_grad_(True), fR.cuda().requires_grad_(True), cot.cuda()

    def step():
        out = cv.corr1d(gl, gr, case.D, case.s, case.k, sim="cosine", eps=EPS)
        return (out,) + torch.autograd.grad(out, (gl, gr), gcot)
    eager = [t.detach().clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for o in outs:
            o.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            assert torch.equal(o.detach(), e)


def test_module_path_equals_the_op(cv):
    from dsmnet_amd.models.util_conv import Corr1d
    fL, fR = seeded(7, 2, 64, 3, 160).cuda(), seeded(8, 2, 64, 3, 160).cuda()
    cot = seeded(9, 2, 41, 3, 160).cuda()
    res = []
    for fn in (Corr1d(3, 2, 41, simfun=nn.CosineSimilarity(dim=1)).cuda(),
               lambda a, b: cv.corr1d(a, b, 41, 2, 3, sim="cosine", eps=1e-8)):
        l, r = fL.clone().requires_grad_(True), fR.clone().requires_grad_(True)
        out = fn(l, r)
        res.append((out.detach(),) + torch.autograd.grad(out, (l, r), cot))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    ref = CS.corr1d_cosine(fL.double().cpu(), fR.double().cpu(), 41, 2, 3, 1e-8)
    assert maxerr(res[0][0], ref) <= fwd_tol(64, 3)
