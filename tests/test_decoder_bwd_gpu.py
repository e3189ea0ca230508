"""GPU: ``dsm_decoder_cat_bwd`` / ``DecoderCatFunction`` (csrc/decoder.hip) against float64 CPU autograd through
the stock ops of one decoder level (bias add, ReLU, bilinear x2 upsampling, the three crops, ``cat``:
models/dispnetcorr.py:89-132, util_fun.py:7-15).

ReLU's gradient jumps at ``up + bias == 0``: the inputs keep ``|up + bias| >= 0.05`` and no element is left out
of any comparison.  ``g_up`` and ``g_skip`` are masks and copies: they must equal the stock fp32 GPU result
exactly.  ``g_pr`` and ``g_bias`` are sums: the stock fp32 GPU ops run on the same inputs, their worst error
against float64 relative to the reference tensor's maximum is measured, and the new path gets 4x that with a floor
of 2e-6 (an fp32 sum of a handful of terms taken in another order).  Both figures are printed."""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.helpers import seeded

pytestmark = pytest.mark.gpu

FLOOR = 2e-6
# (B, Cu, Cp, Cs), (Hu, Wu), (Hp, Wp), (Hs, Ws)
SHAPES = [((2, 3, 1, 2), (6, 10), (3, 5), (5, 9)),        # crops to 5 x 9, odd sizes, w no multiple of 4
          ((1, 2, 1, 1), (2, 4), (1, 2), (2, 4)),         # Hp = 1: both clamps of the upsampling at once
          ((1, 4, 0, 3), (4, 8), None, (4, 8)),           # no pr
          ((1, 4, 1, 0), (8, 12), (4, 6), None),          # no skip
          ((1, 2, 1, 1), (40, 120), (20, 60), (40, 119))]  # more than one block per plane: the bias sum crosses blocks


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


def stock_ops(up, bias, pr, skip, relu):
    """What ``decoder_level``'s stock branch does after the transposed convolution's matrix product."""
    a = up if bias is None else up + bias.view(1, -1, 1, 1)
    seq = [F.relu(a) if relu else a]
    if pr is not None:
        seq.append(F.interpolate(pr, scale_factor=2, mode="bilinear", align_corners=False))
    if skip is not None:
        seq.append(skip)
    h = min(t.shape[2] for t in seq)
    w = min(t.shape[3] for t in seq)
    return torch.cat([t[:, :, :h, :w] for t in seq], dim=1)


def grads_of(fn, tensors, g, dtype, device):
    ins = [None if t is None else t.to(device=device, dtype=dtype).requires_grad_(True) for t in tensors]
    out = fn(*ins)
    got = iter(torch.autograd.grad(out, [t for t in ins if t is not None], g.to(device=device, dtype=dtype)))
    return out, [None if t is None else next(got) for t in ins]


@functools.lru_cache(maxsize=None)
def case(idx, with_bias=True):
    (B, Cu, Cp, Cs), (Hu, Wu), ps, ss = SHAPES[idx]
    bias = seeded(10 + idx, Cu) if with_bias else None
    pre = seeded(20 + idx, B, Cu, Hu, Wu).double()
    pre = torch.sign(pre) * (0.05 + pre.abs())
    up = (pre - (bias.double().view(1, -1, 1, 1) if with_bias else 0.0)).float()
    pr = seeded(30 + idx, B, Cp, *ps) if Cp else None
    skip = seeded(40 + idx, B, Cs, *ss) if Cs else None
    h = min([Hu] + ([2 * ps[0]] if Cp else []) + ([ss[0]] if Cs else []))
    w = min([Wu] + ([2 * ps[1]] if Cp else []) + ([ss[1]] if Cs else []))
    g = seeded(50 + idx, B, Cu + Cp + Cs, h, w)
    return (up, bias, pr, skip), g


def rel(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def check(tag, got, stk, ref):
    e_stock, e_new = rel(stk, ref), rel(got, ref)
    print("%s: stock fp32 vs fp64 %.3e, new vs fp64 %.3e (of max |ref| = %.3e)"
          % (tag, e_stock, e_new, ref.abs().max().item()))
    assert e_new <= max(4 * e_stock, FLOOR), (tag, e_new, e_stock)


def run_case(cv, idx, relu, with_bias):
    tensors, g = case(idx, with_bias)
    _, ref = grads_of(lambda *a: stock_ops(*a, relu=relu), tensors, g, torch.float64, "cpu")
    want, stk = grads_of(lambda *a: stock_ops(*a, relu=relu), tensors, g, torch.float32, "cuda")
    out, got = grads_of(lambda *a: cv.DecoderCatFunction.apply(*a, relu), tensors, g, torch.float32, "cuda")
    Cu, Cp = SHAPES[idx][0][1:3]
    assert torch.equal(out[:, :Cu], want[:, :Cu]) and torch.equal(out[:, Cu + Cp:], want[:, Cu + Cp:])
    tag = "shape %d relu %d bias %d" % (idx, relu, with_bias)
    assert got[0].shape == tensors[0].shape and torch.equal(got[0], stk[0]), tag + " g_up"
    if tensors[3] is not None:
        assert got[3].shape == tensors[3].shape and torch.equal(got[3], stk[3]), tag + " g_skip"
    if tensors[2] is not None:
        assert got[2].shape == tensors[2].shape
        check(tag + " g_pr", got[2], stk[2], ref[2])
    if with_bias:
        check(tag + " g_bias", got[1], stk[1], ref[1])


@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_gradients_match_float64_autograd(cv, idx):
    run_case(cv, idx, relu=True, with_bias=True)


@pytest.mark.parametrize("relu,with_bias", [(False, True), (True, False), (False, False)])
def test_bare_deconvolution_and_no_bias(cv, relu, with_bias):
    run_case(cv, 0, relu, with_bias)


def test_single_gradients_and_repeated_backward(cv):
    """Each gradient asked for alone (the NULL-pointer paths) equals what the full call wrote; g_bias, the one
    atomic sum, starts from zero on every call."""
    tensors, g = case(0)
    _, full = grads_of(lambda *a: cv.DecoderCatFunction.apply(*a, True), tensors, g, torch.float32, "cuda")
    _, ref = grads_of(lambda *a: stock_ops(*a, relu=True), tensors, g, torch.float64, "cpu")
    _, stk = grads_of(lambda *a: stock_ops(*a, relu=True), tensors, g, torch.float32, "cuda")
    for k in range(4):
        ins = [t.cuda().requires_grad_(i == k) for i, t in enumerate(tensors)]
        out = cv.DecoderCatFunction.apply(*ins, True)
        for _ in range(2):
            got, = torch.autograd.grad(out, [ins[k]], g.cuda(), retain_graph=True)
            if k == 1:
                check("g_bias alone", got, stk[1], ref[1])
            else:
                assert torch.equal(got, full[k]), k


def _level_case():
    """A level whose pre-activation stays 0.05 clear of zero (seeds are tried in order until one does)."""
    for seed in range(400):
        torch.manual_seed(seed)
        conv = nn.ConvTranspose2d(3, 2, 4, 2, 1, bias=True)
        x = seeded(1000 + seed, 1, 3, 3, 5) * 5
        with torch.no_grad():
            if conv.double()(x.double()).abs().min().item() >= 0.05:
                return conv.float(), x
    raise AssertionError("no seed keeps |up + bias| >= 0.05")


def test_decoder_level_end_to_end(cv):
    conv, x = _level_case()
    deconv = nn.Sequential(conv, nn.ReLU(inplace=True))
    pr, skip = seeded(61, 1, 1, 3, 5), seeded(62, 1, 2, 5, 9)
    g = seeded(63, 1, 5, 5, 9)

    def run(dtype, device, on, timer=None):
        m = copy.deepcopy(deconv).to(device=device, dtype=dtype)
        ins = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in (x, pr, skip)]
        old = cv.set_option("decoder_train", on)
        cv.set_timer(timer)
        try:
            out = cv.decoder_level(m, *ins)
            grads = torch.autograd.grad(out, [ins[0], m[0].weight, m[0].bias, ins[1], ins[2]],
                                        g.to(device=device, dtype=dtype))
        finally:
            cv.set_timer(None)
            cv.set_option("decoder_train", old)
        return out, grads
    _, ref = run(torch.float64, "cpu", True)                   # CPU tensors never reach the library
    t_off, t_on = cv.LaunchTimer(), cv.LaunchTimer()
    o_off, off = run(torch.float32, "cuda", False, t_off)
    o_on, on = run(torch.float32, "cuda", True, t_on)
    torch.cuda.synchronize()
    assert t_off.summary() == {}
    s = t_on.summary()
    assert sorted(s) == ["decoder_cat_bwd_kernel", "decoder_cat_kernel"], s
    assert s["decoder_cat_kernel"]["launches"] == 1 and s["decoder_cat_bwd_kernel"]["launches"] == 1
    assert (o_on - o_off).abs().max().item() <= 1e-6            # the forward test's band for the upsampled channel
    for name, a, b, r in zip(("x", "weight", "bias", "pr", "skip"), on, off, ref):
        check("decoder_level grad " + name, a, b, r)
