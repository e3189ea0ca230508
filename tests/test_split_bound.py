"""CPU: the per-element yardstick of tests/split_bound.py discriminates before any GPU time is spent on it.

On a 32 -> 32 3x3x3 and a 64 -> 64 3x3 layer, for every input class of tests/test_split_contract_gpu.py:
the emulated f16x2 split (hi / lo through ``Tensor.half()``, which keeps subnormals; products summed in float64)
stays under half of the bound, the emulated f16 and bf16x3 forms under the bound itself; the split with its low
term dropped breaks the bound on the Gaussian control and on every heavy-tailed class; the split whose subnormal
residuals are flushed breaks it on every heavy-tailed class (on Gaussian inputs it is invisible under either
metric -- printed, not asserted).  And the Python restatement of
the exponent rule equals hand-computed values."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import split_bound as SB
from tests.helpers import seeded

LAYERS = {
    "3d": ((1, 32, 4, 8, 32), (32, 32, 3, 3, 3), lambda a, b: F.conv3d(a, b, padding=1)),
    "2d": ((1, 64, 12, 40), (64, 64, 3, 3), lambda a, b: F.conv2d(a, b, padding=1)),
}


@functools.lru_cache(maxsize=None)
def case(layer, cls):
    """(x, w, conv, terms) of one layer and class: the float64 convolutions are computed once."""
    shape, wshape, conv = LAYERS[layer]
    w = seeded(2, *wshape, scale=0.05)
    x, w = SB.make_input(cls, 1, shape, w)
    return x, w, conv, SB.conv_terms(x, w, conv)


def measured(layer, cls, mode="f16x2", mutant=None):
    x, w, conv, t = case(layer, cls)
    K = w[0].numel()
    ref, bound = SB.bound_from_terms(t, mode, SB.n_forward(mode, K), x.abs().max().item(), w.abs().max().item())
    return SB.ratio(SB.emulate(x, w, conv, mode, mutant=mutant), ref, bound)


@pytest.mark.parametrize("cls", SB.CLASSES)
@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_the_emulated_split_stays_under_half_the_bound(layer, cls):
    for mode in SB.MODES:
        r = measured(layer, cls, mode)
        print("%s %s %s: correct split at %.3f of the bound" % (layer, cls, mode, r))
        # f16 rounds each operand once: an output that is a single product (class Z) can sit at the bound itself
        assert r <= (0.5 if mode == "f16x2" else 1.0), (mode, r)


@pytest.mark.parametrize("cls", ("G",) + SB.HEAVY)
@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_a_dropped_low_term_breaks_the_bound(layer, cls):
    r = measured(layer, cls, mutant="drop_lo")
    x, w, conv, t = case(layer, cls)
    err = (SB.emulate(x, w, conv, "f16x2", mutant="drop_lo") - t["pre"]).abs()
    old = err.max().item() / t["pre"].abs().max().item()
    print("%s %s: low term dropped at %.1f x the bound (max/max %.1e)" % (layer, cls, r, old))
    assert r > 1.0, r


@pytest.mark.parametrize("cls", SB.HEAVY)
@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_flushed_subnormal_residuals_break_the_bound(layer, cls):
    r = measured(layer, cls, mutant="flush_lo")
    print("%s %s: subnormal residuals flushed at %.2f x the bound (Gaussian: %.3f, invisible)"
          % (layer, cls, r, measured(layer, "G", mutant="flush_lo")))
    assert r > 1.0, r


def test_the_mutants_are_the_split_itself_where_they_do_not_apply():
    """f16 has no low term and bf16x3 no subnormals to flush; an unknown mutant is refused."""
    x, w, conv, _ = case("2d", "G")
    assert torch.equal(SB.emulate(x, w, conv, "f16", mutant="drop_lo"), SB.emulate(x, w, conv, "f16"))
    with pytest.raises(ValueError):
        SB.emulate(x, w, conv, "f16x2", mutant="other")


ULP = 2.0 ** -11          # of float32 values in [2^12, 2^13): 2^12 * 2^-23


@pytest.mark.parametrize("amax,want", [
    (0.0, 60),                       # no exponent field to read: clamped
    (1.0, 12),
    (2.0 ** 12, 0),
    (2.0 ** 13 - ULP, 0),            # the top of [2^12, 2^13)
    (2.0 ** 13, -1),
    (2.0 ** -48, 60),                # the last maximum that still lands at 2^12
    (2.0 ** -49, 60),                # clamped from 61
    (2.0 ** -100, 60),
    (2.0 ** 72, -60),                # the first maximum that still lands at 2^12
    (2.0 ** 75, -60),                # clamped from -63: lands at 2^15, below fp16's 65504
    (2.0 ** -140, 60),               # a float32 subnormal
    (0.75, 13), (3.0, 11), (1e4, -1), (1e-9, 42),
])
def test_the_exponent_rule_equals_hand_computed_values(amax, want):
    e = SB.amax_exponent(amax)
    assert e == want
    if 2.0 ** -48 <= amax < 2.0 ** 73:
        assert 2.0 ** 12 <= amax * 2.0 ** e < 2.0 ** 13


def test_ratio_demands_exactness_where_the_bound_is_zero():
    ref, bound = torch.zeros(3, dtype=torch.float64), torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    assert SB.ratio(torch.tensor([0.0, 0.5, 0.0]), ref, bound) == 0.5
    assert SB.ratio(torch.tensor([0.0, 0.5, 1e-30]).double(), ref, bound) == float("inf")
    assert SB.ratio(torch.tensor([0.0, float("nan"), 0.0]), ref, bound) == float("inf")


def test_with_max_hits_the_value_exactly():
    x = seeded(3, 4, 5)
    for t in (2.0 ** -70, 2.0 ** -48, 2.0 ** 75, 3.0):
        assert SB.with_max(x, t).abs().max().item() == t
