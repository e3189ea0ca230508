"""CPU: the colour-augmentation planner (dsmnet_amd.transforms) and the float64 restatement
(tests/color_oracle.py) against the fixture written from the reference's own transforms, and the
argument checks of the fused op (no kernel is launched)."""
import ctypes
import random

import pytest
import torch

from tests import color_oracle as CO
from tests.conftest import Golden


def _case(case):
    z = Golden("color")
    meta = z.meta["cases"][case]
    return meta, torch.from_numpy(z[case + ".x"]), torch.from_numpy(z[case + ".out"]).double()


def _transform(kind):
    from dsmnet_amd import transforms as T
    if kind == "normalize":
        return T.Stereo_normalize()
    return T.Stereo_color(same_group=kind == "color_same")


def _planned(meta):
    random.seed(meta["seed"])
    torch.manual_seed(meta["seed"])
    B, C = meta["shape"][:2]
    return _transform(meta["kind"]).plan(B, C, "cpu")


def _restate(x, planned, reference_nan):
    out = x.double()
    for recs, alpha, G in planned:
        out = CO.restate(out, recs, alpha, G, reference_nan=reference_nan)
    return out


@pytest.mark.parametrize("case", ["same", "split", "normalize"])
def test_planner_and_restatement_reproduce_the_reference(case):
    meta, x, want = _case(case)
    got = _restate(x, _planned(meta), reference_nan=True)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert (got[~nan] - want[~nan]).abs().max().item() <= 2e-6


def test_fixture_reaches_the_nan_case():
    assert torch.isnan(_case("same")[2]).any() and torch.isnan(_case("split")[2]).any()


@pytest.mark.parametrize("case", ["same", "split", "normalize"])
def test_gamma_drift_is_finite_and_equal_where_the_reference_is(case):
    meta, x, want = _case(case)
    got = _restate(x, _planned(meta), reference_nan=False)
    assert torch.isfinite(got).all()
    ok = torch.isfinite(want)
    assert (got[ok] - want[ok]).abs().max().item() <= 2e-6


@pytest.mark.parametrize("case", ["same", "normalize"])
def test_channels_from_six_are_untouched(case):
    meta, x, want = _case(case)
    assert x.shape[1] == 7
    assert torch.equal(want[:, 6:], x[:, 6:].double())
    got = _restate(x, _planned(meta), reference_nan=False)
    assert torch.equal(got[:, 6:], x[:, 6:].double())


def test_planner_draw_counts():
    """randperm + 3 uniforms per step per image (per group when split), one normal_ per image
    (per group when split), nothing for Stereo_normalize."""
    from dsmnet_amd import transforms as T
    for same, G_draws in ((True, 1), (False, 2)):
        random.seed(3)
        torch.manual_seed(3)
        T.Stereo_color(same_group=same).plan(2, 6, "cpu")
        py, cpu = random.random(), torch.rand(1).item()
        random.seed(3)
        torch.manual_seed(3)
        for _ in range(2):                               # image by image, as the reference
            for _ in range(G_draws):
                torch.randperm(4)
                [random.random() for _ in range(12)]
            for _ in range(G_draws):
                torch.empty(3).normal_(0, 0.1)
        assert (py, cpu) == (random.random(), torch.rand(1).item())
    random.seed(4)
    torch.manual_seed(4)
    recs, alpha, G = T.Stereo_normalize().plan(3, 6, "cpu")[0]
    assert alpha is None and G == 2 and all(r[2] == CO.NORMALIZE for r in recs)
    py, cpu = random.random(), torch.rand(1).item()
    random.seed(4)
    torch.manual_seed(4)
    assert (py, cpu) == (random.random(), torch.rand(1).item())


def test_lighting_alphastd_zero_draws_nothing():
    from dsmnet_amd import transforms as T
    t = T.Compose([T.ColorJitter(), T.Lighting(alphastd=0.0), T.Normalize_Imagenet()])
    assert len(t.launches) == 1
    recs, alpha, G = t.plan(2, 6, "cpu")[0]
    assert alpha is None and all(r[2] == CO.JITTER | CO.NORMALIZE for r in recs)


def test_ops_refuse_cpu_tensors():
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd import transforms as T
    x = torch.rand(2, 6, 4, 8)
    recs = [((0, 1, 2, 3), (1.0, 0.0, 0.0, 1.0), CO.NORMALIZE, 0)] * 4
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.stereo_color(x, recs, None, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.Stereo_color()(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.Stereo_color_batch(x, T.Stereo_normalize())


def test_dsm_stereo_color_rejects_bad_arguments(hip_lib):
    from dsmnet_amd import _lib
    one = ctypes.c_void_p(16)

    def recs(n, order=(0, 1, 2, 3), flags=7, row=0):
        a = (_lib.ColorRecord * n)()
        for r in a:
            r.order[:] = list(order)
            r.jitter[:] = [1.0, 0.0, 0.0, 1.0]
            r.flags, r.alpha_row = flags, row
        return a

    good = recs(4)
    call = hip_lib.dsm_stereo_color
    assert call(None, one, good, 4, 2, 6, 4, 8, 2, None) == -1             # null x
    assert call(one, one, None, 4, 2, 6, 4, 8, 2, None) == -1              # null records
    assert call(one, None, good, 4, 2, 6, 4, 8, 2, None) == -1             # Lighting without alpha
    assert call(one, one, good, 4, 2, 5, 4, 8, 2, None) == -1              # C < 6
    assert call(one, one, good, 3, 2, 6, 4, 8, 2, None) == -1              # records != B * groups
    assert call(one, one, good, 4, 2, 6, 0, 8, 2, None) == -1              # H < 1
    assert call(one, one, good, 4, 2, 6, 4, 0, 2, None) == -1              # W < 1
    assert call(one, one, good, 4, 0, 6, 4, 8, 2, None) == -1              # B < 1
    assert call(one, one, recs(6), 6, 2, 6, 4, 8, 3, None) == -1           # groups not 1 or 2
    assert call(one, one, recs(4, order=(0, 1, 1, 3)), 4, 2, 6, 4, 8, 2, None) == -1   # not a permutation
    assert call(one, one, recs(4, order=(0, 1, 2, 4)), 4, 2, 6, 4, 8, 2, None) == -1
    assert call(one, one, recs(4, row=4), 4, 2, 6, 4, 8, 2, None) == -1    # alpha row out of range
    assert call(one, one, recs(4, flags=8), 4, 2, 6, 4, 8, 2, None) == -1  # unknown step
