"""CPU: the head-confidence op's float64 oracle (tests/headconf_oracle.py), its host-side dispatch and
argument checks (``dsm_disp_confidence_fwd_plan`` launches nothing), and the Python layers' refusals."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import headconf_oracle as HO


@pytest.mark.parametrize("name", sorted(HO.CASES))
def test_oracle_agrees_with_interpolate_and_softmax_in_float64(name):
    """The explicit interpolation against ``F.interpolate(mode="trilinear")`` -> ``softmax`` in float64:
    the fine values, and the two maps that do not depend on the arg-max bin, to 1e-12 (relative to the
    disparity range for ``disp``).  (``F.interpolate`` evaluates the clamped top bins as w0 P + w1 P, so its
    arg-max there is decided by rounding: the window maps are not compared.)"""
    _, osize, negate, align, _ = HO.CASES[name]
    cost = HO.case_cost(name)
    v = HO.fine_values(cost, osize, negate, align)
    got = HO.from_values(v, 4)
    ref = HO.torch_heads(cost, osize, negate, align, 4, dtype=torch.float64)
    assert np.abs(v - ref["values"]).max() <= 1e-12
    assert np.abs(got["entropy"] - ref["entropy"]).max() <= 1e-12
    assert np.abs(got["disp"] - ref["disp"]).max() <= 1e-12 * v.shape[1]


@pytest.mark.parametrize("name", ["up4_empty_seg", "interp_align", "gc_ds4"])
def test_oracle_whole_range_window_is_the_expectation(name):
    _, osize, negate, align, _ = HO.CASES[name]
    v = HO.fine_values(HO.case_cost(name), osize, negate, align)
    for r in (v.shape[1] - 1, v.shape[1], 10 ** 6):
        got = HO.from_values(v, r)
        assert np.abs(got["pwin"] - 1.0).max() <= 1e-14
        assert np.abs(got["peak"] - got["disp"]).max() <= 1e-11


def test_oracle_constant_cost():
    got = HO.heads(torch.full((1, 6, 3, 5), 2.5), (24, 7, 11), radius=3)
    assert (got["dstar"] == 0).all()
    assert np.abs(got["entropy"] - math.log(24)).max() <= 1e-13
    assert np.abs(got["pmax"] - 1.0 / 24).max() <= 1e-15
    assert np.abs(got["pwin"] - 4.0 / 24).max() <= 1e-15
    assert np.isinf(got["gap"]).all()


def test_oracle_is_shift_invariant_and_keeps_the_end_ties():
    cost = HO.case_cost("up4_empty_seg")
    a = HO.heads(cost, (24, 12, 70))
    b = HO.heads(cost.double() + 3.0, (24, 12, 70))
    assert (a["dstar"] == b["dstar"]).all()
    for k in HO.MAPS:
        assert np.abs(a[k] - b[k]).max() <= 1e-12 * (24 if k in ("disp", "peak") else 1)
    # D = 4 Dc, align_corners = False: bins (0, 1) and (D-2, D-1) are equal, so d* is never 1 or D-1
    v = HO.fine_values(cost, (24, 12, 70))
    assert np.array_equal(v[:, 0], v[:, 1]) and np.array_equal(v[:, 22], v[:, 23])
    assert not np.isin(a["dstar"], (1, 23)).any()
    assert np.isin(a["dstar"], (0, 22)).mean() > 0.1            # and a fair share of pixels sit on such a pair


# ------------------------------------------------------------------------------------------ dispatch --
PLANS = [
    ((2, 6, 3, 18), (24, 12, 70), False, "conf_up4<4>"),
    ((1, 48, 96, 320), (192, 384, 1280), False, "conf_up4<4>"),
    ((2, 5, 4, 9), (13, 9, 23), True, "conf<true,4>"),
    ((1, 5, 3, 6), (12, 7, 15), False, "conf<true,4>"),
    ((1, 6, 3, 18), (24, 12, 70), True, "conf<true,4>"),         # x4 with align_corners: not the x4 head
    ((1, 2, 3, 5), (8, 6, 10), False, "conf<true,4>"),           # D = 4 Dc with Dc < 4: not the x4 head
    ((1, 1, 3, 5), (4, 6, 10), False, "conf<true,2>"),
    ((2, 10, 5, 70), None, False, "conf<false,4>"),
    ((1, 6, 3, 17), None, False, "conf<false,2>"),
    ((1, 3, 2, 9), None, False, "conf<false,1>"),
]


@pytest.mark.parametrize("cshape,osize,align,plan", PLANS)
def test_plan_name_of_every_branch(hip_lib, cshape, osize, align, plan):
    from dsmnet_amd import costvolume as cv
    B, Dc, Hc, Wc = cshape
    D, H, W = osize or (Dc, Hc, Wc)
    p = ctypes.c_void_p(16)
    assert cv.confidence_plan_name(p, p, B, Dc, Hc, Wc, D, H, W, align_corners=align) == plan
    # the selection is the soft-argmin forward's
    sa = cv.soft_argmin_fwd_plan_name(p, p, None, B, Dc, Hc, Wc, D, H, W, align_corners=align)
    assert plan == ("conf_" + sa if sa.startswith("up4") else sa.replace("fwd", "conf"))


def test_argument_validation_returns_codes(hip_lib):
    from dsmnet_amd import _lib
    null, one = None, ctypes.c_void_p(16)
    dims = (1, 6, 3, 18, 24, 12, 70)
    buf = ctypes.create_string_buffer(96)
    for fn, tail in ((hip_lib.dsm_disp_confidence_fwd, (null,)), (hip_lib.dsm_disp_confidence_fwd_plan, (buf, 96))):
        call = lambda cost, disp, radius, dtype: fn(cost, disp, one, one, one, one, *dims, 0, 0, radius, dtype, *tail)
        assert call(null, one, 4, _lib.DSM_F32) == -1          # no cost
        assert call(one, null, 4, _lib.DSM_F32) == -1          # no disp
        assert call(one, one, -1, _lib.DSM_F32) == -1          # radius
        assert call(one, one, 4, 7) == -2                      # dtype
    assert hip_lib.dsm_disp_confidence_fwd_plan(one, one, null, null, null, null, 1, 6, 3, 18, 0, 12, 70, 0, 0, 4, 0, buf, 96) == -1
    assert hip_lib.dsm_disp_confidence_fwd_plan(one, one, null, null, null, null, *dims, 0, 0, 2 ** 31 - 1, 0, buf, 96) == 0
    assert buf.value == b"conf_up4<4>"
    assert hip_lib.dsm_disp_confidence_fwd_plan(one, one, null, null, null, null, *dims, 0, 0, 4, 0, None, 96) == -1


# ------------------------------------------------------------------------------------ Python layers --
def test_op_refuses_cpu_tensors_and_bad_arguments():
    from dsmnet_amd import costvolume as cv
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.soft_argmin_confidence(torch.zeros(1, 4, 2, 8))
    assert cv.DispConfidence._fields == ("disp", "peak", "pmax", "pwin", "entropy")


def test_predict_confidence_refuses_a_direct_regression_network():
    from dsmnet_amd import postprocess
    from dsmnet_amd.models import model_create_by_name
    model = model_create_by_name("dispnetcorr", 192)
    x = torch.zeros(1, 3, 64, 128)
    with pytest.raises(TypeError, match="dispnetcorr.*regresses disparity directly"):
        postprocess.predict_confidence(model, x, x)


def test_models_with_a_cost_head_expose_it():
    from dsmnet_amd.models import model_create_by_name
    for name in ("psmnet", "gcnet"):
        assert callable(model_create_by_name(name, 16).head_cost)
    for name in ("dispnet", "dispnetcorr", "iresnet"):
        assert not hasattr(model_create_by_name(name, 192), "head_cost")


def test_deploy_parser_knows_the_confidence_options():
    from dsmnet_amd import deploy
    ap = deploy.build_parser()
    d = ap.parse_args([])
    assert (d.confidence, d.peak, d.conf_radius, d.conf_threshold) == (False, False, 4, None)
    a = ap.parse_args(["--confidence", "--peak", "--conf_radius", "2", "--conf_threshold", "0.8", "--lr_check"])
    assert a.confidence and a.peak and a.lr_check and a.conf_radius == 2 and a.conf_threshold == 0.8
    # refusals that need no GPU: they come before the device check
    for argv in (["--peak", "--lr_check"], ["--conf_threshold", "0.5"], ["--confidence", "--conf_radius", "-1"],
                 ["--fill"]):
        with pytest.raises(SystemExit) as e:
            deploy.main(argv)
        assert isinstance(e.value.code, str)
