"""CPU: the Cap[_ds][_lr][-mask] restatement (tests/cap_oracle.py) against the reference fixture
(tests/golden/golden_cap.npz), the loss factory's name gate, the divisor that losses_pyramid1
hands to the fused op, and the op's argument validation (no kernel is launched)."""
import math

import pytest
import torch

from tests import cap_oracle as CO
from tests.conftest import Golden

BUILT = ["Cap", "Cap_ds", "Cap-mask", "Cap_ds-mask"]
CASES = [("pyr7", "Cap_ds-mask"), ("pyr7", "Cap_ds"), ("small", "Cap-mask"), ("small", "Cap_ds_lr-mask"),
         ("lowcontrast", "Cap_ds-mask"), ("novalid", "Cap_ds-mask")]


def _inputs(z, case):
    meta = z.meta["cases"][case]
    batch = torch.from_numpy(z[case + ".batch"]).double() / 255.0
    H, W, nedge, n = meta["H"], meta["W"], meta["nedge"], meta["levels"]
    batch1 = torch.flip(batch, dims=[-1])
    dLs = [torch.from_numpy(z["%s.dispL.%d" % (case, i)]).double().requires_grad_() for i in range(n)]
    dL1s = [torch.from_numpy(z["%s.dispL1.%d" % (case, i)]).double().requires_grad_() for i in range(n)]
    args = (batch[:, 3:6], batch[:, :3, nedge:H - nedge, nedge:W - nedge], dLs, list(range(n)), [nedge, nedge],
            batch1[:, :3], batch1[:, 3:6, nedge:H - nedge, nedge:W - nedge], dL1s, [nedge, nedge])
    return meta, args, dLs, dL1s


def _weights(n, maxepoch, epoch):
    from dsmnet_amd import train
    lf = train.losses("Cap_ds-mask", n, maxepoch)
    lf.Weight_Adjust_levels(epoch)
    return lf.weight_levels


@pytest.mark.parametrize("name", BUILT + ["cap_DS-mask"])
def test_cap_names_build_the_fused_pyramid_loss(name):
    from dsmnet_amd import train
    lf = train.losses(name, 7, 10)
    assert lf.flag_mask == ("mask" in name)
    assert lf.lossesfun == lf.losses_pyramid1
    assert lf.lossfun == lf.loss_Cap_ds_lr
    assert lf.cap_terms == (("ds",) if "ds" in name.lower() else ())
    assert lf.weight_levels == [0, 0, 0, 0, 0, 0, 1]


@pytest.mark.parametrize("name", ["Cap_lr", "Cap_ds_lr", "Cap_ds_lr-mask", "cap_LR-mask", "common", "common-mask",
                                  "SsSMnet", "SsSMnet-mask", "depthmono"])
def test_unbuilt_names_still_raise(name):
    from dsmnet_amd import train
    with pytest.raises(NotImplementedError, match="not built"):
        train.losses(name, 7)


def test_the_message_lists_what_is_built():
    from dsmnet_amd import train
    with pytest.raises(NotImplementedError, match="Cap_ds-mask"):
        train.losses("Cap_ds_lr", 7)


def test_nedge_follows_the_mask_flag(monkeypatch):
    """train_step_selfsup crops 64 pixels with -mask and none without (stereo_selfsupervised.py)."""
    from dsmnet_amd import train
    seen = []

    def forward(model, lossfun, batch, nedge, augment):
        seen.append(nedge)
        return 0, [torch.zeros(1, 1, 4, 4)]
    monkeypatch.setattr(train, "_selfsup_forward", forward)

    class Model(object):
        def train(self):
            pass

    class Optim(object):
        def zero_grad(self):
            pass
    for name in ("Cap_ds-mask", "Cap_ds"):
        train.train_step_selfsup(Model(), Optim(), train.losses(name, 7), torch.zeros(1, 6, 8, 8), world=1)
    assert seen == [64, 0]


@pytest.mark.parametrize("case,name", CASES)
def test_restatement_matches_reference_fixture(case, name):
    z = Golden("cap")
    assert name in z.meta["cases"][case]["names"]
    meta, args, dLs, dL1s = _inputs(z, case)
    wl = _weights(meta["count_levels"], meta["maxepoch"], meta["epoch"])
    stats = []
    torch.manual_seed(meta["seed"])
    loss, delts = CO.losses_pyramid1(wl, "mask" in name, CO.terms_of(name), *args, stats=stats)
    loss.backward()
    tag = "%s.%s" % (case, name)
    want = float(z[tag + ".loss"])
    assert len(delts) == meta["levels"]
    assert abs(float(loss.detach()) - want) <= 1e-12 * abs(want), (tag, float(loss.detach()), want)
    ws = z[tag + ".w"]
    assert len(ws) == len(stats)
    for (w, n_valid, _), w_ref, n_ref in zip(stats, ws, z[tag + ".valid"]):
        assert int(n_valid) == int(n_ref)
        assert abs(float(w) - float(w_ref)) <= 1e-12 * float(w_ref)
    for i in range(meta["levels"]):
        for d, key in ((dLs[i], "gL"), (dL1s[i], "gL1")):
            g = torch.from_numpy(z["%s.%s.%d" % (tag, key, i)])
            assert g.dtype == torch.float64
            err = (d.grad - g).abs().max().item()
            assert err <= 1e-12 * max(g.abs().max().item(), 1e-300), (tag, key, i, err)


def test_zero_valid_pixels_give_w_0001_and_a_finite_loss():
    """What the reference's own lines give when mask_ap selects nothing: the empty mean is NaN,
    Python's max(0, nan) is 0, so w = 0.001 -- recorded by the generator, restated without NaN."""
    z = Golden("cap")
    tag = "novalid.Cap_ds-mask"
    assert z[tag + ".valid"].tolist() == [0, 0]
    assert z[tag + ".w"].tolist() == [0.001, 0.001]
    assert math.isfinite(float(z[tag + ".loss"]))
    meta, args, dLs, dL1s = _inputs(z, "novalid")
    stats = []
    torch.manual_seed(meta["seed"])
    loss, _ = CO.losses_pyramid1([1], True, ("ds",), *args, stats=stats)
    loss.backward()
    assert [float(s[0]) for s in stats] == [0.001, 0.001]
    assert math.isfinite(float(loss.detach()))
    assert all(bool(torch.isfinite(d.grad).all()) for d in dLs + dL1s)


def test_the_fixture_holds_the_masked_mean_and_w_above_its_floor():
    """"lowcontrast": some pixels invalid, the masked mean SSIM above 0.75 and the mean over every
    pixel below it.  The reference's own w is then above 0.001, and only a restatement that takes
    the mean over mask_ap (no fallback, though fewer than 1024 pixels are valid) reproduces it --
    which test_restatement_matches_reference_fixture holds to 1e-12."""
    from tests import selfsup_oracle as SO
    z = Golden("cap")
    tag = "lowcontrast.Cap_ds-mask"
    assert all(0 < n < 0.9 * 960 for n in z[tag + ".valid"].tolist())
    assert all(w > 0.002 for w in z[tag + ".w"].tolist())
    meta, args, dLs, dL1s = _inputs(z, "lowcontrast")
    stats = []
    SO.losses_pyramid1([1], True, *args, delts=[(1e-5,) * 4], stats=stats)        # the depthmono rule, same inputs
    assert all(bool(fallback) and float(w) == 0.001 for w, fallback, _ in stats)


def test_upsampled_levels_pass_their_own_level_as_the_divisor(monkeypatch):
    """loss.py:456: factor = 2**level of the output's own level, while the warp's scale_factor and
    the image level stop at maxlevel = 2."""
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd import train
    calls = []

    def stub(*args, **kwargs):
        calls.append((args, kwargs))
        return torch.zeros(())
    monkeypatch.setattr(cv, "selfsup_pyramid_loss", stub)
    lf = train.losses("Cap_ds-mask", 7, 10)
    lf.Weight_Adjust_levels(3)
    h, w = 64, 128
    im = torch.rand(1, 3, h, w)
    dLs = [torch.rand(1, 1, -(-h // 2 ** k), -(-w // 2 ** k)) for k in range(7)]
    torch.manual_seed(0)
    lf({"imR_src": im, "imL": im, "dispLs": dLs, "scale_dispLs": list(range(7)), "LeftTop": [0, 0],
        "imR1_src": im, "imL1": im, "dispL1s": dLs, "scale_dispL1s": list(range(7)), "LeftTop1": [0, 0]})
    (args, kwargs), = calls
    assert kwargs["objective"] == "cap" and kwargs["terms"] == ("ds",)
    assert kwargs["ds_divisors"] == [1, 2, 4, 8, 16, 32, 64]
    levels, weights, factors, flag_mask, delts = args[8:13]
    assert levels == [0, 1, 2, 2, 2, 2, 2] and factors == [1, 2, 4, 4, 4, 4, 4] and flag_mask is True
    assert all(tuple(d.shape[2:]) == (16, 32) for d in args[3][2:])
    # the CPU random stream: four draws per weighted entry, in order
    torch.manual_seed(0)
    assert delts == [tuple(train._draw_delt() for _ in range(4)) for _ in range(7)]
    # depthmono-mask: today's call, no new keyword
    calls.clear()
    lf = train.losses("depthmono-mask", 7, 10)
    lf({"imR_src": im, "imL": im, "dispLs": dLs, "scale_dispLs": list(range(7)), "LeftTop": [0, 0],
        "imR1_src": im, "imL1": im, "dispL1s": dLs, "scale_dispL1s": list(range(7)), "LeftTop1": [0, 0]})
    assert calls[0][1] == {}


@pytest.mark.parametrize("kwargs", [{"objective": "capp"}, {"objective": "cap", "terms": ("ds", "rl")},
                                    {"objective": "cap", "terms": ("ds",), "ds_divisors": [0]},
                                    {"objective": "cap", "ds_divisors": [1, 2]},
                                    {"objective": "depthmono", "ds_divisors": [2]},
                                    {"terms": ("ds",)}])
def test_argument_validation(kwargs):
    from dsmnet_amd import costvolume as cv
    im = torch.rand(1, 3, 16, 24)
    d = torch.rand(1, 1, 16, 24)
    with pytest.raises(ValueError):
        cv.selfsup_pyramid_loss(im, im, (0, 0), [d], im, im, (0, 0), [d], [0], [1.0], [1], True, [(1e-5,) * 4],
                                **kwargs)


def test_cpu_tensors_have_no_fallback():
    from dsmnet_amd import costvolume as cv
    im = torch.rand(1, 3, 16, 24)
    d = torch.rand(1, 1, 16, 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.selfsup_pyramid_loss(im, im, (0, 0), [d], im, im, (0, 0), [d], [0], [1.0], [1], True, [(1e-5,) * 4],
                                objective="cap", terms=("ds",), ds_divisors=[2])


def test_abi_flags_word(hip_lib):
    """0 and 1 are depthmono as ever; the Cap bits need DSM_SELFSUP_CAP; anything else is refused
    before any launch (the pointers here are never dereferenced on the host)."""
    import ctypes
    from dsmnet_amd import _lib
    items = (_lib.SelfsupItem * 2)()
    for it in items:
        it.im = it.src = it.disp = it.disp_other = 16
        it.B, it.h, it.w, it.H0, it.W0, it.scale_factor = 1, 20, 30, 20, 30, 1
    ws = ctypes.c_void_p(16)
    for flags in (4, 5, 8, 12, 16, 32, -1):
        assert hip_lib.dsm_selfsup_fwd(items, 2, flags, ws, ws, ws, None) == -1, flags
    items[0].ds_divisor = -1
    assert hip_lib.dsm_selfsup_fwd(items, 2, _lib.DSM_SELFSUP_CAP | _lib.DSM_SELFSUP_DS, ws, ws, ws, None) == -1
    # The gather needs only grad_disp: without it the call is refused as an argument error; with it
    # and no grad_other the pointer check passes for a flags word without the lr term only.  The
    # work list here has more than 2^30 tiles, which is refused after that check and before any
    # launch, with another code.
    items[0].ds_divisor = 0
    for it in items:
        it.B, it.h, it.w = 1 << 20, 1600, 1600
    cap, cap_lr = _lib.DSM_SELFSUP_CAP | _lib.DSM_SELFSUP_DS, _lib.DSM_SELFSUP_CAP | _lib.DSM_SELFSUP_LR
    assert hip_lib.dsm_selfsup_bwd(items, 2, cap, ws, ws, ws, None) == -1
    for it in items:
        it.grad_disp = 16
    assert hip_lib.dsm_selfsup_bwd(items, 2, cap, ws, ws, ws, None) == -2
    for flags in (cap_lr, 0, 1):
        assert hip_lib.dsm_selfsup_bwd(items, 2, flags, ws, ws, ws, None) == -1, flags
