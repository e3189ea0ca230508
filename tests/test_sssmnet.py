"""CPU: the SsSMnet[-mask] / common[-mask] restatement (tests/sssmnet_oracle.py) against the
reference fixture (tests/golden/golden_sssmnet.npz), the epsilon draw count and order, the name
dispatch of ``train.selfsup_losses``, the gate of ``train.losses`` (which did not move), and the
argument validation of the op and of the new entry points (no kernel is launched)."""
import math

import pytest
import torch

from tests import sssmnet_oracle as XO
from tests.conftest import Golden

NAMES = ["SsSMnet", "SsSMnet-mask", "common", "common-mask"]
CASES = [(c, n) for c in ("pyr7", "lowcontrast", "novalid", "sub1024") for n in NAMES]
# every spelling that the existing tests list as refused by train.losses
UNBUILT = ["Cap_lr", "Cap_ds_lr", "Cap_ds_lr-mask", "cap_LR-mask", "common", "common-mask", "SsSMnet", "SsSMnet-mask",
           "depthmono"]
BUILT = ["depthmono-mask", "Cap", "Cap_ds", "Cap-mask", "Cap_ds-mask"]


def _objective(name):
    return "sssmnet" if "sssmnet" in name.lower() else "common"


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
    lf = train.selfsup_losses("common-mask", n, maxepoch)
    lf.Weight_Adjust_levels(epoch)
    return lf.weight_levels


@pytest.mark.parametrize("case,name", CASES)
def test_restatement_matches_reference_fixture(case, name):
    z = Golden("sssmnet")
    assert name in z.meta["cases"][case]["names"]
    meta, args, dLs, dL1s = _inputs(z, case)
    wl = _weights(meta["count_levels"], meta["maxepoch"], meta["epoch"])
    stats = []
    torch.manual_seed(meta["seed"])
    loss, delts = XO.losses_pyramid(_objective(name), wl, "mask" in name, *args, stats=stats)
    # the epsilon draws: their count, and where they leave the CPU generator (the reference's next draw)
    per_entry = 6 if name == "SsSMnet-mask" else 4
    assert [len(d) for d in delts] == [per_entry] * meta["levels"]
    assert sum(len(d) for d in delts) == int(z["%s.%s.draws" % (case, name)])
    assert float(torch.rand(1)[0]) == float(z["%s.%s.next" % (case, name)])
    loss.backward()
    tag = "%s.%s" % (case, name)
    want = float(z[tag + ".loss"])
    assert abs(float(loss.detach()) - want) <= 1e-12 * abs(want), (tag, float(loss.detach()), want)
    ws = z[tag + ".w"]
    assert len(ws) == len(stats)
    for (w, second, _), w_ref, second_ref in zip(stats, ws, z[tag + ".second"]):
        assert int(second) == int(second_ref)           # common: the fallback flag; SsSMnet: valid pixels
        assert abs(float(w) - float(w_ref)) <= 1e-12 * float(w_ref)
    for i in range(meta["levels"]):
        for d, key in ((dLs[i], "gL"), (dL1s[i], "gL1")):
            g = torch.from_numpy(z["%s.%s.%d" % (tag, key, i)])
            assert g.dtype == torch.float64
            err = (d.grad - g).abs().max().item()
            assert err <= 1e-12 * max(g.abs().max().item(), 1e-300), (tag, key, i, err)


def test_the_draw_order_is_the_references():
    """imL_wrap, imL1_wrap, then the two second warps; with the same seed the restatement given the
    draws explicitly equals the restatement that draws them itself."""
    from tests import selfsup_oracle as SO
    z = Golden("sssmnet")
    for name in ("common-mask", "SsSMnet-mask"):
        meta, args, _, _ = _inputs(z, "sub1024")
        torch.manual_seed(meta["seed"])
        drawn = tuple(SO.draw_delt() for _ in range(6 if name == "SsSMnet-mask" else 4))
        a, _ = XO.losses_pyramid(_objective(name), [1], True, *args, delts=[drawn])
        assert abs(float(a.detach()) - float(z["sub1024.%s.loss" % name])) <= 1e-12
        if name == "common-mask":               # swapping two draws is seen
            b, _ = XO.losses_pyramid("common", [1], True, *args, delts=[(drawn[1], drawn[0]) + drawn[2:]])
            assert float(b.detach()) != float(a.detach())


def test_the_fixture_holds_what_its_cases_are_for():
    z = Golden("sssmnet")
    for name in NAMES:
        assert all(w > 0.002 for w in z["lowcontrast.%s.w" % name].tolist())
        assert z["novalid.%s.w" % name].tolist() == [0.001, 0.001]
        assert math.isfinite(float(z["novalid.%s.loss" % name]))
    assert z["novalid.SsSMnet-mask.second"].tolist() == [0, 0]                   # no valid pixel
    assert z["novalid.common-mask.second"].tolist() == [1, 1]                    # fallback
    assert z["sub1024.common.second"].tolist() == [1, 1]
    assert all(0 < n < 1024 for n in z["sub1024.SsSMnet.second"].tolist())
    assert z["lowcontrast.common.second"].tolist() == [0, 0]                     # the masked mean
    assert set(z["pyr7.common.second"].tolist()) == {0, 1}
    assert z.meta["cases"]["pyr7"]["levels"] == 7


@pytest.mark.parametrize("name", UNBUILT + BUILT + ["COMMON-mask", "cap_ds_LR"])
def test_selfsup_losses_dispatches_in_setlossfuns_order(name):
    from dsmnet_amd import train
    low = name.split("-")[0].lower()
    lf = train.selfsup_losses(name, 7, 10)
    assert isinstance(lf, train.losses)
    assert lf.flag_mask == ("mask" in name)
    assert lf.lossesfun == (lf.losses_pyramid2 if "sssmnet" in low else lf.losses_pyramid1)
    assert lf.weight_levels == [0, 0, 0, 0, 0, 0, 1]
    if "sssmnet" in low:
        assert lf.lossfun == lf.loss_SsSMnet
    elif "depthmono" in low:
        assert lf.lossfun == lf.loss_depthmono
    elif "cap" in low:
        assert lf.lossfun == lf.loss_Cap_ds_lr
        assert lf.cap_terms == tuple(t for t in ("ds", "lr") if t in low)
    else:
        assert lf.lossfun == lf.loss_common


def test_selfsup_losses_refuses_what_is_not_self_supervised():
    from dsmnet_amd import train
    with pytest.raises(ValueError, match="train.losses"):
        train.selfsup_losses("supervised", 3)
    with pytest.raises(ValueError):
        train.selfsup_losses("photometric", 3)            # the reference's assert, loss.py:348
    with pytest.raises(ValueError):
        train.selfsup_losses("depthmono2", 3)
    # setlossfun's order (loss.py:363-377) for names that hold two of its words
    with pytest.raises(ValueError, match="train.losses"):
        train.selfsup_losses("cap_supervised", 3)
    assert train.selfsup_losses("cap_depthmono", 3).lossfun.__name__ == "loss_depthmono"
    assert train.selfsup_losses("sssmnet_cap", 3).lossfun.__name__ == "loss_SsSMnet"
    assert train.selfsup_losses("cap_common", 3).lossfun.__name__ == "loss_Cap_ds_lr"


@pytest.mark.parametrize("name", UNBUILT)
def test_train_losses_kept_its_gate(name):
    from dsmnet_amd import train
    with pytest.raises(NotImplementedError, match="not built"):
        train.losses(name, 7)


def _pyramid_call(lf, monkeypatch, n_delts=4):
    from dsmnet_amd import costvolume as cv
    calls = []

    def stub(*args, **kwargs):
        calls.append((args, kwargs))
        return torch.zeros(())
    monkeypatch.setattr(cv, "selfsup_pyramid_loss", stub)
    lf.Weight_Adjust_levels(3)
    h, w = 64, 128
    im = torch.rand(1, 3, h, w)
    dLs = [torch.rand(1, 1, -(-h // 2 ** k), -(-w // 2 ** k)) for k in range(7)]
    torch.manual_seed(0)
    lf({"imR_src": im, "imL": im, "dispLs": dLs, "scale_dispLs": list(range(7)), "LeftTop": [0, 0],
        "imR1_src": im, "imL1": im, "dispL1s": dLs, "scale_dispL1s": list(range(7)), "LeftTop1": [0, 0]})
    (args, kwargs), = calls
    # the CPU random stream: n_delts draws per weighted entry, in order
    torch.manual_seed(0)
    from dsmnet_amd import train
    assert args[12] == [tuple(train._draw_delt() for _ in range(n_delts)) for _ in range(7)]
    return args, kwargs


@pytest.mark.parametrize("name,kwargs", [
    ("common-mask", {"objective": "common"}), ("common", {"objective": "common"}), ("depthmono", {}),
    ("SsSMnet-mask", {"objective": "sssmnet", "ds_divisors": [1, 2, 4, 8, 16, 32, 64]}),
    ("SsSMnet", {"objective": "sssmnet", "ds_divisors": [1, 2, 4, 8, 16, 32, 64]}),
    ("Cap_ds_lr-mask", {"objective": "cap", "terms": ("ds", "lr"), "ds_divisors": [1, 2, 4, 8, 16, 32, 64]}),
    ("Cap_lr", {"objective": "cap", "terms": ("lr",), "ds_divisors": [1, 2, 4, 8, 16, 32, 64]})])
def test_selfsup_losses_hands_the_objective_to_the_op(monkeypatch, name, kwargs):
    from dsmnet_amd import train
    args, got = _pyramid_call(train.selfsup_losses(name, 7, 10), monkeypatch, 6 if name == "SsSMnet-mask" else 4)
    assert got == kwargs
    levels, weights, factors, flag_mask, delts = args[8:13]
    assert levels == [0, 1, 2, 2, 2, 2, 2] and factors == [1, 2, 4, 4, 4, 4, 4] and flag_mask is ("mask" in name)


@pytest.mark.parametrize("name", BUILT)
def test_built_names_make_the_same_call_through_either_class(monkeypatch, name):
    from dsmnet_amd import train
    a = _pyramid_call(train.losses(name, 7, 10), monkeypatch)
    b = _pyramid_call(train.selfsup_losses(name, 7, 10), monkeypatch)
    assert a[1] == b[1] and a[0][8:13] == b[0][8:13]
    assert all(torch.equal(x, y) for x, y in zip(a[0][3], b[0][3]))


@pytest.mark.parametrize("kwargs,message", [
    ({"objective": "common", "ds_divisors": [2]}, "common has both terms and no ds_divisors"),
    ({"objective": "common", "terms": ("ds",)}, "common has both terms"),
    ({"objective": "common", "delts": [(1e-5,) * 6]}, "common-mask takes four epsilons"),
    ({"objective": "sssmnet"}, "sssmnet-mask takes six epsilons"),
    ({"objective": "sssmnet", "mask": False, "delts": [(1e-5,) * 6]}, "sssmnet takes four epsilons"),
    ({"objective": "sssmnet", "delts": [(1e-5,) * 6], "terms": ("lr",)}, "sssmnet has both terms"),
    ({"objective": "sssmnet", "delts": [(1e-5,) * 6], "ds_divisors": [0]}, "one integer >= 1"),
    ({"objective": "Common"}, "is none of")])
def test_argument_validation(kwargs, message):
    """Each refusal by its own message: on a tree without the objectives every one of these would be
    the "is none of" error instead."""
    from dsmnet_amd import costvolume as cv
    im = torch.rand(1, 3, 16, 24)
    d = torch.rand(1, 1, 16, 24)
    kw = dict(kwargs)
    delts, mask = kw.pop("delts", [(1e-5,) * 4]), kw.pop("mask", True)
    with pytest.raises(ValueError, match=message):
        cv.selfsup_pyramid_loss(im, im, (0, 0), [d], im, im, (0, 0), [d], [0], [1.0], [1], mask, delts, **kw)


def test_cpu_tensors_have_no_fallback():
    from dsmnet_amd import costvolume as cv
    im = torch.rand(1, 3, 16, 24)
    d = torch.rand(1, 1, 16, 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.selfsup_pyramid_loss(im, im, (0, 0), [d], im, im, (0, 0), [d], [0], [1.0], [1], True, [(1e-5,) * 4],
                                objective="common")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.selfsup_pyramid_loss(im, im, (0, 0), [d], im, im, (0, 0), [d], [0], [1.0], [1], True, [(1e-5,) * 6],
                                objective="sssmnet", ds_divisors=[2])


def test_abi_flags_word_of_the_new_entry_points(hip_lib):
    """The new entry points take common[-mask] and SsSMnet[-mask] and nothing else; the older ones
    still refuse the new bits; SsSMnet needs its side array (the pointers here are never
    dereferenced on the host, and no call here gets as far as a launch)."""
    import ctypes
    from dsmnet_amd import _lib
    items = (_lib.SelfsupItem * 2)()
    for it in items:
        it.im = it.src = it.disp = it.disp_other = 16
        it.B, it.h, it.w, it.H0, it.W0, it.scale_factor = 2, 20, 30, 20, 30, 1
    ws = ctypes.c_void_p(16)
    common, sss = _lib.DSM_SELFSUP_COMMON, _lib.DSM_SELFSUP_SSSMNET
    assert ctypes.sizeof(_lib.SelfsupExt) == 24 and ctypes.sizeof(_lib.SelfsupItem) == 128
    ext = (_lib.SelfsupExt * 2)()
    for flags in (0, 1, 2, 6, 7, 15, common | 2, common | 4, common | sss, sss | 8, 64, -1):
        assert hip_lib.dsm_selfsup_ext_fwd(items, ext, 2, flags, ws, ws, ws, None) == -1, flags
        assert hip_lib.dsm_selfsup_ext_workspace_floats(items, 2, flags) == 0, flags
    for flags in (common, common | 1, sss, sss | 1):
        assert hip_lib.dsm_selfsup_fwd(items, 2, flags, ws, ws, ws, None) == -1, flags
        base = hip_lib.dsm_selfsup_workspace_floats(items, 2)
        # 16 row chunks x 2 sums per (item, sample) on top of the older workspace
        assert hip_lib.dsm_selfsup_ext_workspace_floats(items, 2, flags) == base + 2 * 2 * 16 * 2
        assert hip_lib.dsm_selfsup_ext_bwd(items, ext, 2, flags, ws, ws, ws, None) == -1       # no gradient buffers
    assert hip_lib.dsm_selfsup_ext_fwd(items, None, 3, common, ws, ws, ws, None) == -1
    # SsSMnet: no side array, or one without its warp buffer; backward: without the scatter buffer
    assert hip_lib.dsm_selfsup_ext_fwd(items, None, 2, sss, ws, ws, ws, None) == -1
    assert hip_lib.dsm_selfsup_ext_fwd(items, ext, 2, sss | 1, ws, ws, ws, None) == -1
    for it, e in zip(items, ext):
        it.grad_disp, e.warp = 16, 16
    assert hip_lib.dsm_selfsup_ext_bwd(items, ext, 2, sss, ws, ws, ws, None) == -1
    # refused after the argument checks and before any launch: 3 h w beyond the pre-pass's 32-bit index
    for it in items:
        it.B, it.h, it.w = 1, 1 << 15, 1 << 15
    assert hip_lib.dsm_selfsup_ext_fwd(items, None, 2, common, ws, ws, ws, None) == -2
    assert hip_lib.dsm_selfsup_ext_fwd(items, ext, 2, sss, ws, ws, ws, None) == -2
