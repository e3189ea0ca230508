"""CPU: the self-supervised depthmono restatement (tests/selfsup_oracle.py) against the
reference fixture and the live reference, the loss factory, and the C ABI's argument checks of
the fused op (no kernel is launched)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import reference_loader as RL
from tests import selfsup_oracle as SO
from tests.conftest import Golden


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
    lf = train.losses("depthmono-mask", n, maxepoch)
    lf.Weight_Adjust_levels(epoch)
    return lf.weight_levels


@pytest.mark.parametrize("case", ["pyr7", "ragged"])
def test_restatement_matches_reference_fixture(case):
    z = Golden("selfsup")
    for name in z.meta["cases"][case]["names"]:
        meta, args, dLs, dL1s = _inputs(z, case)
        wl = _weights(meta["count_levels"], meta["maxepoch"], meta["epoch"])
        torch.manual_seed(meta["seed"])
        loss, delts = SO.losses_pyramid1(wl, "mask" in name, *args)
        loss.backward()
        tag = "%s.%s" % (case, name)
        assert len(delts) == meta["levels"]
        assert abs(float(loss) - float(z[tag + ".loss"])) <= 1e-9 * abs(float(z[tag + ".loss"]))
        for i in range(meta["levels"]):
            for d, key in ((dLs[i], "gL"), (dL1s[i], "gL1")):
                want = torch.from_numpy(z["%s.%s.%d" % (tag, key, i)]).double()
                err = (d.grad - want).abs().max().item()
                assert err <= 1e-6 * max(want.abs().max().item(), 1e-12), (tag, key, i, err)


@pytest.mark.skipif(not RL.available(), reason="reference tree not present")
def test_restatement_matches_live_reference():
    from tests.golden import make_goldens_selfsup as MG
    ref = MG.load_reference()
    z = Golden("selfsup")
    meta, args, dLs, dL1s = _inputs(z, "ragged")
    wl = _weights(meta["count_levels"], meta["maxepoch"], meta["epoch"])
    ref.flag_mask, ref.weight_levels = True, wl
    keys = ("imR_src", "imL", "dispLs", "scale_dispLs", "LeftTop", "imR1_src", "imL1", "dispL1s", "LeftTop1")
    rargs = dict(zip(keys, args))
    rins = [d.detach().clone().requires_grad_() for d in dLs + dL1s]
    n = meta["levels"]
    rargs["dispLs"], rargs["dispL1s"], rargs["scale_dispL1s"] = rins[:n], rins[n:], list(range(n))
    torch.manual_seed(17)
    want = ref.losses_pyramid1(**rargs)
    want.backward()
    torch.manual_seed(17)
    mine, _ = SO.losses_pyramid1(wl, True, *args)
    mine.backward()
    assert abs(float(mine) - float(want)) <= 1e-9 * abs(float(want))
    for a, b in zip(dLs + dL1s, rins):
        assert (a.grad - b.grad).abs().max().item() <= 1e-9 * b.grad.abs().max().item()


def test_depthmono_mask_builds_the_fused_pyramid_loss():
    from dsmnet_amd import train
    lf = train.losses("depthmono-mask", 7, 10)
    assert lf.flag_mask
    assert lf.lossesfun == lf.losses_pyramid1
    assert lf.lossfun == lf.loss_depthmono
    assert lf.weight_levels == [0, 0, 0, 0, 0, 0, 1]


@pytest.mark.parametrize("name", ["SsSMnet", "SsSMnet-mask", "Cap_ds_lr", "common-mask"])
def test_unbuilt_objectives_still_raise(name):
    from dsmnet_amd import train
    with pytest.raises(NotImplementedError, match="not built"):
        train.losses(name)


def test_cpu_tensors_have_no_fallback():
    from dsmnet_amd import costvolume as cv
    im = torch.rand(1, 3, 16, 24)
    d = torch.rand(1, 1, 16, 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.selfsup_pyramid_loss(im, im, (0, 0), [d], im, im, (0, 0), [d], [0], [1.0], [1], True, [(1e-5,) * 4])


def test_train_step_selfsup_is_single_rank():
    from dsmnet_amd import train
    lf = train.losses("depthmono-mask", 1)
    with pytest.raises(NotImplementedError):
        train.train_step_selfsup(None, None, lf, torch.zeros(1, 6, 200, 200), world=2)


def test_abi_argument_checks(hip_lib):
    from dsmnet_amd import _lib
    assert ctypes.sizeof(_lib.SelfsupItem) == 128
    items = (_lib.SelfsupItem * 2)()
    for it in items:
        it.im = it.src = it.disp = it.disp_other = 16
        it.B, it.h, it.w, it.H0, it.W0, it.scale_factor = 1, 20, 30, 20, 30, 1
    assert hip_lib.dsm_selfsup_workspace_floats(items, 2) == 2 * (1 * 2 * 2 * 8 + 5 * 20 * 30)
    ws = ctypes.c_void_p(16)
    assert hip_lib.dsm_selfsup_fwd(None, 2, 0, ws, ws, ws, None) == -1
    assert hip_lib.dsm_selfsup_fwd(items, 1, 0, ws, ws, ws, None) == -1          # odd item count
    assert hip_lib.dsm_selfsup_fwd(items, 2, 0, None, ws, ws, None) == -1        # no workspace
    items[1].w = 31
    assert hip_lib.dsm_selfsup_fwd(items, 2, 0, ws, ws, ws, None) == -1          # the views differ
    items[1].w, items[0].h = 30, 1
    assert hip_lib.dsm_selfsup_fwd(items, 2, 0, ws, ws, ws, None) == -1          # imwrap.py:48
    items[0].h = 20
    assert hip_lib.dsm_selfsup_bwd(items, 2, 0, ws, ws, ws, None) == -1          # no gradient buffers
