"""CPU: the C ABI of the fused supervised pyramid loss (struct size, argument checks, workspace
size; no kernel is launched), the op's refusal of CPU tensors, and the untouched stock path of
``train.losses("supervised")`` on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

from oracle import train as OT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _items(n, B=1, hc=20, wc=70, level=0):
    from dsmnet_amd import _lib
    items = (_lib.SuplossItem * max(n, 1))()
    for it in items:
        it.pred = 16
        it.B, it.hc, it.wc, it.level, it.weight = B, hc, wc, level, 1.0
    return items


def test_item_size_is_the_headers():
    from dsmnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "dsmnet_hip.h")).read()
    stated = int(re.search(r"sizeof\(dsm_suploss_item\) == (\d+)", header).group(1))
    assert ctypes.sizeof(_lib.SuplossItem) == stated == 48
    assert int(re.search(r"#define DSM_SUPLOSS_MAX_ITEMS (\d+)", header).group(1)) == _lib.DSM_SUPLOSS_MAX_ITEMS == 16


def test_argument_checks_return_codes(hip_lib):
    ws = ctypes.c_void_p(16)
    items = _items(17)
    ok = (20, 70, 1, 1, ws, ws, ws, None)
    assert hip_lib.dsm_suploss_fwd(None, 1, ws, *ok) == -1                        # no items
    assert hip_lib.dsm_suploss_fwd(items, 1, None, *ok) == -1                     # no ground truth
    assert hip_lib.dsm_suploss_fwd(items, 1, ws, 20, 70, 1, 1, None, ws, ws, None) == -1   # no workspace
    assert hip_lib.dsm_suploss_fwd(items, 1, ws, 20, 70, 1, 1, ws, None, ws, None) == -1   # no loss
    assert hip_lib.dsm_suploss_fwd(items, 0, ws, *ok) == -1
    assert hip_lib.dsm_suploss_fwd(items, 17, ws, *ok) == -1
    assert hip_lib.dsm_suploss_fwd(items, 1, ws, 0, 70, 1, 1, ws, ws, ws, None) == -1      # H = 0
    assert hip_lib.dsm_suploss_bwd(None, 1, ws, 20, 70, 1, ws, ws, ws, None) == -1
    assert hip_lib.dsm_suploss_bwd(items, 1, None, 20, 70, 1, ws, ws, ws, None) == -1
    assert hip_lib.dsm_suploss_bwd(items, 1, ws, 20, 70, 1, None, ws, ws, None) == -1
    assert hip_lib.dsm_suploss_bwd(items, 0, ws, 20, 70, 1, ws, ws, ws, None) == -1
    assert hip_lib.dsm_suploss_bwd(items, 17, ws, 20, 70, 1, ws, ws, ws, None) == -1
    items[0].hc = 0
    assert hip_lib.dsm_suploss_fwd(items, 1, ws, *ok) == -1                       # non-positive size
    items[0].hc, items[1].B = 20, 2
    assert hip_lib.dsm_suploss_fwd(items, 2, ws, *ok) == -1                       # batch sizes differ
    # the upsampled map would not cover gt (the reference's crop comes out smaller): unsupported
    small = _items(1, hc=5, wc=35, level=1)
    assert hip_lib.dsm_suploss_fwd(small, 1, ws, *ok) == -2
    small[0].hc = 10
    assert hip_lib.dsm_suploss_fwd(small, 1, ws, 20, 71, 1, 1, ws, ws, ws, None) == -2


def test_workspace_floats(hip_lib):
    # gt (1,1,20,70): 2 x 2 tiles of 16 x 64, four partial sums each; 1400 saved floats per item
    assert hip_lib.dsm_suploss_workspace_floats(2, 1, 20, 70, 1) == 2 * (4 * 4 + 20 * 70) == 2832
    assert hip_lib.dsm_suploss_workspace_floats(2, 1, 20, 70, 0) == 32
    assert hip_lib.dsm_suploss_workspace_floats(3, 2, 16, 64, 1) == 3 * (2 * 4 + 2 * 16 * 64)
    assert hip_lib.dsm_suploss_workspace_floats(0, 1, 20, 70, 1) == 0
    assert hip_lib.dsm_suploss_workspace_floats(17, 1, 20, 70, 1) == 0


def test_cpu_tensors_have_no_fallback():
    from dsmnet_amd import costvolume as cv
    gt, d = torch.rand(1, 1, 8, 12), torch.rand(1, 1, 8, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.supervised_pyramid_loss(gt, [d], [0], [1.0])


def test_option_follows_the_options_interface():
    from dsmnet_amd import costvolume as cv
    assert cv.get_option("fused_supervised_loss") in (True, False)
    old = cv.set_option("fused_supervised_loss", False)
    try:
        assert cv.get_option("fused_supervised_loss") is False
    finally:
        cv.set_option("fused_supervised_loss", old)
    assert cv.get_option("fused_supervised_loss") == old


def test_cpu_pyramid_keeps_the_stock_path():
    """CPU tensors never reach the fused op: a 7-level pyramid still equals the oracle, with
    gradients, and no metrics are stored."""
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd import train
    cv.get_option("fused_supervised_loss")       # the option exists; CPU tensors never look at it
    g = torch.Generator().manual_seed(5)
    H, W = 72, 136
    gt = torch.rand(2, 1, H, W, generator=g) * 40 - 8
    disps = [(torch.rand(2, 1, 128 >> k, 192 >> k, generator=g) * 40).requires_grad_() for k in range(7)]
    disps[0] = disps[0].detach()[:, :, :H, :W].clone().requires_grad_()
    lf = train.losses("supervised", 7, 37)
    lf.Weight_Adjust_levels(10)
    got = lf({"disp_gt": gt, "disps": disps, "scale_disps": list(range(7)), "flag_smooth": True})
    want = OT.losses_pyramid0(lf.weight_levels, gt, [d.detach() for d in disps], list(range(7)), True)
    assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want))
    assert lf.last_metrics is None
    got.backward()
    assert all(d.grad is not None and torch.isfinite(d.grad).all() for d in disps)
