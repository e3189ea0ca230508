"""GPU: iResNet and DispNetC trained through the fused warp and decoder levels (options ``warp_train`` and
``decoder_train``) against the same models with both options off, at one pair of 64 x 128 (iResNet's ``pr6`` is
then 1 x 2: the ``Hp = 1`` edge of the upsampling's adjoint inside a model).

This is a wiring test: a wrong sign, a dropped term or an un-zeroed buffer moves a parameter gradient by O(1) of
its maximum.  The bound is 1e-3 of each gradient's maximum and no tighter because one ``floorf`` that falls on
the other side in the two fp32 warps moves a parameter gradient by about 1 / (H W) = 1.2e-4; precision is
what tests/test_warp_bwd_gpu.py and tests/test_decoder_bwd_gpu.py measure."""
import pytest
import torch

from tests.helpers import seeded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


def run(cv, model, imL, imR, cots, on):
    old = (cv.set_option("warp_train", on), cv.set_option("decoder_train", on))
    timer = cv.LaunchTimer()
    cv.set_timer(timer)
    try:
        model.zero_grad(set_to_none=True)
        torch.manual_seed(5)                         # iResNet's warp draws its epsilon from the global generator
        with torch.enable_grad():
            outs = model(imL, imR)[1]
            if cots is None:
                cots = [seeded(70 + i, *o.shape).cuda() for i, o in enumerate(outs)]
            sum((o * c).sum() for o, c in zip(outs, cots)).backward()
    finally:
        cv.set_timer(None)
        cv.set_option("warp_train", old[0])
        cv.set_option("decoder_train", old[1])
    torch.cuda.synchronize()
    launches = {k: v["launches"] for k, v in timer.summary().items()}
    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    return [o.detach() for o in outs], grads, launches, cots


@pytest.mark.parametrize("name,warps,levels", [("iresnet", 1, 8), ("dispnetcorr", 0, 5)])
def test_options_on_against_off(cv, name, warps, levels):
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(11)
    model = model_create_by_name(name, 192).cuda()
    imL, imR = seeded(21, 1, 3, 64, 128).cuda(), seeded(22, 1, 3, 64, 128).cuda()
    o_off, g_off, l_off, cots = run(cv, model, imL, imR, None, False)
    o_on, g_on, l_on, _ = run(cv, model, imL, imR, cots, True)
    assert l_off.get("warp_abs_error_bwd_kernel", 0) == 0 and l_off.get("decoder_cat_bwd_kernel", 0) == 0, l_off
    assert l_off.get("warp_abs_error_kernel", 0) == 0 and l_off.get("decoder_cat_kernel", 0) == 0, l_off
    assert l_on.get("warp_abs_error_bwd_kernel", 0) == warps and l_on.get("warp_abs_error_kernel", 0) == warps, l_on
    assert l_on.get("decoder_cat_bwd_kernel", 0) == levels and l_on.get("decoder_cat_kernel", 0) == levels, l_on
    worst_out = max((a - b).abs().max().item() for a, b in zip(o_on, o_off))
    worst = max(((g_on[n] - g_off[n]).abs().max().item() / max(g_off[n].abs().max().item(), 1e-30), n) for n in g_off)
    print("%s: outputs differ by %.3e, worst parameter gradient %.3e of its maximum (%s)"
          % ((name, worst_out) + worst))
    assert len(g_off) == len(list(model.parameters())) and all(bool(torch.isfinite(g).all()) for g in g_on.values())
    assert worst_out <= 2e-5
    for n in g_off:
        assert (g_on[n] - g_off[n]).abs().max().item() <= 1e-3 * g_off[n].abs().max().item(), n


def test_two_refinement_iterations_launch_the_warp_backward_twice(cv):
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(11)
    model = model_create_by_name("iresnet", 192).cuda()
    imL, imR = seeded(21, 1, 3, 64, 128).cuda(), seeded(22, 1, 3, 64, 128).cuda()
    old = (cv.set_option("warp_train", True), cv.set_option("decoder_train", True))
    timer = cv.LaunchTimer()
    cv.set_timer(timer)
    try:
        with torch.enable_grad():
            sum(o.sum() for o in model(imL, imR, iter=2)[1]).backward()
    finally:
        cv.set_timer(None)
        cv.set_option("warp_train", old[0])
        cv.set_option("decoder_train", old[1])
    torch.cuda.synchronize()
    s = timer.summary()
    assert s["warp_abs_error_bwd_kernel"]["launches"] == 2 and s["decoder_cat_bwd_kernel"]["launches"] == 6 + 2 * 2
