"""GPU: the confidence heads (csrc/soft_argmin.hip ``dsm_disp_confidence_fwd``; ``costvolume.soft_argmin_confidence``,
``PSMNet.head_cost`` / ``gcnet.head_cost``, ``postprocess.predict_confidence``) against tests/headconf_oracle.py.

Tolerances.  ``disp``: the project's bound for the soft-argmin, 1e-3 px, and 1e-4 px from ``cv.soft_argmin``
on the same input.  For ``peak``, ``pmax``, ``pwin`` and ``entropy`` no number is fixed in advance: the
yardstick is float32 torch on the CPU (``F.interpolate`` -> ``softmax`` -> the sums of the definition, the
window centred on the oracle's arg-max), whose max abs error E_ref against the float64 oracle is measured
per map and per case, and the kernel gets 4 * E_ref -- it uses v_exp_f32 (1-2 ulp), rescales its sums a few
times and sums in another order.  E_ref is floored at half a float32 ulp of the map's largest magnitude:
the kernel stores float32, and a yardstick that happens to hit the float64 value exactly says nothing
about what float32 can hold.  Both errors are printed (run with -s).

``peak``, ``pmax`` and ``pwin`` depend on the arg-max bin d*.  They are compared at every pixel except those
where the oracle's second-largest DISTINCT fine value lies within 1e-3 of the largest: there float32 may
legitimately pick the other bin.  At most 2 % of a case's pixels may be left out this way (a condition: the
test fails if more are).  Exact end ties are not left out: the tie rule covers them.

Measured on an MI355X, radius 4 (E_ref of float32 torch | the kernel's error), the largest over the cases:
see profiles/headconf.md."""
import functools
import itertools
import math
import os

import numpy as np
import pytest
import torch

from tests import headconf_oracle as HO
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

GAP = 1e-3
WINDOW_MAPS = ("peak", "pmax", "pwin")


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


@functools.lru_cache(maxsize=None)
def case_values(name):
    _, osize, negate, align, _ = HO.CASES[name]
    return HO.fine_values(HO.case_cost(name), osize, negate, align)


def reference(cost, osize, negate, align, radius, values=None):
    """(oracle maps, keep mask, E_ref per map) of one input; computed on the CPU."""
    v = HO.fine_values(cost, osize, negate, align) if values is None else values
    ref = HO.from_values(v, radius)
    keep = ref["gap"] > GAP
    yard = HO.torch_heads(cost, osize, negate, align, radius, dstar=ref["dstar"])
    e_ref = {}
    for k in HO.MAPS:
        sel = keep if k in WINDOW_MAPS else np.ones_like(keep)
        err = np.abs(yard[k] - ref[k])[sel].max() if sel.any() else 0.0
        e_ref[k] = max(err, 2.0 ** -24 * np.abs(ref[k]).max())
    return ref, keep, e_ref


@functools.lru_cache(maxsize=None)
def case_reference(name, radius):
    _, osize, negate, align, _ = HO.CASES[name]
    return reference(HO.case_cost(name), osize, negate, align, radius, case_values(name))


def check(tag, got, ref, keep, e_ref, maps=HO.MAPS):
    """``got``: a DispConfidence on the device."""
    left_out = 1.0 - keep.mean()
    assert left_out <= 0.02, "%s: %.2f %% of the pixels have a near-tie at the top" % (tag, 100 * left_out)
    worst = {}
    for k in maps:
        g = getattr(got, k).cpu().double().numpy()
        assert g.shape == ref[k].shape and np.isfinite(g).all(), (tag, k)
        sel = keep if k in WINDOW_MAPS else np.ones_like(keep)
        worst[k] = np.abs(g - ref[k])[sel].max()
    print("%-34s left out %.2f %% | " % (tag, 100 * left_out) +
          "  ".join("%s %.2e (ref %.2e)" % (k, worst[k], e_ref[k]) for k in maps))
    for k in maps:
        bound = 1e-3 if k == "disp" else 4.0 * e_ref[k]
        assert worst[k] <= bound, "%s: %s off by %.3e > %.3e" % (tag, k, worst[k], bound)
    return worst


def radii(name):
    return (0, 1, 4, case_values(name).shape[1])


# ---------------------------------------------------------------------------------------------------
# parity on the seeded cases
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HO.CASES))
def test_parity_with_the_oracle(cv, name):
    _, osize, negate, align, _ = HO.CASES[name]
    cost = HO.case_cost(name).cuda()
    plain = cv.soft_argmin(cost, osize, negate=negate, align_corners=align)
    for r in radii(name):
        got = cv.soft_argmin_confidence(cost, osize, negate=negate, align_corners=align, radius=r)
        ref, keep, e_ref = case_reference(name, r)
        check("%s r=%d" % (name, r), got, ref, keep, e_ref)
        assert (got.disp - plain).abs().max().item() <= 1e-4
        assert got.entropy.min().item() >= 0.0 and got.entropy.max().item() <= math.log(case_values(name).shape[1]) + 1e-6
        assert got.pwin.max().item() <= 1.0 and got.pmax.min().item() > 0.0


@pytest.mark.parametrize("name", ["up4_empty_seg", "interp_align", "gc_ds4"])
def test_whole_range_window_is_the_expectation(cv, name):
    _, osize, negate, align, _ = HO.CASES[name]
    D = case_values(name).shape[1]
    cost = HO.case_cost(name).cuda()
    _, _, e_ref = case_reference(name, D)
    for r in (D - 1, D, 2 ** 31 - 1):
        got = cv.soft_argmin_confidence(cost, osize, negate=negate, align_corners=align, radius=r)
        assert (got.pwin - 1.0).abs().max().item() <= 4.0 * e_ref["pwin"]
        assert (got.peak - got.disp).abs().max().item() <= 4.0 * e_ref["peak"]


@pytest.mark.parametrize("name", ["up4_d192", "interp_ratio", "gc_ds2"])
def test_a_shifted_cost_gives_the_same_maps(cv, name):
    _, osize, negate, align, _ = HO.CASES[name]
    cost = HO.case_cost(name).cuda() + 3.0
    got = cv.soft_argmin_confidence(cost, osize, negate=negate, align_corners=align, radius=4)
    ref, keep, e_ref = case_reference(name, 4)           # the unshifted input's oracle and tolerances
    check(name + " +3.0", got, ref, keep, e_ref)


# ---------------------------------------------------------------------------------------------------
# hand-built costs: against the oracle and against what they must be
# ---------------------------------------------------------------------------------------------------
def run(cv, cost, osize, radius, negate=False, align=False):
    got = cv.soft_argmin_confidence(cost.cuda(), osize, negate=negate, align_corners=align, radius=radius)
    ref, keep, e_ref = reference(cost, osize, negate, align, radius)
    return got, ref, keep, e_ref


@pytest.mark.parametrize("cshape,osize", [((2, 6, 3, 18), (24, 12, 72)), ((1, 2, 3, 5), (8, 12, 20)),
                                          ((1, 10, 5, 70), None)])
def test_constant_cost(cv, cshape, osize):
    """The x4 head, the interpolating form and the GCNet form.  (All ratios are 4 and the constant has few
    bits, so every interpolation weight and product is exact and the fine values are equal bit for bit, in
    the oracle and in the kernel: d* = 0 by the lowest-index rule.)"""
    D = (osize or cshape[1:])[0]
    for r in (0, 3):
        got, ref, keep, e_ref = run(cv, torch.full(cshape, -1.75), osize, r)
        assert keep.all() and (ref["dstar"] == 0).all()
        check("constant %s r=%d" % (cshape, r), got, ref, keep, e_ref)
        assert (got.entropy - math.log(D)).abs().max().item() <= 4.0 * e_ref["entropy"]
        assert (got.pmax - 1.0 / D).abs().max().item() <= 4.0 * e_ref["pmax"]
        assert (got.pwin - (r + 1.0) / D).abs().max().item() <= 4.0 * e_ref["pwin"]
        assert (got.peak - r / 2.0).abs().max().item() <= 4.0 * e_ref["peak"]       # d* = 0: bins 0..r


@pytest.mark.parametrize("k,dstar", [(0, 0), (5, 22), (3, None)])
def test_one_dominant_coarse_plane(cv, k, dstar):
    """Dc = 6 -> D = 24.  k = 0: bins 0 and 1 are equal, d* = 0 and the window is clipped at the bottom;
    k = Dc - 1: bins D-2 and D-1 are equal BY THE TIE RULE, d* = D - 2 and the window is clipped at the
    top; an interior plane: d* is 4k+1 or 4k+2, whichever neighbour is larger."""
    g = torch.Generator().manual_seed(11)
    cost = 0.5 * torch.randn(2, 6, 3, 18, generator=g)
    cost[:, k] += 20.0
    for r in (0, 2, 4):
        got, ref, keep, e_ref = run(cv, cost, (24, 12, 70), r)
        check("dominant k=%d r=%d" % (k, r), got, ref, keep, e_ref)
        if dstar is not None:
            assert (ref["dstar"] == dstar).all()
            # the two equal end bins: each holds pmax, so a window of radius 0 holds exactly pmax
            if r == 0:
                assert (got.pwin - got.pmax).abs().max().item() <= 4.0 * e_ref["pwin"]
                assert (got.peak - float(dstar)).abs().max().item() <= 4.0 * e_ref["peak"]
        else:
            assert np.isin(ref["dstar"], (4 * k + 1, 4 * k + 2)).all()


def test_isolated_peaks_of_the_exact_fallback(cv):
    """The inputs of test_soft_argmin_up4_isolated_peaks_force_the_exact_fallback: peaks of height 300..3000
    leave every fine value more than the range of 2^x below the running maximum of the planes."""
    g = torch.Generator().manual_seed(5)
    for scale in (1.0, 300.0, 3000.0):
        cost = torch.randn(1, 1, 12, 9, 17, generator=g)
        peaks = torch.randint(0, 12, (9, 17), generator=g)
        cost[0, 0].scatter_(0, peaks.unsqueeze(0), scale * (1.0 + torch.rand(1, 9, 17, generator=g)))
        got, ref, keep, e_ref = run(cv, cost, (48, 36, 68), 4)
        check("isolated peaks x%g" % scale, got, ref, keep, e_ref)


def test_two_bumps_of_unequal_height(cv):
    """Two Gaussian bumps 12 coarse planes (48 bins) apart over a flat background: the expectation lands
    between them, the peak-window disparity stays within r of the higher one, and the window's mass says so."""
    k = torch.arange(48.0).view(1, 48, 1, 1)
    g = torch.Generator().manual_seed(3)
    cost = 6.0 * torch.exp(-0.5 * (k - 14.3) ** 2) + 5.3 * torch.exp(-0.5 * (k - 26.3) ** 2)
    cost = cost + 0.01 * torch.randn(1, 48, 2, 5, generator=g)
    hi, lo = 4 * 14.3 + 1.5, 4 * 26.3 + 1.5                    # the bumps' centres on the fine axis
    got, ref, keep, e_ref = run(cv, cost, (192, 8, 20), 4)
    check("two bumps", got, ref, keep, e_ref)
    assert (got.peak - hi).abs().max().item() <= 4.0
    assert got.disp.min().item() > hi + 4.0 and got.disp.max().item() < lo - 4.0
    assert got.pwin.max().item() < 0.9


# ---------------------------------------------------------------------------------------------------
# the Python op
# ---------------------------------------------------------------------------------------------------
def test_every_subset_of_want(cv):
    cost = HO.case_cost("up4_empty_seg").cuda()
    full = cv.soft_argmin_confidence(cost, (24, 12, 70))
    names = ("peak", "pmax", "pwin", "entropy")
    for n in range(len(names) + 1):
        for sub in itertools.combinations(names, n):
            got = cv.soft_argmin_confidence(cost, (24, 12, 70), want=sub)
            assert torch.equal(got.disp, full.disp)
            for k in names:
                if k in sub:
                    assert torch.equal(getattr(got, k), getattr(full, k)), (sub, k)
                else:
                    assert getattr(got, k) is None
    with pytest.raises(ValueError):
        cv.soft_argmin_confidence(cost, (24, 12, 70), want=("disp",))
    with pytest.raises(ValueError):
        cv.soft_argmin_confidence(cost, (24, 12, 70), radius=-1)


def test_five_dimensional_cost_and_grad_refusal(cv):
    cost = HO.case_cost("gc_ds4").cuda()
    a = cv.soft_argmin_confidence(cost, None, negate=True)
    b = cv.soft_argmin_confidence(cost.unsqueeze(1), None, negate=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    leaf = cost.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        cv.soft_argmin_confidence(leaf)
    with torch.no_grad():
        c = cv.soft_argmin_confidence(leaf, None, negate=True)
    assert all(not t.requires_grad for t in c) and torch.equal(c.disp, a.disp)


def test_a_view_with_a_storage_offset(cv):
    """A contiguous view one element into a larger buffer (a 4-byte-aligned pointer), and a non-contiguous
    one: ``_p`` / ``.contiguous()`` as in the siblings."""
    cost = HO.case_cost("up4_empty_seg")
    want = cv.soft_argmin_confidence(cost.cuda(), (24, 12, 70))
    buf = torch.zeros(cost.numel() + 1, device="cuda")
    buf[1:] = cost.flatten().cuda()
    view = buf[1:].view(cost.shape)
    assert view.storage_offset() == 1 and view.is_contiguous()
    strided = cost.cuda().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not strided.is_contiguous()
    for c in (view, strided):
        got = cv.soft_argmin_confidence(c, (24, 12, 70))
        for x, y in zip(got, want):
            assert torch.equal(x, y)


def test_replayed_graph_follows_its_input(cv):
    a, b = HO.case_cost("up4_empty_seg"), HO.case_cost("up4_empty_seg").flip(0) + 0.25
    static = a.cuda()
    step = lambda: cv.soft_argmin_confidence(static, (24, 12, 70))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    seen = []
    for inp in (b, a):
        static.copy_(inp)
        graph.replay()
        torch.cuda.synchronize()
        eager = cv.soft_argmin_confidence(inp.cuda(), (24, 12, 70))
        for x, y in zip(out, eager):
            assert torch.equal(x, y)
        seen.append(out.peak.cpu().clone())
    assert not torch.equal(seen[0], seen[1])


def test_launches_are_timed(cv):
    timer = cv.LaunchTimer()
    cv.set_timer(timer)
    try:
        cv.soft_argmin_confidence(HO.case_cost("up4_empty_seg").cuda(), (24, 12, 70))
        cv.soft_argmin_confidence(HO.case_cost("gc_ds2").cuda(), None, negate=True)
        torch.cuda.synchronize()
    finally:
        cv.set_timer(None)
    assert sorted(timer.summary()) == ["disp_confidence_kernel", "disp_confidence_up4_kernel"]


# ---------------------------------------------------------------------------------------------------
# the models and predict_confidence
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,size", [("psmnet", (256, 256)), ("gcnet", (32, 64))])
def test_predict_confidence_of_the_models(hip_lib, net, size):
    """Random weights, eval mode, maxdisp 16.  (PSMNet's SPP pools 64 x 64 at quarter resolution: 256 x 256 is
    the smallest pair it takes; its head costs are scaled into a trained network's range, see below.)
    ``disp`` is the model's own first map within 1e-4 px, all maps are finite and shaped like it, and
    ``forward`` gives the same bits before and after."""
    from dsmnet_amd import postprocess
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(1)
    model = model_create_by_name(net, 16).cuda().eval()
    if net == "psmnet":
        # He-normal weights under identity BatchNorm statistics let the activations grow through the 3-D
        # trunk: the head cost of the untouched random PSMNet has std 4.5e6 (|max| 2e7, where one float32
        # ulp is 2 -- more than the range a softmax resolves), and ``forward``'s own map is then 0.13 px
        # from the float64 soft-argmin of that cost (the confidence kernel 1.1e-3 px).  A trained network's
        # cost is O(10).  The three Cout = 1 head convolutions are linear and bias-free, so scaling their
        # random weights by 1e-6 scales the cost into that regime (std 4.5) and nothing else.
        with torch.no_grad():
            for head in (model.classif1, model.classif2, model.classif3):
                for m in head.modules():
                    if isinstance(m, torch.nn.Conv3d) and m.out_channels == 1:
                        m.weight.mul_(1e-6)
    g = torch.Generator().manual_seed(2)
    imL, imR = (torch.rand(1, 3, *size, generator=g).cuda() for _ in range(2))
    with torch.no_grad():
        before = model(imL, imR)[1][0].clone()
    res = postprocess.predict_confidence(model, imL, imR, radius=2)
    with torch.no_grad():
        after = model(imL, imR)[1][0]
    assert torch.equal(before, after)
    assert sorted(res) == sorted(HO.MAPS)
    for k, t in res.items():
        assert t.shape == before.shape and torch.isfinite(t).all(), k
        assert not t.requires_grad
    assert (res["disp"] - before).abs().max().item() <= 1e-4
    D = 16                                               # gcnet: maxdisparity // 2 planes, doubled by l37
    assert res["entropy"].max().item() <= math.log(D) + 1e-6 and res["pwin"].max().item() <= 1.0
    assert (res["peak"] - res["disp"]).abs().max().item() <= D


# ---------------------------------------------------------------------------------------------------
# cv.soft_argmin itself is untouched
# ---------------------------------------------------------------------------------------------------
def test_soft_argmin_is_bit_identical_to_the_parent_build(cv):
    """Outputs of ``cv.soft_argmin`` captured on an MI355X from the build BEFORE the confidence kernels were
    added to csrc/soft_argmin.hip: the existing kernels' code generation must not have moved."""
    z = np.load(os.path.join(GOLDEN, "golden_headconf_soft_argmin.npz"), allow_pickle=False)
    for key, name in (("up4_2x6x3x18", "up4_empty_seg"), ("gc_2x10x5x70", "gc_ds4"), ("interp_2x5x4x9", "interp_align")):
        _, osize, negate, align, _ = HO.CASES[name]
        got = cv.soft_argmin(HO.case_cost(name).cuda(), osize, negate=negate, align_corners=align)
        assert np.array_equal(got.cpu().numpy(), z[key]), name


# ---------------------------------------------------------------------------------------------------
# deploy
# ---------------------------------------------------------------------------------------------------
def test_cli_writes_the_confidence_map_and_the_peak_disparity(hip_lib, tmp_path, capsys):
    """``deploy --confidence [--conf_threshold t --path_disp_gt gt]`` and ``--peak`` on a small random GCNet:
    the disparity equals ``disp_predict``'s within 1e-4 px, ``<stem>_conf.png`` is ``pwin`` as 8-bit gray,
    the thresholded metrics line is printed, and ``--peak`` writes ``predict_confidence``'s peak map."""
    from dsmnet_amd import deploy, img_rw, postprocess
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(4)
    model = model_create_by_name("gcnet", 16)
    w = str(tmp_path / "w.pkl")
    torch.save({"state_dict": model.state_dict()}, w)
    rng = np.random.RandomState(6)
    imgL, imgR = (rng.randint(0, 256, (32, 64, 3)).astype(np.uint8) for _ in range(2))
    pl, pr, gt = str(tmp_path / "L.png"), str(tmp_path / "R.png"), str(tmp_path / "gt.pfm")
    img_rw.imwrite(pl, imgL)
    img_rw.imwrite(pr, imgR)
    img_rw.save_pfm(gt, (1.0 + 6.0 * rng.rand(32, 64)).astype(np.float32))
    common = ["--net", "gcnet", "--maxdisparity", "16", "--path_weight", w, "--path_left", pl, "--path_right", pr]
    model = model.cuda().eval()
    plain = deploy.disp_predict(model, imgL, imgR)
    maps = deploy.conf_predict(model, imgL, imgR, radius=2)
    assert sorted(maps) == sorted(HO.MAPS) and all(v.shape == (32, 64) for v in maps.values())

    out = str(tmp_path / "d.pfm")
    assert deploy.main(common + ["--out", out, "--confidence", "--conf_radius", "2", "--conf_threshold", "0.5",
                                 "--path_disp_gt", gt]) == out
    d = np.asarray(img_rw.load_disp(out), dtype=np.float32)
    assert d.shape == (32, 64) and np.abs(d - plain).max() <= 1e-4
    gray = np.asarray(img_rw.imread(str(tmp_path / "d_conf.png")))
    gray = gray[..., 0] if gray.ndim == 3 else gray
    assert gray.shape == (32, 64)
    assert np.array_equal(gray, np.rint(np.clip(maps["pwin"], 0.0, 1.0) * 255.0).astype(np.uint8))
    printed = capsys.readouterr().out
    assert "confident pixels (pwin >= 0.5, %.2f %%)" % (100.0 * (maps["pwin"] >= 0.5).mean()) in printed

    out2 = str(tmp_path / "p.pfm")
    assert deploy.main(common + ["--out", out2, "--peak", "--conf_radius", "2"]) == out2
    assert np.abs(np.asarray(img_rw.load_disp(out2), dtype=np.float32) - maps["peak"]).max() <= 1e-6
    with pytest.raises(SystemExit, match="regresses disparity directly"):
        sd = str(tmp_path / "c.pkl")
        torch.save({"state_dict": model_create_by_name("dispnetcorr", 16).state_dict()}, sd)
        deploy.main(["--net", "dispnetcorr", "--maxdisparity", "16", "--path_weight", sd, "--path_left", pl,
                     "--path_right", pr, "--out", str(tmp_path / "x.pfm"), "--confidence"])
