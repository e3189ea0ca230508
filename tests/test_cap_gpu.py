"""Cap[_ds][_lr][-mask] objective on the GPU (the Cap rule of csrc/selfsup.hip): the fused op
against the float64 restatement (tests/cap_oracle.py) run on the same device with the same
epsilons, the whole pyramid against the reference fixture, launch counts, bit-reproducibility of
the gather-only backward, and the training / validation steps.

Tolerances are those of tests/test_selfsup_gpu.py, for the reasons at the top of that file: loss
1e-5 relative; gradients by its ``_grad_close`` (at most 0.2 % outliers, 2e-4 relative L2 on the
rest).  The no-lr cases have no atomic sum, so nothing here needs more.

Cases with low-contrast images exist because random full-contrast images keep simlary below 0.75
and w at its floor of 0.001: only where w = (simlary - 0.75) / 2 + 0.001 leaves the floor does the
Cap arithmetic (w from the masked mean, w / ds_divisor in the loss) show in the loss.  There w
amplifies simlary's error by simlary / (2 w), which is why the Cap work list takes torch's own fp32
Gaussian taps (csrc/selfsup.hip make_work).  The bound stays 1e-5 everywhere.
"""
import numpy as np
import pytest
import torch

from tests import cap_oracle as CO
from tests import selfsup_oracle as SO
from tests.test_selfsup_gpu import _grad_close, _selfsup_batch, _smooth

pytestmark = pytest.mark.gpu


def _inputs(B, h, w, nedge, levels, seed, dlo, dhi, contrast=1.0):
    """CPU tensors (so that a seed's properties can be checked without a GPU): the image pair and
    its flip, one disparity pair per level, the four epsilons per level.  ``contrast`` < 1 shrinks
    the images towards 0.5: with sigma well below sqrt(C2) = 0.03 the SSIM of two unrelated images
    is near 1 wherever the sample is valid (and near 0 where it is not), so simlary exceeds 0.75
    and w leaves its floor of 0.001 -- random full-contrast images never get there."""
    g = torch.Generator().manual_seed(seed)
    H0, W0 = h + 2 * nedge, w + 2 * nedge
    full = _smooth(g, B, 6, H0, W0, 0.0, 1.0, 6) + 0.05 * torch.rand(B, 6, H0, W0, generator=g)
    full = 0.5 + contrast * (full - 0.5)
    dLs, dL1s = [], []
    for k in levels:
        hk, wk = -(-h // 2 ** k), -(-w // 2 ** k)
        dLs.append(_smooth(g, B, 1, hk, wk, dlo, dhi, 4) / 2 ** k)
        dL1s.append(_smooth(g, B, 1, hk, wk, dlo, dhi, 4) / 2 ** k)
    torch.manual_seed(seed)
    delts = [tuple(SO.draw_delt() for _ in range(4)) for _ in levels]
    return full, dLs, dL1s, delts


def _views(full, h, w, nedge):
    full1 = torch.flip(full, dims=[-1])
    return (full[:, :3, nedge:nedge + h, nedge:nedge + w], full[:, 3:6],
            full1[:, 3:6, nedge:nedge + h, nedge:nedge + w], full1[:, :3])


def _oracle(views, lt, dLs, dL1s, levels, weights, factors, divisors, mask, terms, delts, stats=None, bands=None):
    """The fused op's contract in float64 on the tensors' device (entry by entry)."""
    d = lambda t: t.detach().double()
    imL, imR_src, imL1, imR1_src = map(d, views)
    dLs = [d(x).requires_grad_() for x in dLs]
    dL1s = [d(x).requires_grad_() for x in dL1s]
    loss = 0
    for p, (k, wt, sf, dv, dl) in enumerate(zip(levels, weights, factors, divisors, delts)):
        dL, dL1 = dLs[p], dL1s[p]
        im, im1 = imL[:, :, ::2 ** k, ::2 ** k], imL1[:, :, ::2 ** k, ::2 ** k]
        w0 = SO.imwrap_bchw(imR_src, dL, dl[0], False, lt, sf)
        w1 = SO.imwrap_bchw(imR1_src, dL1, dl[1], False, lt, sf)
        dw = SO.imwrap_bchw(dL1, dL, dl[2], True, (0, 0), 1)
        dw1 = SO.imwrap_bchw(dL, dL1, dl[3], True, (0, 0), 1)
        wc = SO.weight_common(dL, dw, sf) if mask else None
        wc1 = SO.weight_common(dL1, dw1, sf) if mask else None
        if bands is not None:
            bands.append((dL - dw).abs().detach() / sf)
        loss = loss + (CO.loss_cap_ds_lr(im, w0, dL, dw, dv, wc, terms, stats) +
                       CO.loss_cap_ds_lr(im1, w1, dL1, dw1, dv, wc1, terms, stats)) * wt
    loss.backward()
    return loss.detach(), [x.grad for x in dLs], [x.grad for x in dL1s]


def _case(B, h, w, nedge, levels, mask, terms, seed, dlo, dhi, divisors=None, factors=None, contrast=1.0):
    from dsmnet_amd import costvolume as cv
    full, dLs, dL1s, delts = _inputs(B, h, w, nedge, levels, seed, dlo, dhi, contrast)
    views = _views(full.cuda(), h, w, nedge)
    dLs = [x.cuda().requires_grad_() for x in dLs]
    dL1s = [x.cuda().requires_grad_() for x in dL1s]
    weights = [1.0 / (p + 1) for p in range(len(levels))]
    factors = factors or [2 ** k for k in levels]
    divisors = divisors or [1] * len(levels)
    lt = (nedge, nedge)
    loss, aux = cv.selfsup_pyramid_loss(views[0], views[1], lt, dLs, views[2], views[3], lt, dL1s, levels, weights,
                                        factors, mask, delts, return_aux=True, objective="cap", terms=terms,
                                        ds_divisors=divisors)
    loss.backward()
    stats, bands = [], []
    want, gL, gL1 = _oracle(views, lt, dLs, dL1s, levels, weights, factors, divisors, mask, terms, delts, stats, bands)
    torch.cuda.synchronize()
    grads = [x.grad for x in dLs] + [x.grad for x in dL1s]
    rel = abs(float(loss.detach()) - float(want)) / abs(float(want))
    print("cap%s B%d %dx%d nedge %d levels %s mask %s contrast %g: loss %.6f vs %.6f rel %.2e, w %s" % (
        list(terms), B, h, w, nedge, levels, mask, contrast, float(loss.detach()), float(want), rel,
        ["%.4f" % float(s[0]) for s in stats]))
    assert all(bool(torch.isfinite(x).all()) for x in grads) and bool(torch.isfinite(loss))
    assert rel <= 1e-5
    _grad_close(grads, gL + gL1, "cap case seed %d" % seed)
    return {"loss": loss.detach(), "want": want, "aux": aux.cpu(), "grads": grads, "stats": stats, "bands": bands,
            "args": (views, lt, dLs, dL1s, levels, weights, factors, mask, delts)}


def test_cap_ds_one_level_no_mask(hip_lib):
    """The gather-only backward with the disparity warp skipped."""
    _case(1, 48, 80, 0, [0], False, ("ds",), 1, 1.0, 9.0)


def test_cap_ds_mask_ragged_batch3_divisor_is_not_the_scale_factor(hip_lib):
    kw = dict(factors=[1, 2, 4])
    a = _case(3, 37, 101, 0, [0, 1, 2], True, ("ds",), 4, 1.0, 12.0, divisors=[1, 2, 16], **kw)
    delta = torch.cat([b.flatten() for b in a["bands"]])
    for lo, hi in ((0, 1), (1, 3), (3, 1e9)):
        frac = ((delta >= lo) & (delta < hi)).double().mean().item()
        assert frac >= 0.05, (lo, hi, frac)
    # Changing only the last divisor (w/16 against w/4) on these very inputs.  w is at its floor
    # of 0.001 here, so the loss moves by only 4e-5 of itself -- but the two runs share every
    # rounding except the last entry's smoothness term in the fp64 reduction, and the loss comes
    # back as fp32 (ulp 6e-8 at 0.92), so the difference is resolved to well under 1 % of itself
    b = _case(3, 37, 101, 0, [0, 1, 2], True, ("ds",), 4, 1.0, 12.0, divisors=[1, 2, 4], **kw)
    _divisor_moved_the_loss(a, b)
    # and where w has left its floor (~0.03 at level 0): the loss moves by 1e-3 of itself
    c = _case(3, 37, 101, 0, [0, 1, 2], True, ("ds",), 4, 1.0, 12.0, divisors=[1, 2, 16], contrast=0.05, **kw)
    d = _case(3, 37, 101, 0, [0, 1, 2], True, ("ds",), 4, 1.0, 12.0, divisors=[1, 2, 4], contrast=0.05, **kw)
    assert all(float(st[0]) > 0.001 for st in c["stats"])
    _divisor_moved_the_loss(c, d)


def _divisor_moved_the_loss(a, b):
    want = float(b["want"]) - float(a["want"])
    got = float(b["loss"]) - float(a["loss"])
    print("last divisor 16 -> 4: loss moves by %.4e (oracle %.4e)" % (got, want))
    assert want > 0 and abs(got - want) <= 0.01 * want


def test_cap_ds_mask_nedge64_scale_factors_1_2_4(hip_lib):
    _case(1, 64, 96, 64, [0, 1, 2], True, ("ds",), 3, 2.0, 14.0, divisors=[1, 2, 4])


def test_cap_mask_without_the_smoothness_term(hip_lib):
    a = _case(2, 40, 96, 0, [0, 1], True, (), 9, 1.0, 12.0)
    b = _case(2, 40, 96, 0, [0, 1], True, ("ds",), 9, 1.0, 12.0)
    assert float(b["loss"]) > float(a["loss"])


@pytest.mark.parametrize("mask", [True, False])
def test_cap_ds_lr_runs_the_scatter_path(hip_lib, mask):
    _case(2, 40, 96, 0, [0], mask, ("ds", "lr"), 5, 2.0, 20.0, divisors=[2])


def _depthmono(a):
    """aux of the depthmono rule on the inputs of case ``a``, and the restatement's (w, fallback,
    simlary) per view."""
    from dsmnet_amd import costvolume as cv
    views, lt, dLs, dL1s, levels, weights, factors, mask, delts = a["args"]
    _, aux = cv.selfsup_pyramid_loss(views[0], views[1], lt, dLs, views[2], views[3], lt, dL1s, levels, weights,
                                     factors, mask, delts, return_aux=True)
    d = lambda t: t.detach().double()
    stats, dl = [], delts[0]
    for im, src, dd, do, e_im, e_d in ((views[0], views[1], dLs[0], dL1s[0], dl[0], dl[2]),
                                       (views[2], views[3], dL1s[0], dLs[0], dl[1], dl[3])):
        iw = SO.imwrap_bchw(d(src), d(dd), e_im, False, lt, factors[0])
        dw = SO.imwrap_bchw(d(do), d(dd), e_d, True, (0, 0), 1)
        SO.loss_depthmono(d(im), iw, d(dd), dw, SO.weight_common(d(dd), dw, factors[0]), stats)
    return aux.cpu(), stats


def _check_w(a):
    """aux against the oracle: simlary to 1e-5 relative (an fp32 mean of fp32 SSIM values, as the
    loss), and w = max(0, simlary - 0.75) / 2 + 0.001 therefore to half of that, absolute."""
    for v, (w, n_valid, simlary) in enumerate(a["stats"]):
        got_w, got_s = float(a["aux"][v, 0]), float(a["aux"][v, 3])
        print("view %d: valid %d of 960, simlary %.7f vs %.7f, w %.7f vs %.7f" % (
            v, int(n_valid), got_s, float(simlary), got_w, float(w)))
        assert abs(got_s - float(simlary)) <= 1e-5 * float(simlary)
        assert abs(got_w - float(w)) <= 0.5e-5 * float(simlary) + 1e-7


def _valid_on_the_cpu(seed, dlo, dhi, contrast=1.0):
    """Valid pixels per view of the 24x40 case, by the restatement on the CPU."""
    full, dLs, dL1s, delts = _inputs(1, 24, 40, 0, [0], seed, dlo, dhi, contrast)
    stats = []
    _oracle(_views(full, 24, 40, 0), (0, 0), dLs, dL1s, [0], [1.0], [1], [1], True, ("ds",), delts, stats)
    return [int(st[1]) for st in stats]


def test_no_fallback_below_1024_valid_pixels(hip_lib):
    """24 x 40 = 960 pixels per view, disparities 0.5..30 (a third of the samples fall outside):
    depthmono falls back to every pixel, Cap keeps the masked mean, and w is the restatement's.
    With these inputs both means are below 0.75 (with random images the masked one is for every
    seed: the 11-tap window drags the SSIM down next to the invalid region), so w is 0.001 under
    both rules -- asserted, so that it is seen should that ever change -- and what differs for
    the same inputs is simlary; the next test has inputs where w itself differs."""
    assert all(0 < n <= 0.9 * 960 for n in _valid_on_the_cpu(6, 0.5, 30.0))    # at least 10 % invalid
    a = _case(1, 24, 40, 0, [0], True, ("ds",), 6, 0.5, 30.0)
    assert a["aux"][:, 1].tolist() == [0.0, 0.0]
    _check_w(a)
    dm, dm_stats = _depthmono(a)
    assert dm[:, 1].tolist() == [1.0, 1.0]
    for v in range(2):
        sim_cap, sim_dm = float(a["stats"][v][2]), float(dm_stats[v][2])
        assert float(a["stats"][v][0]) == 0.001 == float(dm_stats[v][0])
        assert bool(dm_stats[v][1]) and abs(float(dm[v, 3]) - sim_dm) <= 1e-5 * sim_dm
        assert abs(sim_cap - sim_dm) > 100 * 1e-5 * sim_cap              # the rules differ far beyond the tolerance
        assert abs(float(a["aux"][v, 3]) - float(dm[v, 3])) > 0.9 * abs(sim_cap - sim_dm)


def test_no_fallback_changes_w(hip_lib):
    """The same 960 pixels, disparities 4..12 (a fifth invalid) and low-contrast images: the masked
    mean is ~0.80, the mean over every pixel ~0.63, so Cap's w is ~0.025 where depthmono's is 0.001
    (the reference's own lines give the same on the fixture's "lowcontrast" case)."""
    assert all(0 < n <= 0.9 * 960 for n in _valid_on_the_cpu(6, 4.0, 12.0, 0.02))
    a = _case(1, 24, 40, 0, [0], True, ("ds",), 6, 4.0, 12.0, contrast=0.02)
    assert a["aux"][:, 1].tolist() == [0.0, 0.0]
    _check_w(a)
    dm, dm_stats = _depthmono(a)
    assert dm[:, 1].tolist() == [1.0, 1.0]
    for v in range(2):
        assert float(a["stats"][v][0]) > 0.015 and float(dm_stats[v][0]) == 0.001
        assert float(a["aux"][v, 0]) > 0.015 and float(dm[v, 0]) == float(np.float32(0.001)), (a["aux"][v], dm[v])


def test_zero_valid_pixels(hip_lib):
    """Every disparity larger than the source width: mask_ap selects nothing, w = 0.001 (what the
    reference's own lines give, tests/golden/golden_cap.npz "novalid"), nothing is NaN."""
    a = _case(1, 24, 40, 0, [0], True, ("ds",), 7, 50.0, 60.0)
    assert [int(s[1]) for s in a["stats"]] == [0, 0]
    assert a["aux"][:, 0].tolist() == [float(np.float32(0.001))] * 2
    assert a["aux"][:, 1].tolist() == [0.0, 0.0]
    assert bool(torch.isfinite(a["aux"][:, [0, 1, 2]]).all())


def _grads_of(args, divisors, poison=False):
    from dsmnet_amd import costvolume as cv
    views, lt, dLs, dL1s, levels, weights, factors, mask, delts = args
    for d in dLs + dL1s:
        d.grad = None
    loss = cv.selfsup_pyramid_loss(views[0], views[1], lt, dLs, views[2], views[3], lt, dL1s, levels, weights,
                                   factors, mask, delts, objective="cap", terms=("ds",), ds_divisors=divisors)
    if poison:
        # the op does not expose its gradient buffer: leave NaNs in the caching allocator's free
        # block of the same size, which the backward's torch.empty most likely gets (best effort)
        n = sum(d.numel() for d in dLs + dL1s)
        torch.cuda.synchronize()
        junk = torch.full((n,), float("nan"), device="cuda")
        torch.cuda.synchronize()
        poisoned = junk.data_ptr()
        del junk
    loss.backward()
    torch.cuda.synchronize()
    if poison:
        # should the backward have been given another block, the NaN one is still free and is the
        # best fit for this request: overwrite it, so that no NaN stays behind in device memory
        scrub = torch.zeros(n, device="cuda")
        torch.cuda.synchronize()
        print("the backward %s the poisoned block" % ("did not get" if scrub.data_ptr() == poisoned else "got"))
        del scrub
    return [d.grad.clone() for d in dLs + dL1s]


def test_gather_backward_is_bit_reproducible_and_fills_every_element(hip_lib):
    a = _case(3, 37, 101, 0, [0, 1, 2], True, ("ds",), 4, 1.0, 12.0, divisors=[1, 2, 16], factors=[1, 2, 4])
    g1 = _grads_of(a["args"], [1, 2, 16])
    g2 = _grads_of(a["args"], [1, 2, 16])
    g3 = _grads_of(a["args"], [1, 2, 16], poison=True)
    for x, y, z, first in zip(g1, g2, g3, a["grads"]):
        assert torch.equal(x, y) and torch.equal(x, first)
        assert bool(torch.isfinite(z).all()) and torch.equal(x, z)


def _launches(fn, monkeypatch):
    """Launch names as tests/test_suploss_gpu.py counts them (one "+"-joined name per entry into
    the library), and how often torch.zeros was called meanwhile (the fill launch; the kernel-level
    list is in profiles/cap.md)."""
    from dsmnet_amd import costvolume as cv
    names, fills = [], []

    class Timer(cv.LaunchTimer):
        def stop(self, name, start, work):
            names.append(name)
    real = torch.zeros

    def zeros(*a, **k):
        fills.append(a)
        return real(*a, **k)
    cv.set_timer(Timer())
    try:
        with monkeypatch.context() as m:
            m.setattr(torch, "zeros", zeros)
            fn()
            torch.cuda.synchronize()
    finally:
        cv.set_timer(None)
    return names, len(fills)


def test_launch_counts(hip_lib, monkeypatch):
    from dsmnet_amd import costvolume as cv
    full, dLs, dL1s, delts = _inputs(2, 40, 96, 0, [0, 1], 12, 1.0, 10.0)
    views = _views(full.cuda(), 40, 96, 0)
    dLs = [x.cuda().requires_grad_() for x in dLs]
    dL1s = [x.cuda().requires_grad_() for x in dL1s]
    base = (views[0], views[1], (0, 0), dLs, views[2], views[3], (0, 0), dL1s, [0, 1], [1.0, 0.5], [1, 2], True, delts)

    def run(**kw):
        return _launches(lambda: cv.selfsup_pyramid_loss(*base, **kw).backward(), monkeypatch)
    names, fills = run(objective="cap", terms=("ds",), ds_divisors=[1, 2])
    assert names == ["selfsup_cap_ds_fwd_tiles+reduce", "selfsup_cap_ds_bwd_gather"] and fills == 0
    assert [len(n.split("+")) for n in names] == [2, 1]
    names, fills = run(objective="cap", terms=(), ds_divisors=[1, 2])
    assert names == ["selfsup_cap_fwd_tiles+reduce", "selfsup_cap_bwd_gather"] and fills == 0
    names, fills = run(objective="cap", terms=("ds", "lr"))
    assert names == ["selfsup_cap_ds_lr_fwd_tiles+reduce", "selfsup_cap_ds_lr_bwd"] and fills == 1
    names, fills = run()                                   # depthmono-mask: as before
    assert names == ["selfsup_fwd", "selfsup_bwd"] and fills == 1


@pytest.mark.parametrize("name", ["Cap_ds-mask", "Cap_ds"])
def test_full_pyramid_vs_reference_fixture(hip_lib, name):
    """train.losses(name, 7) end to end (upsampling, epsilon draws, divisors, fused op) against the
    reference's own losses_pyramid1 + loss_Cap_ds_lr executed in fp64
    (tests/golden/make_goldens_cap.py)."""
    from dsmnet_amd import train
    from tests.conftest import Golden
    z, case = Golden("cap"), "pyr7"
    meta = z.meta["cases"][case]
    assert name in meta["names"]
    lossfun = train.losses(name, meta["count_levels"], meta["maxepoch"])
    lossfun.Weight_Adjust_levels(meta["epoch"])
    assert any(w != 0.01 for w in lossfun.weight_levels[3:])
    batch = torch.from_numpy(z[case + ".batch"].astype(np.float32) / 255.0).cuda()
    nedge, n = meta["nedge"], meta["levels"]
    h, w = batch.shape[2:]
    batch1 = torch.flip(batch, dims=[-1])
    dLs = [torch.from_numpy(z["%s.dispL.%d" % (case, i)]).cuda().requires_grad_() for i in range(n)]
    dL1s = [torch.from_numpy(z["%s.dispL1.%d" % (case, i)]).cuda().requires_grad_() for i in range(n)]
    args = {"imR_src": batch[:, 3:6], "imL": batch[:, :3, nedge:h - nedge, nedge:w - nedge],
            "dispLs": dLs, "scale_dispLs": list(range(n)), "LeftTop": [nedge, nedge],
            "imR1_src": batch1[:, :3], "imL1": batch1[:, 3:6, nedge:h - nedge, nedge:w - nedge],
            "dispL1s": dL1s, "scale_dispL1s": list(range(n)), "LeftTop1": [nedge, nedge]}
    torch.manual_seed(meta["seed"])
    loss = lossfun(args)
    loss.backward()
    tag = "%s.%s" % (case, name)
    want = float(z[tag + ".loss"])
    got = float(loss.detach())
    print("%s: loss %.8f vs %.8f rel %.2e" % (tag, got, want, abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-5 * abs(want), (tag, got, want)
    _grad_close([d.grad for d in dLs] + [d.grad for d in dL1s],
                [torch.from_numpy(z["%s.gL.%d" % (tag, i)]).cuda() for i in range(n)] +
                [torch.from_numpy(z["%s.gL1.%d" % (tag, i)]).cuda() for i in range(n)], tag)


def test_train_and_validate_step_dispnetcorr_cap_ds_mask(hip_lib):
    """The KITTI preset's objective through train_step_selfsup / validate_step_selfsup (B=2,
    192x384 source, nedge 64).  A first step with a zero learning rate leaves the parameters where
    they were, so a second step with the same seed (the epsilon draws) sees the same loss: the loss
    forward has a fixed summation order, 1e-6 only allows for the model's own kernels."""
    from dsmnet_amd import train
    from dsmnet_amd.models import model_create_by_name
    batch = _selfsup_batch(2, 192, 384, 21)
    torch.manual_seed(0)
    model = model_create_by_name("dispnetcorr", 192).cuda()
    lossfun = train.losses("Cap_ds-mask", model.count_levels, 10)
    lossfun.Weight_Adjust_levels(4)
    before = [p.detach().clone() for p in model.parameters()]
    out = []
    for opt in (torch.optim.SGD(model.parameters(), lr=0.0), train.make_optimizer(model, lr=1e-4)):
        torch.manual_seed(5)
        out.append(train.train_step_selfsup(model, opt, lossfun, batch))
        assert np.isfinite(out[-1][0]) and out[-1][1:] == (-1.0, -1.0)
        assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    assert abs(out[0][0] - out[1][0]) <= 1e-6 * abs(out[0][0]), out
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    torch.manual_seed(9)
    val = train.validate_step_selfsup(model, lossfun, batch)
    assert np.isfinite(val[0]) and val[1:] == (-1.0, -1.0)
