"""TEST INFRASTRUCTURE ONLY: float64 stock-torch restatement of the reference's "Cap[_ds][_lr]
[-mask]" objective, the yardstick of the Cap rule of the fused csrc/selfsup.hip path.

  loss_cap_ds_lr        losses/loss.py:238-283 (loss_Cap_ds_lr)
  losses_pyramid1       losses/loss.py:424-467 driving it (factor = 2**level of the output's OWN
                        level, :456; scale_factor = 2**min(level, maxlevel))
  terms_of              losses/loss.py:345-346, 270, 275: the terms a loss name selects

Everything else -- ssim, imwrap_bchw, weight_common, c_ds1, draw_delt, create_impyramid -- is
tests/selfsup_oracle.py's, imported, with the same version-drift decisions (DESIGN.md section
12): align_corners=False sampling and the uint8 mask expressions in their PyTorch 0.3 meaning.

What differs from loss_depthmono: mask_ap has no "< 1024 valid pixels" fallback; C_ds is weighted
w / factor; C_ds and C_lr exist only when the name has "ds" / "lr".  With no valid pixel the
reference's mean of an empty selection is NaN and its ``max(0, nan)`` (Python's builtin) returns
0, so w = 0.001: restated here without the NaN.

Pinned against the reference's own lines (tests/golden/make_goldens_cap.py, fixture
tests/golden/golden_cap.npz).  Works on CPU and GPU tensors.
"""
import torch
import torch.nn.functional as F

from tests.selfsup_oracle import c_ds1, create_impyramid, draw_delt, imwrap_bchw, ssim, weight_common


def terms_of(loss_name):
    """("ds", "lr") subset named by the part of ``loss_name`` before "-", lower-cased."""
    name = loss_name.split("-")[0].lower()
    return tuple(t for t in ("ds", "lr") if t in name)


def loss_cap_ds_lr(im, im_wrap, disp, disp_wrap, factor=1.0, weight_common=None, terms=("ds", "lr"),
                   stats=None):
    """One view of one level.  ``stats``: a list that receives (w, n_valid, simlary)."""
    img_ssim = ssim(im, im_wrap)
    mask_ap = (im_wrap[:, :1] != 0).detach()
    m = mask_ap.to(img_ssim.dtype)
    n_valid = m.sum()
    simlary = ((img_ssim * m).sum() / n_valid.clamp_min(1)).detach()
    w = torch.where(n_valid > 0, (simlary - 0.75).clamp(min=0) / 2 + 0.001, torch.full_like(simlary, 0.001))
    if stats is not None:
        stats.append((w, n_valid, simlary))
    c_ap = 0.425 * (1 - img_ssim) + 0.15 * (im - im_wrap).abs()
    c_lr = (disp - disp_wrap).abs()
    if weight_common is not None:
        mask_im = ((disp_wrap == 0) & mask_ap).detach()   # PyTorch 0.3: (a + b) > 1 on uint8
        mask_lr = disp_wrap == 0
        weight_im = torch.where(mask_im, torch.ones_like(weight_common), weight_common)
        weight_lr = torch.where(mask_lr, torch.zeros_like(weight_common), weight_common)
        c_ap = c_ap * weight_im
        c_lr = c_lr * weight_lr
    c = c_ap.mean()
    if "ds" in terms:
        c = c + c_ds1(im, disp).mean() * (w / factor)
    if "lr" in terms:
        c = c + c_lr.mean() * w
    return c


def losses_pyramid1(weight_levels, flag_mask, terms, imR_src, imL, dispLs, scale_dispLs, LeftTop,
                    imR1_src, imL1, dispL1s, LeftTop1, delts=None, dtype=torch.float64, stats=None):
    """The weighted pyramid sum, as selfsup_oracle.losses_pyramid1 with the Cap objective.
    Returns (loss, delts used)."""
    cast = lambda t: t.to(dtype)
    imR_src, imL, imR1_src, imL1 = map(cast, (imR_src, imL, imR1_src, imL1))
    dispLs = [cast(d.unsqueeze(1) if d.dim() == 3 else d) for d in dispLs]
    dispL1s = [cast(d.unsqueeze(1) if d.dim() == 3 else d) for d in dispL1s]
    maxlevel = min(2, max(scale_dispLs))
    h = w = None
    if maxlevel in scale_dispLs:
        _, _, h, w = dispLs[maxlevel].shape
    imLs = create_impyramid(imL, maxlevel + 1)
    imL1s = create_impyramid(imL1, maxlevel + 1)
    used, j, loss = [], 0, 0
    for i, level in enumerate(scale_dispLs):
        weight = weight_levels[level]
        if weight <= 0:
            continue
        if level > maxlevel:
            sf = 2 ** maxlevel
            up = lambda d: F.interpolate(d, scale_factor=2 ** (level - maxlevel), mode="bilinear",
                                         align_corners=False)[:, :, :h, :w]
            dL, dL1 = up(dispLs[i]), up(dispL1s[i])
        else:
            sf = 2 ** level
            dL, dL1 = dispLs[i], dispL1s[i]
        dl = tuple(delts[j]) if delts is not None else tuple(draw_delt() for _ in range(4))
        used.append(dl)
        j += 1
        imL_wrap = imwrap_bchw(imR_src, dL, dl[0], False, LeftTop, sf)
        imL1_wrap = imwrap_bchw(imR1_src, dL1, dl[1], False, LeftTop1, sf)
        dispL_wrap = imwrap_bchw(dL1, dL, dl[2], True, (0, 0), 1)
        dispL1_wrap = imwrap_bchw(dL, dL1, dl[3], True, (0, 0), 1)
        wc = wc1 = None
        if flag_mask:
            wc = weight_common(dL, dispL_wrap, sf)
            wc1 = weight_common(dL1, dispL1_wrap, sf)
        k = min(level, maxlevel)
        t0 = loss_cap_ds_lr(imLs[k], imL_wrap, dL, dispL_wrap, 2 ** level, wc, terms, stats)
        t1 = loss_cap_ds_lr(imL1s[k], imL1_wrap, dL1, dispL1_wrap, 2 ** level, wc1, terms, stats)
        loss = loss + (t0 + t1) * weight
    return loss, used
