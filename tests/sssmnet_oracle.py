"""TEST INFRASTRUCTURE ONLY: float64 stock-torch restatement of the reference's "SsSMnet[-mask]"
and "common[-mask]" objectives, the yardstick of those rules of the fused csrc/selfsup.hip path.

  diff2_dx / diff2_dy   losses/loss.py:46-54
  diff_z_dx / diff_z_dy losses/loss.py:56-64
  c_imdiff1             losses/loss.py:66-69
  c_ds2                 losses/loss.py:85-97
  c_ds3                 losses/loss.py:99-114
  loss_common           losses/loss.py:154-194 (through losses_pyramid1, :424-467)
  loss_sssmnet          losses/loss.py:285-324
  losses_pyramid2       losses/loss.py:469-512 (the warp of a warp; four epsilons per weighted
                        entry, six with -mask: imL_wrap, imL1_wrap, imL_wrap1, imL1_wrap1,
                        dispL_wrap, dispL1_wrap)

Everything else -- ssim, imwrap_bchw, weight_common, draw_delt, create_impyramid, wfun, diff1 --
is tests/selfsup_oracle.py's, imported, with the same version-drift decisions (DESIGN.md section
12): align_corners=False sampling and the uint8 mask expressions in their PyTorch 0.3 meaning
(loss.py:171 and :300: ``(a + b) > 1`` on uint8 is ``a & b``).

loss_common is loss_depthmono with c_ds3 in place of c_ds1.  loss_sssmnet has no "< 1024 valid
pixels" fallback; with no valid pixel the reference's mean of an empty selection is NaN and its
``max(0, nan)`` (Python's builtin) returns 0, so w = 0.001: restated here without the NaN, as
tests/cap_oracle.py does.

Pinned against the reference's own lines (tests/golden/make_goldens_sssmnet.py, fixture
tests/golden/golden_sssmnet.npz).  Works on CPU and GPU tensors; ``dtype=torch.float32`` gives the
stock path for timing.
"""
import torch
import torch.nn.functional as F

from tests.selfsup_oracle import (create_impyramid, diff1_dx, diff1_dy, draw_delt, imwrap_bchw, ssim,
                                  weight_common, wfun)


def diff2_dx(img):
    return F.pad(img[:, :, :, 2:] + img[:, :, :, :-2] - img[:, :, :, 1:-1] - img[:, :, :, 1:-1], [1, 1, 0, 0])


def diff2_dy(img):
    return F.pad(img[:, :, 2:] + img[:, :, :-2] - img[:, :, 1:-1] - img[:, :, 1:-1], [0, 0, 1, 1])


def diff_z_dx(d):
    return F.pad(d[:, :, :, 1:-1] / d[:, :, :, 2:] + d[:, :, :, 1:-1] / d[:, :, :, :-2] - 2, [1, 1, 0, 0])


def diff_z_dy(d):
    return F.pad(d[:, :, 1:-1] / d[:, :, 2:] + d[:, :, 1:-1] / d[:, :, :-2] - 2, [0, 0, 1, 1])


def c_imdiff1(img, img_wrap):
    return (diff1_dx(img) - diff1_dx(img_wrap)).abs() + (diff1_dy(img) - diff1_dy(img_wrap)).abs()


def c_ds2(img, disp):
    wx = torch.exp(-diff2_dx(img).abs().sum(1, keepdim=True))
    wy = torch.exp(-diff2_dy(img).abs().sum(1, keepdim=True))
    return diff2_dx(disp).abs() * wx + diff2_dy(disp).abs() * wy


def c_ds3(img, disp):
    d = disp.abs() + 1
    ix, iy = diff1_dx(img).abs(), diff1_dy(img).abs()
    mx = ix.mean(-1, True).mean(-2, True).mean(-3, True)
    my = iy.mean(-1, True).mean(-2, True).mean(-3, True)
    wx = torch.exp(-ix.max(dim=1, keepdim=True)[0] / (0.5 * mx))
    wy = torch.exp(-iy.max(dim=1, keepdim=True)[0] / (0.5 * my))
    return diff_z_dx(d).abs().clamp(0, 10) * wx + diff_z_dy(d).abs().clamp(0, 10) * wy


def loss_common(im, im_wrap, disp, disp_wrap, weight_common=None, stats=None):
    """One view of one level.  ``stats``: a list that receives (w, fallback, simlary)."""
    mask_ap = (im_wrap[:, :1] != 0).detach()
    fallback = mask_ap.sum() < 1024
    mask_ap = mask_ap | fallback
    img_ssim = ssim(im, im_wrap)
    m = mask_ap.to(img_ssim.dtype)
    simlary = ((img_ssim * m).sum() / m.sum()).detach()
    w = wfun(simlary)
    if stats is not None:
        stats.append((w, fallback, simlary))
    c_ap = 0.425 * (1 - img_ssim) + 0.15 * (im - im_wrap).abs()
    c_lr = (disp - disp_wrap).abs()
    if weight_common is not None:
        mask_im = ((disp_wrap == 0) & mask_ap).detach()
        mask_lr = (disp_wrap == 0).detach()
        c_ap = c_ap * torch.where(mask_im, torch.ones_like(weight_common), weight_common)
        c_lr = c_lr * torch.where(mask_lr, torch.zeros_like(weight_common), weight_common)
    return c_ap.mean() + c_ds3(im, disp).mean() * w + c_lr.mean() * w


def loss_sssmnet(im, im_wrap, im_wrap1, disp, factor=1.0, weight_common=None, stats=None):
    """One view of one level.  ``stats``: a list that receives (w, n_valid, simlary)."""
    img_ssim = ssim(im, im_wrap)
    mask_ap = (im_wrap[:, :1] != 0).detach()
    m = mask_ap.to(img_ssim.dtype)
    n_valid = m.sum()
    simlary = ((img_ssim * m).sum() / n_valid.clamp_min(1)).detach()
    w = torch.where(n_valid > 0, wfun(simlary), torch.full_like(simlary, 0.001))
    if stats is not None:
        stats.append((w, n_valid, simlary))
    c_ap = 0.425 * (1 - img_ssim) + 0.15 * ((im - im_wrap).abs() + c_imdiff1(im, im_wrap))
    c_lr = (im - im_wrap1).abs()
    if weight_common is not None:
        mask_lr = im_wrap1[:, :1] == 0
        mask_im = (mask_lr & mask_ap).detach()
        c_ap = c_ap * torch.where(mask_im, torch.ones_like(weight_common), weight_common)
        c_lr = c_lr * torch.where(mask_lr, torch.zeros_like(weight_common), weight_common)
    return c_ap.mean() + c_ds2(im, disp).mean() * (w / factor) + c_lr.mean() * w + disp.abs().mean() * 1e-4


N_DELTS = {("common", False): 4, ("common", True): 4, ("sssmnet", False): 4, ("sssmnet", True): 6}


def losses_pyramid(objective, weight_levels, flag_mask, imR_src, imL, dispLs, scale_dispLs, LeftTop,
                   imR1_src, imL1, dispL1s, LeftTop1, delts=None, dtype=torch.float64, stats=None):
    """losses_pyramid1 with loss_common (``objective="common"``) or losses_pyramid2 with
    loss_sssmnet (``"sssmnet"``): the weighted pyramid sum.  ``delts``: one tuple per level with a
    nonzero weight, in the reference's draw order; None draws them here with ``draw_delt``.
    Returns (loss, delts used).  Inputs are cast to ``dtype`` (autograd flows)."""
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
    nd = N_DELTS[(objective, bool(flag_mask))]
    used, j, loss = [], 0, 0
    for i, level in enumerate(scale_dispLs):
        weight = weight_levels[level]
        if weight <= 0 if objective == "common" else weight == 0:      # loss.py:437 against :482
            continue
        if level > maxlevel:
            sf = 2 ** maxlevel
            up = lambda d: F.interpolate(d, scale_factor=2 ** (level - maxlevel), mode="bilinear",
                                         align_corners=False)[:, :, :h, :w]
            dL, dL1 = up(dispLs[i]), up(dispL1s[i])
        else:
            sf = 2 ** level
            dL, dL1 = dispLs[i], dispL1s[i]
        dl = tuple(delts[j]) if delts is not None else tuple(draw_delt() for _ in range(nd))
        used.append(dl)
        j += 1
        k = min(level, maxlevel)
        imL_wrap = imwrap_bchw(imR_src, dL, dl[0], False, LeftTop, sf)
        imL1_wrap = imwrap_bchw(imR1_src, dL1, dl[1], False, LeftTop1, sf)
        wc = wc1 = None
        if objective == "common":
            dispL_wrap = imwrap_bchw(dL1, dL, dl[2], True, (0, 0), 1)
            dispL1_wrap = imwrap_bchw(dL, dL1, dl[3], True, (0, 0), 1)
            if flag_mask:
                wc = weight_common(dL, dispL_wrap, sf)
                wc1 = weight_common(dL1, dispL1_wrap, sf)
            t0 = loss_common(imLs[k], imL_wrap, dL, dispL_wrap, wc, stats)
            t1 = loss_common(imL1s[k], imL1_wrap, dL1, dispL1_wrap, wc1, stats)
        else:
            imL_wrap1 = imwrap_bchw(imL1_wrap, dL, dl[2], True, (0, 0), 1)
            imL1_wrap1 = imwrap_bchw(imL_wrap, dL1, dl[3], True, (0, 0), 1)
            if flag_mask:
                wc = weight_common(dL, imwrap_bchw(dL1, dL, dl[4], True, (0, 0), 1), sf)
                wc1 = weight_common(dL1, imwrap_bchw(dL, dL1, dl[5], True, (0, 0), 1), sf)
            t0 = loss_sssmnet(imLs[k], imL_wrap, imL_wrap1, dL, 2 ** level, wc, stats)
            t1 = loss_sssmnet(imL1s[k], imL1_wrap, imL1_wrap1, dL1, 2 ** level, wc1, stats)
        loss = loss + (t0 + t1) * weight
    return loss, used
