"""TEST INFRASTRUCTURE ONLY: float64 stock-torch restatement of the reference's self-supervised
"depthmono[-mask]" objective, the yardstick of the fused csrc/selfsup.hip path.

  create_impyramid      losses/loss.py:17-22
  wfun                  losses/loss.py:33-34
  diff1_dx / diff1_dy   losses/loss.py:36-44
  c_ds1                 losses/loss.py:71-83
  loss_depthmono        losses/loss.py:196-236
  weight_common         losses/loss.py:393-405
  losses_pyramid1       losses/loss.py:424-467
  gaussian / ssim       losses/SSIM.py:6-14, 24-42, 94-117 (ONE output channel: the window is
                        divided by C and applied with groups=1)
  imwrap_bchw           utils/imwrap.py:37-72 (LeftTop, scale_factor, fliplr)
  draw_delt             utils/imwrap.py:70 (one torch.rand(1) from the CPU generator per warp)

Version drift, as DESIGN.md section 12 records: align_corners=False sampling; the two uint8 mask
expressions in their PyTorch 0.3 meaning (mask2 = (delta < 3) & ~(delta < 1), mask_im =
(disp_wrap == 0) & mask_ap); simlary a detached device scalar, not a host read.

Pinned against the reference's own lines (tests/golden/make_goldens_selfsup.py, fixture
tests/golden/golden_selfsup.npz).  Works on CPU and GPU tensors; computes in float64 unless the
inputs are another floating dtype and ``dtype`` says so.
"""
from math import exp

import torch
import torch.nn.functional as F


def draw_delt():
    """``1e-4 * (torch.rand(1)[0] + 0.1)`` in the reference's fp32 arithmetic, as a float."""
    return float(1e-4 * (torch.rand(1)[0] + 0.1))


def create_impyramid(im, levels):
    out = [im]
    for _ in range(1, levels):
        out.append(out[-1][:, :, ::2, ::2])
    return out


def wfun(similarity):
    return (similarity - 0.75).clamp(min=0) / 2 + 0.001


def diff1_dx(img):
    return F.pad(img[:, :, :, 1:] - img[:, :, :, :-1], [0, 1, 0, 0])


def diff1_dy(img):
    return F.pad(img[:, :, 1:] - img[:, :, :-1], [0, 0, 0, 1])


def c_ds1(img, disp):
    wx = torch.exp(-diff1_dx(img).abs().sum(1, keepdim=True))
    wy = torch.exp(-diff1_dy(img).abs().sum(1, keepdim=True))
    return diff1_dx(disp).abs() * wx + diff1_dy(disp).abs() * wy


def gaussian_window():
    """The 11x11 window: fp32 1-D taps (sigma 1.5) normalised in fp32, outer product in fp32."""
    g = torch.tensor([exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = g / g.sum()
    return g.unsqueeze(1).mm(g.unsqueeze(0))


def ssim(img1, img2):
    """(B,1,H,W) map: channel-mean Gaussian statistics, zero padding 5."""
    C = img1.shape[1]
    win = gaussian_window().to(img1).expand(C, 1, 11, 11).transpose(0, 1) / C
    conv = lambda x: F.conv2d(x, win, padding=5)
    mu1, mu2 = conv(img1), conv(img2)
    s1 = conv(img1 * img1) - mu1 * mu1
    s2 = conv(img2 * img2) - mu2 * mu2
    s12 = conv(img1 * img2) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))


def imwrap_bchw(im_src, disp, delt, fliplr=False, lefttop=(0, 0), scale_factor=1):
    """grid_sample(im_src + delt, grid, bilinear, zeros, align_corners=False); the base grid is
    torch.linspace in fp32 (as the reference builds it), the disparity offset in im_src's dtype."""
    bn, _, h0, w0 = im_src.shape
    _, c, h, w = disp.shape
    assert c == 1 and min(h, w, h0, w0) > 1
    x = lefttop[0] * 2.0 / (w0 - 1) - 1
    y = lefttop[1] * 2.0 / (h0 - 1) - 1
    x1 = x + (w - 1) * scale_factor * 2.0 / (w0 - 1)
    y1 = y + (h - 1) * scale_factor * 2.0 / (h0 - 1)
    row = torch.linspace(x, x1, w).to(im_src)
    col = torch.linspace(y, y1, h).to(im_src)
    gx = row.view(1, 1, w) - disp[:, 0] * 2.0 / (w0 - 1)
    if fliplr:
        gx = -gx
    gy = col.view(1, h, 1).expand(bn, h, w)
    grid = torch.stack([gx, gy], -1)
    return F.grid_sample(im_src + delt, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def weight_common(disp, disp_wrap, factor=1.0):
    delta = (disp - disp_wrap).abs().detach() / factor
    m1 = delta < 1
    m2 = (delta < 3) & ~m1                       # PyTorch 0.3: uint8 (a - b)
    w = torch.full_like(delta, 0.01)
    w = torch.where(m2, 1.0 - (delta - 1) * (0.99 / 2), w)
    return torch.where(m1, torch.ones_like(w), w)


def loss_depthmono(im, im_wrap, disp, disp_wrap, weight_common=None, stats=None):
    """One view of one level.  ``stats``: a list that receives (w, fallback, simlary)."""
    img_ssim = ssim(im, im_wrap)
    mask_ap = (im_wrap[:, :1] != 0).detach()
    n_valid = mask_ap.sum()
    fallback = n_valid < 1024
    mask_ap = mask_ap | fallback                  # fewer than 1024 valid: every pixel
    m = mask_ap.to(img_ssim.dtype)
    simlary = ((img_ssim * m).sum() / m.sum()).detach()
    w = wfun(simlary)
    if stats is not None:
        stats.append((w, fallback, simlary))
    c_ap = 0.425 * (1 - img_ssim) + 0.15 * (im - im_wrap).abs()
    c_lr = (disp - disp_wrap).abs()
    if weight_common is not None:
        mask_im = ((disp_wrap == 0) & mask_ap).detach()   # PyTorch 0.3: (a + b) > 1 on uint8
        mask_lr = disp_wrap == 0
        weight_im = torch.where(mask_im, torch.ones_like(weight_common), weight_common)
        weight_lr = torch.where(mask_lr, torch.zeros_like(weight_common), weight_common)
        c_ap = c_ap * weight_im
        c_lr = c_lr * weight_lr
    return c_ap.mean() + c_ds1(im, disp).mean() * w + c_lr.mean() * w


def losses_pyramid1(weight_levels, flag_mask, imR_src, imL, dispLs, scale_dispLs, LeftTop,
                    imR1_src, imL1, dispL1s, LeftTop1, delts=None, dtype=torch.float64, stats=None):
    """The weighted pyramid sum.  ``delts``: a list of 4-tuples, one per level with a positive
    weight (draw order imL_wrap, imL1_wrap, dispL_wrap, dispL1_wrap); None draws them here with
    ``draw_delt``.  Returns (loss, delts used).  Inputs are cast to ``dtype`` (autograd flows)."""
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
        t0 = loss_depthmono(imLs[k], imL_wrap, dL, dispL_wrap, wc, stats)
        t1 = loss_depthmono(imL1s[k], imL1_wrap, dL1, dispL1_wrap, wc1, stats)
        loss = loss + (t0 + t1) * weight
    return loss, used
