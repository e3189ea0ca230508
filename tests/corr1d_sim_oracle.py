"""Restatement of ``Corr1d(kernel_size, stride, D, simfun=nn.CosineSimilarity(dim=1, eps))`` in plain torch
(reference: models/util_conv.py:56-86), dtype-generic: float64 when handed float64.  Gradients by autograd.

    a(b,y,x) = 1 / max(|fL[b,:,y,x]|, eps)      r(b,y,x) = 1 / max(|fR[b,:,y,x]|, eps)      x' = x - i*stride
    raw[b,i,y,x] = a(x) r(x') sum_c fL[b,c,y,x] fR[b,c,y,x']        for x' >= 0, else 0
    out = raw (kernel_size 1)  or  AvgPool2d(k, 1, k//2)(raw)       (zero padding counted in the divisor)

Each norm is clamped on its own (``F.cosine_similarity`` of torch >= 1.12), and a clamped norm is a CONSTANT:
the pixel's inverse norm is the number ``1 / eps`` there, so autograd sees no path through it (and never
differentiates a square root at zero).  tests/golden/golden_corr_sim.npz pins this file to the reference."""
import torch
import torch.nn.functional as F


def inv_norm(f, eps):
    """(B,H,W): 1 / max(|f[:, :, y, x]|, eps); constant where the norm is below eps."""
    s = (f * f).sum(dim=1)
    live = s.detach().sqrt() >= eps
    safe = torch.where(live, s, torch.ones_like(s))
    return torch.where(live, 1.0 / safe.sqrt(), torch.full_like(s, 1.0 / eps))


def corr1d_cosine_raw(fL, fR, D, stride=1, eps=1e-8):
    B, C, H, W = fL.shape
    a, r = inv_norm(fL, eps), inv_norm(fR, eps)
    planes = []
    for i in range(D):
        shift = i * stride
        if shift < W:
            dot = (fL[..., shift:] * fR[..., : W - shift]).sum(dim=1)
            planes.append(F.pad(dot * a[..., shift:] * r[..., : W - shift], (shift, 0)))
        else:
            planes.append(fL.new_zeros(B, H, W))
    return torch.stack(planes, dim=1)


def corr1d_cosine(fL, fR, D, stride=1, kernel_size=1, eps=1e-8):
    raw = corr1d_cosine_raw(fL, fR, D, stride, eps)
    if kernel_size > 1:
        if kernel_size % 2 != 1:
            raise AssertionError("kernel_size must be odd")  # util_conv.py:83
        return F.avg_pool2d(raw, kernel_size, stride=1, padding=kernel_size // 2)
    return raw


def with_grads(fL, fR, cot, D, stride=1, kernel_size=1, eps=1e-8):
    """(out, dfL, dfR) of the restatement in the dtype of the inputs."""
    l, r = fL.detach().clone().requires_grad_(True), fR.detach().clone().requires_grad_(True)
    out = corr1d_cosine(l, r, D, stride, kernel_size, eps)
    gl, gr = torch.autograd.grad(out, (l, r), cot.to(out.dtype))
    return out.detach(), gl, gr


def make_degenerate(fL, fR):
    """The clamp region: a zero vector on either side and a left vector shorter than eps (in place)."""
    fL[0, :, 0, 3] = 0
    fR[0, :, 1, 5] = 0
    fL[0, :, 1, 7] *= 1e-10
    return fL, fR


DEGENERATE_PIXELS = (("L", 0, 0, 3), ("R", 0, 1, 5), ("L", 0, 1, 7))
