"""Plain-torch restatement of "first convolution of a concatenation volume from 2-D maps"
(csrc/sepvol.hip), in the dtype of its inputs.  The weight enters in the order the
kernels read it (``costvolume.pack_concat_conv_weight``), so the packing is part of what is checked.

    KL[dz][dx][o, y, s] = sum_{dy,c} W[o, c,     dz, dy, dx] left [c, y + dy, s]
    KR[dz][dx][o, y, s] = sum_{dy,c} W[o, C + c, dz, dy, dx] right[c, y + dy, s]
    conv(vol)[o, d, y, x] = sum over (dz, dx) with 0 <= dd < D, 0 <= xx < W of
          [xx >= dd or not mask_left] KL[dz][dx][o, y, xx] + [xx >= dd] KR[dz][dx][o, y, xx - dd]
"""
import torch
import torch.nn.functional as F

from dsmnet_amd.costvolume import pack_concat_conv_weight


def column_maps(fL, fR, weight):
    """-> K of shape (2, 3, 3, B, Cout, H, W): [side][dz][dx]; 3 taps over dy only, zero padding in y."""
    cout, c2 = weight.shape[:2]
    C = c2 // 2
    wp = pack_concat_conv_weight(weight).reshape(2, 3, 3, 3, C // 2, 2, cout)     # side, dz, dx, dy, cc, h, o
    wk = wp.permute(0, 1, 2, 6, 5, 4, 3).reshape(2, 3, 3, cout, C, 3, 1)          # ..., o, c = h*C/2 + cc, dy, 1
    out = []
    for side, f in enumerate((fL, fR)):
        out.append(torch.stack([torch.stack([F.conv2d(f, wk[side, z, x], padding=(1, 0)) for x in range(3)])
                                for z in range(3)]))
    return torch.stack(out)


def general_form(fL, fR, weight, D, mask_left):
    """Every element of conv3d(concat_volume(fL, fR, D, mask_left), weight, padding=1): (B, Cout, D, H, W)."""
    K = column_maps(fL, fR, weight)
    B, _, H, W = fL.shape
    out = fL.new_zeros(B, weight.shape[0], D, H, W)
    xs = torch.arange(W)
    for d in range(D):
        plane = out[:, :, d]
        for dz in (-1, 0, 1):
            dd = d + dz
            if dd < 0 or dd >= D:
                continue
            for dx in (-1, 0, 1):
                xx = xs + dx
                ok = (xx >= 0) & (xx < W)
                seen = ok & (xx >= dd)                       # the shifted right map (and the masked left) has data
                lm = seen if mask_left else ok
                kl, kr = K[0, dz + 1, dx + 1], K[1, dz + 1, dx + 1]
                plane[..., xs[lm]] += kl[..., xx[lm]]
                plane[..., xs[seen]] += kr[..., xx[seen] - dd]
    return out


def interior_mask(D, W, mask_left):
    """(D, W) bool: elements where F[y, x] + G[y, x - d] applies as is (mask_left False: the left part
    is F for every x - d, the right part still needs x - d >= 2 for all its taps to exist)."""
    d = torch.arange(D)[:, None]
    x = torch.arange(W)[None, :]
    return (d >= 1) & (d <= D - 2) & (x >= 1) & (x <= W - 2) & (x - d >= 2)


def interior_shortcut(fL, fR, weight, D):
    """F + G on the whole (B, Cout, D, H, W) grid -- meaningful where ``interior_mask`` holds.
    F = sum_{dz,dx} KL[dz][dx][y, x + dx]; G[y, u] = sum_{dz,dx} KR[dz][dx][y, u + dx - dz], terms
    of negative index dropped."""
    K = column_maps(fL, fR, weight)
    B, _, H, W = fL.shape
    Fm = fL.new_zeros(B, weight.shape[0], H, W)
    Gm = fL.new_zeros(B, weight.shape[0], H, W)
    xs = torch.arange(W)
    for dz in (-1, 0, 1):
        for dx in (-1, 0, 1):
            xx = xs + dx
            ok = (xx >= 0) & (xx < W)
            Fm[..., xs[ok]] += K[0, dz + 1, dx + 1][..., xx[ok]]
            uu = xs + dx - dz
            ok = (uu >= 0) & (uu < W)
            Gm[..., xs[ok]] += K[1, dz + 1, dx + 1][..., uu[ok]]
    out = fL.new_zeros(B, weight.shape[0], D, H, W)
    for d in range(D):
        out[:, :, d] = Fm
        out[:, :, d, :, d:] += Gm[..., : max(W - d, 0)]
    return out
