"""Folded BatchNorm affines and the keys their caches are held under.

A leaf module: ``costvolume`` (the wide layers' weight packs), ``blocks3d``, ``blocks2d`` and PSMNet's SPP
head all key a cache on ``_versions``, and the last three fold with ``fold_affine``.  It imports only torch,
so any of them can import it; ``blocks3d`` hands the names on to its callers (``graphs``, ``refold()``)."""
import torch

_EPOCH = [0]


def invalidate_folded_caches():
    """Drop every cached packed weight / folded BN affine (3-D blocks, 2-D blocks, SPP head):
    they are re-made at the next forward.  The caches notice ordinary updates by themselves
    (optimizer steps, ``load_state_dict``, ``with torch.no_grad(): w.mul_(...)`` -- all bump the
    tensor's ``_version``); an in-place edit THROUGH ``.data`` (``w.data.mul_()``) does not, and
    needs this call afterwards.  Exported as ``dsmnet_amd.refold()``."""
    _EPOCH[0] += 1


def _bump_running_stats(bn):
    """The BN kernels update the running statistics through raw pointers: bump the two tensors'
    version counters by hand, so that exactly the folds made from THIS layer's statistics are re-made
    at the next eval forward (a global invalidation would re-pack every layer after every step)."""
    if bn.track_running_stats and bn.running_mean is not None:
        torch.autograd.graph.increment_version(bn.running_mean)
        torch.autograd.graph.increment_version(bn.running_var)


def _versions(*tensors):
    return tuple((t.data_ptr(), t._version) for t in tensors if t is not None) + (_EPOCH[0],)


def fold_affine(conv_bias, bn, cout, device):
    """(scale, shift) with ``bn(conv(x) + conv_bias) == conv(x) * scale + shift`` for an eval-mode
    BatchNorm ``bn`` (or None) after a convolution of ``cout`` outputs: what the kernels' epilogues
    apply.  (None, None) when there is neither a BatchNorm nor a bias.  Call under ``torch.no_grad()``."""
    if bn is not None:
        inv = torch.rsqrt(bn.running_var + bn.eps)
        scale = bn.weight * inv if bn.weight is not None else inv
        shift = -bn.running_mean * scale
        if bn.bias is not None:
            shift = shift + bn.bias
        if conv_bias is not None:
            shift = shift + conv_bias * scale
        return scale.contiguous(), shift.contiguous()
    if conv_bias is not None:
        return torch.ones(cout, device=device), conv_bias.detach().clone()
    return None, None
