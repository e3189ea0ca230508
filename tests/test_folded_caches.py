"""When ``blocks3d._Folded`` re-makes its packed weight and folded BN affine, on the host: the packer is a HIP
launch, so a counting stand-in replaces it here; the scale / shift arithmetic is plain torch and runs as it is.

The cache is keyed on the storage address and ``_version`` of every source tensor plus a global epoch.  A
hipGraph replay changes weights and running statistics without running Python, so nothing bumps a version:
``GraphedTrainStep.__call__`` has to advance the epoch itself (``invalidate_folded_caches``), and the BN
kernels' eager wrappers bump the running statistics by hand (``_bump_running_stats``)."""
import pytest
import torch
import torch.nn as nn

from dsmnet_amd import blocks3d


@pytest.fixture
def packs(monkeypatch):
    calls = []

    def pack(weight, transposed):
        calls.append((weight.data_ptr(), weight._version, bool(transposed)))
        return weight.detach().clone().flatten()
    monkeypatch.setattr(blocks3d.cv, "pack_conv3d_weight", pack)
    return calls


def _pair():
    torch.manual_seed(3)
    conv, bn = nn.Conv3d(4, 8, 3, padding=1, bias=False), nn.BatchNorm3d(8)
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.normal_()
        bn.bias.normal_()
    return conv, bn


def _want(conv, bn):
    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return scale, bn.bias.double() - bn.running_mean.double() * scale


def _check(folded, conv, bn):
    packed, scale, shift = folded.get(conv, bn)
    ws, wb = _want(conv, bn)
    assert torch.equal(packed, conv.weight.detach().flatten())
    assert (scale.double() - ws).abs().max().item() <= 1e-6 * ws.abs().max().item()
    assert (shift.double() - wb).abs().max().item() <= 1e-6 * max(1.0, wb.abs().max().item())
    return packed, scale, shift


def test_folds_are_kept_until_a_source_changes(packs):
    conv, bn = _pair()
    folded = blocks3d._Folded()
    first = _check(folded, conv, bn)
    again = folded.get(conv, bn)
    assert len(packs) == 1 and all(a is b for a, b in zip(first, again))         # served from the cache
    bn.eval()
    conv(torch.zeros(1, 4, 2, 2, 2))                                             # reading changes nothing
    assert folded.get(conv, bn)[0] is first[0] and len(packs) == 1
    with torch.no_grad():
        conv.weight.mul_(2.0)                                                    # an optimizer step does this
    _check(folded, conv, bn)
    assert len(packs) == 2
    with torch.no_grad():
        bn.running_var.add_(1.0)
    _check(folded, conv, bn)
    assert len(packs) == 3 and folded.get(conv, bn)[1] is folded.scale and len(packs) == 3


def test_writes_that_bump_no_version_need_the_epoch_or_the_hand_bump(packs):
    """What a graph replay (or a kernel writing through a raw pointer) does: the values change, the version
    counters do not.  The cache cannot notice -- that is stated here, not wished away -- and each of the two
    remedies makes exactly the stale fold fresh."""
    conv, bn = _pair()
    other_conv, other_bn = _pair()
    folded, other = blocks3d._Folded(), blocks3d._Folded()
    _check(folded, conv, bn)
    _check(other, other_conv, other_bn)
    assert len(packs) == 2
    bn.running_mean.data.add_(3.0)                    # through .data: no version bump, as from a raw pointer
    conv.weight.data.mul_(0.5)
    stale = folded.get(conv, bn)
    assert len(packs) == 2                            # still the old fold ...
    assert (stale[2].double() - _want(conv, bn)[1]).abs().max().item() > 1.0     # ... of the old statistics
    blocks3d._bump_running_stats(bn)                  # remedy 1: per layer, what the eager BN wrappers call
    _check(folded, conv, bn)
    assert len(packs) == 3
    other.get(other_conv, other_bn)
    assert len(packs) == 3                            # ... and only that layer was re-made
    conv.weight.data.mul_(0.5)
    assert folded.get(conv, bn)[0] is folded.packed and len(packs) == 3
    assert not torch.equal(folded.packed, conv.weight.detach().flatten())
    blocks3d.invalidate_folded_caches()               # remedy 2: global, what GraphedTrainStep calls per replay
    _check(folded, conv, bn)
    _check(other, other_conv, other_bn)
    assert len(packs) == 5
    folded.get(conv, bn), other.get(other_conv, other_bn)
    assert len(packs) == 5


def test_bump_skips_layers_without_running_statistics(packs):
    bn = nn.BatchNorm3d(8, track_running_stats=False)
    blocks3d._bump_running_stats(bn)                  # nothing to bump, nothing raised
    conv = nn.Conv3d(4, 8, 3, padding=1, bias=True)
    folded = blocks3d._Folded()
    packed, scale, shift = folded.get(conv, None)     # a biased convolution without BN: scale 1, shift bias
    assert torch.equal(scale, torch.ones(8)) and torch.equal(shift, conv.bias.detach())
    assert folded.get(conv, None)[0] is packed and len(packs) == 1
