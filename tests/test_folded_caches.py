"""When ``blocks3d._Folded`` and ``blocks2d._Folded2d`` re-make their packed weight and folded BN affine, on the
host: the packers are HIP launches, so a counting stand-in replaces them here; the scale / shift arithmetic
(``folds.fold_affine``, shared with PSMNet's SPP head) is plain torch and runs as it is.

The caches are keyed on the storage address and ``_version`` of every source tensor plus a global epoch
(``folds._versions``).  A hipGraph replay changes weights and running statistics without running Python, so
nothing bumps a version: ``GraphedTrainStep.__call__`` has to advance the epoch itself
(``invalidate_folded_caches``), and the BN kernels' eager wrappers bump the running statistics by hand
(``_bump_running_stats``)."""
import pytest
import torch
import torch.nn as nn

from dsmnet_amd import blocks2d, blocks3d, folds


class _Fold3d(object):
    """``blocks3d._Folded`` over Conv3d(4, 8) + BatchNorm3d(8)."""
    new, packer, cout, x = blocks3d._Folded, "pack_conv3d_weight", 8, (1, 4, 2, 2, 2)

    @staticmethod
    def layers(bias=False, **bn_args):
        return nn.Conv3d(4, 8, 3, padding=1, bias=bias), nn.BatchNorm3d(8, **bn_args)

    @staticmethod
    def get(folded, conv, bn):
        return folded.get(conv, bn)


class _Fold2d(object):
    """``blocks2d._Folded2d`` over Conv2d(16, 32) + BatchNorm2d(32), ``get(conv, bn, 16)``."""
    new, packer, cout, x = blocks2d._Folded2d, "pack_conv2d_weight", 32, (1, 16, 2, 2)

    @staticmethod
    def layers(bias=False, **bn_args):
        return nn.Conv2d(16, 32, 3, padding=1, bias=bias), nn.BatchNorm2d(32, **bn_args)

    @staticmethod
    def get(folded, conv, bn):
        return folded.get(conv, bn, 16)


@pytest.fixture(params=[_Fold3d, _Fold2d], ids=["3d", "2d"])
def Fold(request):
    return request.param


@pytest.fixture
def packs(Fold, monkeypatch):
    calls = []

    def pack(weight, arg=None):                       # arg: ``transposed`` (3-D) / ``cin_padded`` (2-D)
        calls.append((weight.data_ptr(), weight._version, arg))
        return weight.detach().clone().flatten()
    assert blocks2d.cv is blocks3d.cv                 # both classes look the packer up there at call time
    monkeypatch.setattr(blocks3d.cv, Fold.packer, pack)
    return calls


def _randomise(bn):
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
        if bn.affine:
            bn.weight.normal_()
            bn.bias.normal_()


def _pair(Fold):
    torch.manual_seed(3)
    conv, bn = Fold.layers()
    _randomise(bn)
    return conv, bn


def _want(conv, bn):
    """The fold in float64.  A BatchNorm without affine weights has weight 1 and bias 0; a convolution bias is
    added before the BatchNorm."""
    scale = (1.0 if bn.weight is None else bn.weight.double()) / torch.sqrt(bn.running_var.double() + bn.eps)
    shift = (0.0 if bn.bias is None else bn.bias.double()) - bn.running_mean.double() * scale
    if conv.bias is not None:
        shift = shift + conv.bias.double() * scale
    return scale, shift


def _close(scale, shift, conv, bn):
    ws, wb = _want(conv, bn)
    assert (scale.double() - ws).abs().max().item() <= 1e-6 * ws.abs().max().item()
    assert (shift.double() - wb).abs().max().item() <= 1e-6 * max(1.0, wb.abs().max().item())


def _check(Fold, folded, conv, bn):
    packed, scale, shift = Fold.get(folded, conv, bn)
    assert torch.equal(packed, conv.weight.detach().flatten())
    _close(scale, shift, conv, bn)
    return packed, scale, shift


def test_folds_are_kept_until_a_source_changes(Fold, packs):
    conv, bn = _pair(Fold)
    folded = Fold.new()
    first = _check(Fold, folded, conv, bn)
    again = Fold.get(folded, conv, bn)
    assert len(packs) == 1 and all(a is b for a, b in zip(first, again))         # served from the cache
    bn.eval()
    conv(torch.zeros(*Fold.x))                                                   # reading changes nothing
    assert Fold.get(folded, conv, bn)[0] is first[0] and len(packs) == 1
    with torch.no_grad():
        conv.weight.mul_(2.0)                                                    # an optimizer step does this
    _check(Fold, folded, conv, bn)
    assert len(packs) == 2
    with torch.no_grad():
        bn.running_var.add_(1.0)
    _check(Fold, folded, conv, bn)
    assert len(packs) == 3 and Fold.get(folded, conv, bn)[1] is folded.scale and len(packs) == 3


def test_writes_that_bump_no_version_need_the_epoch_or_the_hand_bump(Fold, packs):
    """What a graph replay (or a kernel writing through a raw pointer) does: the values change, the version
    counters do not.  The cache cannot notice -- that is stated here, not wished away -- and each of the two
    remedies makes exactly the stale fold fresh."""
    conv, bn = _pair(Fold)
    other_conv, other_bn = _pair(Fold)
    folded, other = Fold.new(), Fold.new()
    _check(Fold, folded, conv, bn)
    _check(Fold, other, other_conv, other_bn)
    assert len(packs) == 2
    bn.running_mean.data.add_(3.0)                    # through .data: no version bump, as from a raw pointer
    conv.weight.data.mul_(0.5)
    stale = Fold.get(folded, conv, bn)
    assert len(packs) == 2                            # still the old fold ...
    assert (stale[2].double() - _want(conv, bn)[1]).abs().max().item() > 1.0     # ... of the old statistics
    blocks3d._bump_running_stats(bn)                  # remedy 1: per layer, what the eager BN wrappers call
    _check(Fold, folded, conv, bn)
    assert len(packs) == 3
    Fold.get(other, other_conv, other_bn)
    assert len(packs) == 3                            # ... and only that layer was re-made
    conv.weight.data.mul_(0.5)
    assert Fold.get(folded, conv, bn)[0] is folded.packed and len(packs) == 3
    assert not torch.equal(folded.packed, conv.weight.detach().flatten())
    blocks3d.invalidate_folded_caches()               # remedy 2: global, what GraphedTrainStep calls per replay
    _check(Fold, folded, conv, bn)
    _check(Fold, other, other_conv, other_bn)
    assert len(packs) == 5
    Fold.get(folded, conv, bn), Fold.get(other, other_conv, other_bn)
    assert len(packs) == 5


def test_bump_skips_layers_without_running_statistics(Fold, packs):
    bn = Fold.layers(track_running_stats=False)[1]
    blocks3d._bump_running_stats(bn)                  # nothing to bump, nothing raised
    conv = Fold.layers(bias=True)[0]
    folded = Fold.new()
    packed, scale, shift = Fold.get(folded, conv, None)   # a biased convolution without BN: scale 1, shift bias
    assert torch.equal(scale, torch.ones(Fold.cout)) and torch.equal(shift, conv.bias.detach())
    assert Fold.get(folded, conv, None)[0] is packed and len(packs) == 1


def test_the_names_of_blocks3d_are_those_of_folds():
    for name in ("_versions", "_EPOCH", "invalidate_folded_caches", "_bump_running_stats"):
        assert getattr(blocks3d, name) is getattr(folds, name), name


@pytest.mark.parametrize("case", ["bn without affine", "bn + conv bias", "bias only", "neither"])
def test_fold_affine_against_float64(case):
    torch.manual_seed(5)
    bn = None
    if case.startswith("bn"):
        bn = nn.BatchNorm3d(8, affine=(case != "bn without affine"))
        _randomise(bn)
    conv = nn.Conv3d(4, 8, 3, padding=1, bias=case in ("bn + conv bias", "bias only"))
    with torch.no_grad():
        scale, shift = folds.fold_affine(conv.bias, bn, 8, conv.weight.device)
    if case == "neither":
        assert scale is None and shift is None
    elif case == "bias only":
        assert torch.equal(scale, torch.ones(8)) and torch.equal(shift, conv.bias.detach())
        assert shift.data_ptr() != conv.bias.data_ptr() and not shift.requires_grad       # a copy of its own
    else:
        assert scale.is_contiguous() and shift.is_contiguous() and scale.dtype == shift.dtype == torch.float32
        _close(scale, shift, conv, bn)


def test_the_spp_fold_keeps_its_bits_and_follows_its_sources():
    """``feature_extraction._spp_params``: every row bit-equal to ``scale = weight * rsqrt(var + eps)``,
    ``shift = bias - mean * scale`` (the shared ``fold_affine`` adds ``-mean * scale`` and ``bias`` the other way
    round: the same IEEE sum); served from its cache until a source's version moves."""
    from dsmnet_amd.models.psmnet.submodule import feature_extraction
    torch.manual_seed(7)
    tower = feature_extraction()
    bns = [getattr(tower, "branch%d" % i)[1][1] for i in (4, 3, 2, 1)]
    for bn in bns:
        _randomise(bn)

    def check(params):
        w_t, scale, shift = params
        assert tuple(w_t.shape) == (4, 128, 32) and tuple(scale.shape) == tuple(shift.shape) == (4, 32)
        assert all(t.is_contiguous() for t in params)
        with torch.no_grad():
            for row, bn in enumerate(bns):
                s = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
                assert torch.equal(scale[row], s) and torch.equal(shift[row], bn.bias - bn.running_mean * s), row
    first = tower._spp_params()
    check(first)
    assert all(a is b for a, b in zip(first, tower._spp_params()))              # no bump: the same objects
    with torch.no_grad():
        bns[2].running_var.add_(1.0)
    second = tower._spp_params()
    assert second[1] is not first[1] and not torch.equal(second[1][2], first[1][2])
    assert torch.equal(second[1][0], first[1][0])
    check(second)
    assert all(a is b for a, b in zip(second, tower._spp_params()))
