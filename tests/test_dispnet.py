"""CPU: the DispNet model (dsmnet_amd/models/dispnet.py) against tests/golden/golden_dispnet.npz, the outputs of
the reference's models/dispnet.py for this project's seeded weights (tests/golden/make_goldens_dispnet.py).
On CPU tensors every layer takes its stock path."""
import pytest
import torch
import torch.nn as nn

from tests import dispnet_cases as DC


@pytest.fixture(scope="module")
def fixture():
    return DC.Fixture()


@pytest.fixture(scope="module")
def model():
    return DC.build_model()


def test_the_factory_builds_dispnet():
    from dsmnet_amd.models import dict_models, model_create_by_name
    from dsmnet_amd.models.dispnet import dispnet
    assert "dispnet" in dict_models
    m = model_create_by_name("dispnet", 96)
    assert isinstance(m, dispnet)
    assert (m.name, m.D, m.delt, m.count_levels) == ("dispnet", 96, 1e-6, 7)
    assert isinstance(m.upsample, nn.Upsample)


@pytest.mark.parametrize("name", ["dispnet_m1", "dispnetcorr_m1", "dispnetcorr_m2"])
def test_the_m_names_still_raise(name):
    from dsmnet_amd.models import model_create_by_name
    with pytest.raises(AssertionError):
        model_create_by_name(name)


def test_the_state_dict_is_the_checkpoint_contract(fixture, model):
    want = fixture.param_sums()
    sd = model.state_dict()
    assert len(want) == 52 and set(sd.keys()) == set(want.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == want[k][0], k


def test_the_seeded_model_reproduces_the_fixture_parameters(fixture, model):
    for k, v in model.state_dict().items():
        _, s, a = fixture.param_sums()[k]
        got_s, got_a = v.double().sum().item(), v.double().abs().sum().item()
        assert abs(got_s - s) <= 1e-9 * max(a, 1.0) and abs(got_a - a) <= 1e-9 * max(a, 1.0), \
            ("%s: sums (%r, %r), fixture (%r, %r): torch's random generator draws differently from the torch "
             "that wrote the fixture (%s) -- not a model bug" % (k, got_s, got_a, s, a, fixture.meta["torch"]))


def test_initialisation_scales_the_six_heads(model):
    import math
    for lvl, cin in ((6, 1024), (5, 512), (4, 256), (3, 128), (2, 64), (1, 32)):
        w = getattr(model, "pr%d" % lvl).weight
        assert tuple(w.shape) == (1, cin, 3, 3)
        # net_init: N(0, sqrt(2 / (k k Cout))) = sqrt(2 / 9), times 0.1; 288+ samples
        assert 0.5 < w.std().item() / (0.1 * math.sqrt(2.0 / 9.0)) < 1.5, lvl
    assert 0.8 < model.conv2[0].weight.std().item() / math.sqrt(2.0 / (25 * 128)) < 1.2


def test_child_indices_are_the_reference_s(model):
    from dsmnet_amd.models.util_conv import Conv2dReLU
    for name, cin, cout, k, s in (("conv1", 6, 64, 7, 2), ("conv2", 64, 128, 5, 2), ("conv3a", 128, 256, 5, 2),
                                  ("conv3b", 256, 256, 3, 1), ("conv6a", 512, 1024, 3, 2), ("conv6b", 1024, 1024, 3, 1),
                                  ("iconv5", 1025, 512, 3, 1), ("iconv1", 97, 32, 3, 1)):
        layer = getattr(model, name)
        assert isinstance(layer, Conv2dReLU) and isinstance(layer[0], nn.Conv2d) and isinstance(layer[1], nn.ReLU)
        c = layer[0]
        assert (c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding) == \
            (cin, cout, (k, k), (s, s), ((k - 1) // 2,) * 2), name
    for lvl, cin, cout in ((5, 1024, 512), (4, 512, 256), (3, 256, 128), (2, 128, 64), (1, 64, 32)):
        d = getattr(model, "deconv%d" % lvl)
        assert type(d) is nn.Sequential and isinstance(d[0], nn.ConvTranspose2d) and isinstance(d[1], nn.ReLU)
        assert (d[0].in_channels, d[0].out_channels, d[0].kernel_size, d[0].stride) == (cin, cout, (4, 4), (2, 2))
    assert isinstance(model.pr6, nn.Conv2d)


@pytest.mark.parametrize("mode", DC.MODES)
@pytest.mark.parametrize("tag,seed,h,w", DC.CASES)
def test_cpu_forward_matches_the_reference(fixture, model, tag, seed, h, w, mode):
    imL, imR = DC.images(seed, h, w)
    with torch.no_grad():
        scales, outs = model(imL, imR, mode=mode)
    assert scales == [0, 1, 2, 3, 4, 5, 6] and len(outs) == 7
    for i, (got, want) in enumerate(zip(outs, fixture.outputs(tag, mode))):
        assert got.shape == want.shape, (i, got.shape, want.shape)
        err, top = (got - want).abs().max().item(), want.abs().max().item()
        assert err <= 1e-5 * top, "%s %s out%d: %.3e > 1e-5 x %.3e" % (tag, mode, i, err, top)
    if mode == "test":                        # the clamp lands on the LAST output, the coarsest (the reference's quirk)
        with torch.no_grad():
            raw = model(imL, imR, mode="train")[1]
        if tag == "70x150":                   # there the coarsest output has values below delt: the clamp acts
            assert raw[-1].min().item() < model.delt
        assert torch.equal(outs[-1], raw[-1].clamp(model.delt, max(model.D, w)))
        assert all(torch.equal(a, b) for a, b in zip(outs[:-1], raw[:-1]))


def test_mismatched_pair_is_refused(model):
    with pytest.raises(ValueError):
        model(torch.zeros(1, 3, 64, 128), torch.zeros(1, 3, 64, 64))
