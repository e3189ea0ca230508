"""CPU: the options ``warp_train`` / ``decoder_train`` exist, default to off and leave CPU tensors on the stock
ops; the two backward exports are declared in the header and bound in ``_lib``."""
import os
import re

import torch
import torch.nn as nn

from dsmnet_amd import _lib
from dsmnet_amd import costvolume as cv
from tests.helpers import seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_exist_and_default_to_off():
    for name in ("warp_train", "decoder_train"):
        assert cv.get_option(name) is False
        assert cv.set_option(name, True) is False
        assert cv.get_option(name) is True
        assert cv.set_option(name, False) is True
        assert cv.get_option(name) is False
    assert "warp_train" in cv.set_option.__doc__ and "decoder_train" in cv.set_option.__doc__
    assert "DSM_WARP_TRAIN" in cv.set_option.__doc__ and "DSM_DECODER_TRAIN" in cv.set_option.__doc__


def test_the_options_are_independent():
    old = cv.set_option("warp_train", True)
    try:
        assert cv.get_option("decoder_train") is False
    finally:
        cv.set_option("warp_train", old)


def _level(on):
    torch.manual_seed(3)
    deconv = nn.Sequential(nn.ConvTranspose2d(4, 3, 4, 2, 1, bias=True), nn.ReLU(inplace=True))
    x, pr, skip = (t.requires_grad_(True) for t in (seeded(1, 2, 4, 3, 5), seeded(2, 2, 1, 3, 5), seeded(3, 2, 2, 5, 9)))
    old = (cv.set_option("warp_train", on), cv.set_option("decoder_train", on))
    try:
        out = cv.decoder_level(deconv, x, pr, skip)
        grads = torch.autograd.grad(out, [x, pr, skip] + list(deconv.parameters()), seeded(4, *out.shape))
    finally:
        cv.set_option("warp_train", old[0])
        cv.set_option("decoder_train", old[1])
    return (out.detach(),) + grads


def _iresnet_error(on):
    """``models.iresnet.recon_error``: the lines of ``iresnet.forward`` that choose between the fused warp and
    ``imwrap_BCHW``."""
    from dsmnet_amd.models import iresnet as M
    stemL, stemR = seeded(5, 1, 4, 6, 9).requires_grad_(True), seeded(6, 1, 4, 6, 9).requires_grad_(True)
    pr0 = seeded(7, 1, 1, 6, 9).requires_grad_(True)
    old = (cv.set_option("warp_train", on), cv.set_option("decoder_train", on))
    try:
        torch.manual_seed(9)
        err = M.recon_error(stemL, stemR, pr0)
        grads = torch.autograd.grad(err, [stemL, stemR, pr0], seeded(8, *err.shape))
        after = torch.rand(1)                        # the generator advanced by exactly one draw
    finally:
        cv.set_option("warp_train", old[0])
        cv.set_option("decoder_train", old[1])
    torch.manual_seed(9)
    torch.rand(1)
    assert torch.equal(after, torch.rand(1))
    return (err.detach(), after) + grads


def test_cpu_tensors_never_reach_the_library():
    for fn in (_level, _iresnet_error):
        for a, b in zip(fn(False), fn(True)):
            assert torch.equal(a, b)


def test_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dsmnet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("dsm_warp_abs_error_bwd", "dsm_decoder_cat_bwd"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dsm_warp_abs_error_bwd"][1]) == 15
    assert len(_lib.SIGNATURES["dsm_decoder_cat_bwd"][1]) == 18
    assert "#define DSM_ABI_VERSION 7" in header
