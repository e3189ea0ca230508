"""CPU: the float64 restatement of the left-right check (tests/lrcheck_oracle.py) against the fixture made
from the reference's own lines, the hole-fill oracle on rows whose answers are written out here, and the
host side of dsm_lr_check / dsm_fill_background (nothing is launched)."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from dsmnet_amd import _lib, costvolume as cv, deploy
from tests import lrcheck_oracle as LO
from tests.conftest import GOLDEN, ROOT

CASES = ("c2x2", "c5x63", "c3x65", "c4x257", "c6x1030", "c8x64f4")
N = float("nan")


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "golden_lrcheck.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(z["meta"]).decode())
    return d


def test_fixture_holds_the_cases_of_the_issue(fx):
    shapes = [(c["B"], c["H"], c["W"], c["factor"]) for c in (fx["meta"]["cases"][n] for n in CASES)]
    assert shapes == [(1, 2, 2, 1.0), (2, 5, 63, 1.0), (1, 3, 65, 1.0), (2, 4, 257, 1.0), (1, 6, 1030, 1.0),
                      (1, 8, 64, 4.0)]
    assert sorted(fx["meta"]["cases"]) == sorted(CASES) and fx["meta"]["margin"] == 1e-3
    for n in CASES:
        assert 1e-3 >= 8 * fx[n + ".e_ref"].max(), n              # the generator's own condition
        assert 1e-5 <= float(fx[n + ".delt"]) <= 1.1e-4, n         # 1e-4 * (rand + 0.1)


@pytest.mark.parametrize("name", CASES)
def test_restatement_against_the_reference(fx, name):
    c = fx["meta"]["cases"][name]
    disp, other = torch.from_numpy(fx[name + ".disp"]), torch.from_numpy(fx[name + ".other"])
    wrap, weight = torch.from_numpy(fx[name + ".wrap"]), torch.from_numpy(fx[name + ".weight"])
    assert tuple(disp.shape) == (c["B"], 1, c["H"], c["W"]) and wrap.dtype == torch.float32
    r = LO.lr_check(disp, other, float(fx[name + ".delt"]), c["factor"], c["threshold"])
    e_wrap, e_weight = fx[name + ".e_ref"]
    assert float((r.wrap - wrap.double()).abs().max()) <= e_wrap
    assert float((r.weight - weight.double()).abs().max()) <= e_weight
    # the mask is the thresholding of the REFERENCE's delta (loss.py:394, float32) plus the inside test
    delta32 = (disp - wrap).abs() / c["factor"]
    inside = (r.ix >= 0) & (r.ix <= c["W"] - 1)
    assert torch.equal(r.mask, (delta32 < c["threshold"]) & inside)
    assert torch.equal(r.masked, disp * r.mask)
    # the margin the GPU test relies on
    for edge in (c["threshold"], 1.0, 3.0):
        assert float((r.delta - edge).abs().min()) >= 1e-3
    assert float(torch.minimum(r.ix.abs(), (r.ix - (c["W"] - 1)).abs()).min()) >= 1e-3
    if c["H"] * c["W"] > 4:
        assert r.mask.any() and not r.mask.all() and not inside.all()
        assert ((r.weight > 0.01) & (r.weight < 1)).any()         # the ramp of weight_common is reached


def test_restatement_frames_and_shapes(fx):
    disp, other = torch.from_numpy(fx["c5x63.disp"]), torch.from_numpy(fx["c5x63.other"])
    a = LO.lr_check(disp, other, 0.0)
    b = LO.lr_check(disp, other.flip(-1), 0.0, mirrored=False)
    c = LO.lr_check(disp[:, 0], other[:, 0], 0.0)
    for k in range(4):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k][:, 0], c[k])
    assert c.mask.shape == (2, 5, 63) and a.mask.dtype == torch.bool


def test_restatement_on_the_known_scene():
    dL, dR = LO.known_scene()
    left = LO.lr_check(dL, dR, 0.0, mirrored=False)
    right = LO.lr_check(dR.flip(-1), dL, 0.0)                       # in the mirrored frame (loss.py:452)
    LO.check_known_scene(left.mask, right.mask.flip(-1))
    assert not left.mask[0, 0, :, :5].any() and not right.mask.flip(-1)[0, 0, :, 91:].any()   # sampled outside


# the fill oracle on rows whose answers are written out: (values, valid, answer); N marks a value that
# must never be read
ROWS = {
    "middle": ([5, N, N, 3, 7], [1, 0, 0, 1, 1], [5, 3, 3, 3, 7]),
    "middle_left_smaller": ([2, N, 9], [1, 0, 1], [2, 2, 9]),
    "borders": ([N, N, 4, 6, N], [0, 0, 1, 1, 0], [4, 4, 4, 6, 6]),
    "single": ([N, N, 8, N], [0, 0, 1, 0], [8, 8, 8, 8]),
    "all_valid": ([1, 2, 3], [1, 1, 1], [1, 2, 3]),
    "two_runs": ([N, 5, N, 2, N, N, 9, N], [0, 1, 0, 1, 0, 0, 1, 0], [5, 5, 2, 2, 2, 2, 9, 9]),
}


def _np(rows):
    return np.array(rows, dtype=np.float32)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_fill_oracle_rows(name):
    v, m, want = ROWS[name]
    got = LO.fill_background(_np([[v]]), np.array([[m]], dtype=bool))
    assert got.dtype == np.float32 and np.array_equal(got, _np([[want]]))


def test_fill_oracle_empty_rows_and_images():
    e, z = [N, N, N], [0, 0, 0]
    disp = _np([[e, e, [4, N, 6], e, e, [N, 5, N], e]])
    mask = np.array([[z, z, [1, 0, 1], z, z, [0, 1, 0], z]], dtype=bool)
    want = _np([[[4, 4, 6], [4, 4, 6], [4, 4, 6], [4, 4, 5], [4, 4, 5], [5, 5, 5], [5, 5, 5]]])
    assert np.array_equal(LO.fill_background(disp, mask), want)          # top, middle, bottom
    # an empty image gives zeros, and does not disturb its neighbour in the batch
    both = LO.fill_background(np.concatenate([np.full_like(disp, N), disp]), np.concatenate([np.zeros_like(mask), mask]))
    assert np.array_equal(both[0], np.zeros((7, 3), np.float32)) and np.array_equal(both[1], want[0])
    # fminf: a NaN in a VALID pixel loses against a number
    got = LO.fill_background(_np([[[N, 0, 3]]]), np.array([[[1, 0, 1]]], dtype=bool))
    assert math.isnan(got[0, 0, 0]) and got[0, 0, 1] == 3 and got[0, 0, 2] == 3


def _args(**kw):
    a = _lib.LrcheckArgs()
    a.disp = a.other = a.wrap = a.weight = a.mask = a.masked = 64
    a.B, a.H, a.W, a.delt, a.factor, a.threshold, a.flags = 1, 8, 8, 0.0, 1.0, 1.0, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_lr_check_abi_refusals(hip_lib):
    """Every refusal happens before a launch: the pointers are fake."""
    call = lambda **kw: hip_lib.dsm_lr_check(ctypes.byref(_args(**kw)), None)
    assert hip_lib.dsm_lr_check(None, None) == -1
    assert call(disp=None) == -1 and call(other=None) == -1
    assert call(wrap=None, weight=None, mask=None, masked=None) == -1     # nothing asked for
    for name in ("B", "H", "W"):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    assert call(H=1) == -1 and call(W=1) == -1                              # imwrap.py:48
    for factor in (0.0, -1.0, float("nan")):
        assert call(factor=factor) == -1, factor
    for thr in (float("nan"), float("inf"), -float("inf")):
        assert call(threshold=thr) == -1, thr
    for flags in (2, 3, -1, 256):
        assert call(flags=flags) == -1, flags
    for name in ("disp", "other", "wrap", "weight", "masked"):
        assert call(**{name: 66}) == -4, name                               # not 4-byte aligned
    assert call(B=1 << 20, H=4096, W=4096) == -2                            # 2^34 tiles: past the grid's x extent
    assert call(B=0, H=1 << 20) == -1                                       # the argument checks come first


def test_fill_background_abi_refusals(hip_lib):
    f = lambda disp=64, mask=4096, out=8192, ws=1024, B=1, H=4, W=8: hip_lib.dsm_fill_background(disp, mask, out, ws, B, H, W, None)
    for name in ("disp", "mask", "out", "ws"):
        assert f(**{name: None}) == -1, name
    for name in ("B", "H", "W"):
        assert f(**{name: 0}) == -1 and f(**{name: -1}) == -1, name
    assert f(out=64) == -1                                                  # out aliases disp
    assert f(disp=8192 + 4 * 31) == -1 and f(disp=8192 - 4 * 31) == -1      # one element shared
    assert f(mask=8192 + 127) == -1 and f(ws=8192) == -1
    assert f(disp=66) == -4 and f(out=8194) == -4 and f(ws=1026) == -4
    assert f(B=1 << 16, H=1 << 16, W=1) == -2
    w = hip_lib.dsm_fill_background_workspace_bytes
    assert w(1, 1, 1) == 4 and w(2, 540, 960) == 2 * 540 * 4 and w(0, 4, 4) == 0 and w(1, -1, 4) == 0 and w(1, 4, 0) == 0


def test_struct_size_matches_the_header():
    with open(os.path.join(ROOT, "include", "dsmnet_hip.h")) as fh:
        header = fh.read()
    said = int(re.search(r"sizeof\(dsm_lrcheck_args\) == (\d+)", header).group(1))
    assert ctypes.sizeof(_lib.LrcheckArgs) == said == 80
    assert int(re.search(r"#define DSM_LRCHECK_OTHER_RIGHT_FRAME (\d+)", header).group(1)) == _lib.DSM_LRCHECK_OTHER_RIGHT_FRAME
    assert int(re.search(r"#define DSM_ABI_VERSION (\d+)", header).group(1)) == 7


def test_cpu_tensors_are_refused():
    from dsmnet_amd import postprocess
    d, m = torch.ones(1, 1, 4, 6), torch.ones(1, 1, 4, 6, dtype=torch.bool)
    for fn in (lambda: cv.lr_check(d, d), lambda: cv.lr_check(d[:, 0], d[:, 0], mirrored=False),
               lambda: cv.fill_background(d, m), lambda: cv.fill_background(d[:, 0], m[:, 0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()

    class Stub(torch.nn.Module):
        def forward(self, imL, imR):
            return [0], [imL[:, :1]]

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        postprocess.left_right_check(Stub(), torch.ones(1, 3, 4, 6), torch.ones(1, 3, 4, 6))
    assert cv.LRCheck._fields == ("wrap", "weight", "mask", "masked")


def test_deploy_parser():
    ap = deploy.build_parser()
    old = ap.parse_args([])
    assert (old.net, old.maxdisparity, old.path_weight, old.path_left, old.path_right) == \
        ("dispnetcorr", 192, "", "10L.png", "10R.png")
    assert old.flip is False and old.out is None and old.path_disp_gt is None
    assert old.lr_check is False and old.fill is False and old.lr_threshold == 1.0
    new = ap.parse_args(["--lr_check", "--lr_threshold", "2.5", "--fill", "--flip", "1", "--net", "psmnet"])
    assert new.lr_check is True and new.fill is True and new.lr_threshold == 2.5 and new.flip is True
    assert new.net == "psmnet"
