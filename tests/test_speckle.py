"""CPU: the numpy restatement of the speckle filter (tests/speckle_oracle.py) on hand-made maps and against
scipy's connected components, the stated property of every generated map, and the host side of
dsm_speckle_filter (nothing is launched: the pointers are fake)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dsmnet_amd import _lib, deploy, submit
from dsmnet_amd import costvolume as cv
from tests import speckle_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, I = np.nan, np.inf


def _f(rows):
    return np.array([rows], np.float32)


# ---------------------------------------------------------------------------------------------------
# the oracle, by hand (5x7)
# ---------------------------------------------------------------------------------------------------
def test_hand_made_regions():
    disp = _f([[1, 1, 9, 9, 9, 1, 1],
               [1, 9, 9, 5, 9, 1, 1],
               [9, 9, 5, 5, 9, 9, 9],
               [2, 9, 9, 9, 9, 3, 3],
               [2, 2, 9, 7, 9, 3, 9]])
    size = np.array([[[3, 3, 17, 17, 17, 4, 4],
                      [3, 17, 17, 3, 17, 4, 4],
                      [17, 17, 3, 3, 17, 17, 17],
                      [3, 17, 17, 17, 17, 3, 3],
                      [3, 3, 17, 1, 17, 3, 1]]], np.int32)
    out, keep, got = SO.filter_speckles(disp, 3, 0.0)
    assert got.dtype == np.int32 and keep.dtype == bool and out.dtype == np.float32
    assert np.array_equal(got, size)
    assert np.array_equal(keep, size > 3)                               # size == max_size is a speckle
    assert np.array_equal(out, np.where(size > 3, disp, 0).astype(np.float32))
    assert np.array_equal(SO.filter_speckles(disp, 4, 0.0)[1], size > 4)
    assert SO.filter_speckles(disp, 0, 0.0)[1].all()                    # max_size 0 removes no node
    assert not SO.filter_speckles(disp, 35, 100.0)[1].any()             # one region of 35 is a speckle at 35
    assert np.array_equal(SO.filter_speckles(disp, 34, 100.0)[2], np.full((1, 5, 7), 35))
    out = SO.filter_speckles(disp, 3, 0.0, new_val=-1.0)[0]
    assert np.array_equal(out, np.where(size > 3, disp, -1).astype(np.float32))


def test_hand_made_ramp_is_transitive_and_max_diff_is_inclusive():
    disp = _f([[0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0]] * 5)
    assert np.array_equal(SO.filter_speckles(disp, 0, 0.5)[2], np.full((1, 5, 7), 35))
    below = np.nextafter(np.float32(0.5), np.float32(0))
    assert np.array_equal(SO.filter_speckles(disp, 0, below)[2], np.full((1, 5, 7), 5))
    assert np.array_equal(SO.filter_speckles(disp.transpose(0, 2, 1), 0, below)[2], np.full((1, 7, 5), 5))


def test_hand_made_non_nodes_and_batches():
    disp = _f([[4, 4, N, 4, 4, 4, 4],
               [4, 4, I, 4, 4, 4, 4],
               [4, 4, -I, 4, 4, 4, 4],
               [4, 4, 4, 4, 4, 4, 4],
               [4, 4, 4, 4, 4, 4, 4]])
    valid = np.ones((1, 5, 7), bool)
    valid[0, 3:, 2] = False                                             # the wall goes on to the bottom
    valid[0, 4, 6] = False
    out, keep, size = SO.filter_speckles(disp, 10, 1.0, valid=valid)
    want = np.array([[[10, 10, 0, 19, 19, 19, 19]] * 4 + [[10, 10, 0, 19, 19, 19, 0]]], np.int32)
    assert np.array_equal(size, want)
    assert np.array_equal(keep, want > 10) and np.array_equal(out, np.where(want > 10, 4, 0).astype(np.float32))
    # the value under valid == False is never used
    other = disp.copy()
    other[~valid] = N
    assert all(np.array_equal(a, b) for a, b in zip(SO.filter_speckles(other, 10, 1.0, valid=valid), (out, keep, size)))
    # two images are never joined; (B,1,H,W) keeps its shape
    two = np.full((2, 1, 5, 7), 4, np.float32)
    size = SO.filter_speckles(two, 0, 0.0)[2]
    assert size.shape == (2, 1, 5, 7) and (size == 35).all()


# ---------------------------------------------------------------------------------------------------
# the generators
# ---------------------------------------------------------------------------------------------------
def generated(H, W):
    """name -> (disp, valid, max_diff) of every generator at one shape (max_diff 0.5 where the map leaves it)."""
    c = {"blobs": SO.blobs(H, W, 37), "serpentine": SO.serpentine(H, W), "spiral": SO.spiral(H, W),
         "checker": SO.checker(H, W), "uniform": SO.uniform(H, W), "ramp_joined": SO.ramp(H, W, 0.5, True),
         "ramp_split": SO.ramp(H, W, 0.5, False), "cross": SO.cross(H, W, 16, 64),
         "horseshoe": SO.horseshoe(H, W, 5, 64), "horseshoe_down": SO.horseshoe(H, W, 16, 20, down=True),
         "holes": SO.holes(H, W, 37), "pair": SO.pair(H, W)}
    return {k: (v.disp, v.valid, 0.5 if v.max_diff is None else v.max_diff) for k, v in c.items()}


def test_oracle_against_scipy():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    for name, (disp, valid, md) in generated(33, 65).items():
        p, q, node = SO.edges(disp, valid, md)
        n = disp.size
        g = sparse.coo_matrix((np.ones(len(p)), (p, q)), shape=(n, n))
        _, comp = csgraph.connected_components(g, directed=False)
        comp = comp.reshape(disp.shape)
        cnt = np.bincount(comp[node], minlength=n)
        want = np.where(node, cnt[comp], 0).astype(np.int32)
        assert np.array_equal(SO.filter_speckles(disp, 0, md, valid=valid)[2], want), name


def test_generators_have_their_stated_property():
    H, W = 33, 65
    size = lambda c, md=0.5: SO.filter_speckles(c.disp, 0, c.max_diff if c.max_diff is not None else md, valid=c.valid)[2]
    for md in (0.0, 0.5, 1.0):
        c = SO.blobs(H, W, 37)
        assert [n for _, n in c.info["planted"]] == [37, 38]
        for value, n in c.info["planted"]:
            at = c.disp == np.float32(value)
            assert int(at.sum()) == n and (size(c, md)[at] == n).all(), (md, value)
        keep = SO.filter_speckles(c.disp, 37, md)[1]
        assert not keep[c.disp == 1000].any() and keep[c.disp == 2000].all()
        for c in (SO.serpentine(H, W), SO.spiral(H, W)):
            path = c.info["path"][None]
            assert c.info["size"] == int(path.sum()) > H * W // 3 and (size(c, md)[path] == c.info["size"]).all()
            assert (size(c, md)[~path] < c.info["size"]).all()
        assert (size(SO.checker(H, W), md) == 1).all()
        assert (size(SO.uniform(H, W), md) == H * W).all()
        c = SO.cross(H, W, 16, 63)
        assert c.info["size"] == 5 and (size(c, md)[c.disp == 5] == 5).all() and (size(c, md)[c.disp != 5] == H * W - 5).all()
        assert SO.cross(H, W, 16, 64).info["size"] == 4 and SO.cross(H, W, 32, 64).info["size"] == 3 and SO.cross(H, W, 32, 64).disp[0, 32, 64] == 5
        for c in (SO.horseshoe(H, W, 5, 64), SO.horseshoe(H, W, 16, 20, down=True)):
            assert int((c.disp == 9).sum()) == 9 and (size(c, md)[c.disp == 9] == 9).all()
    assert SO.horseshoe(H, W, 5, 64).disp[0, 5:8, 61:65].tolist() == [[9, 9, 9, 9], [73, 73, 73, 9], [9, 9, 9, 9]]
    assert SO.horseshoe(H, W, 16, 20, down=True).disp[0, 13:17, 20:23].tolist() == \
        [[9, 73, 9], [9, 73, 9], [9, 73, 9], [9, 9, 9]]
    assert (size(SO.ramp(H, W, 0.5, True)) == H * W).all() and (size(SO.ramp(H, W, 0.5, False)) == H).all()
    assert (size(SO.ramp(4, 1030, 0.25, True)) == 4 * 1030).all() and (size(SO.ramp(4, 1030, 0.25, False)) == 4).all()
    c = SO.holes(H, W, 37)
    assert np.isnan(c.info["poisoned"]).sum() > np.isnan(c.info["plain"]).sum() > 0
    assert np.isposinf(c.info["plain"]).any() and np.isneginf(c.info["plain"]).any() and not c.valid.all()
    a = SO.filter_speckles(c.info["poisoned"], 37, 0.5, valid=c.valid)
    b = SO.filter_speckles(c.info["plain"], 37, 0.5, valid=c.valid)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and 0 < a[1].sum() < a[1].size
    c = SO.pair(H, W)
    assert c.disp.shape == (2, H, W) and not np.array_equal(c.disp[0], c.disp[1])
    assert (c.disp[0, -1] == 3).all() and (c.disp[1, 0] == 3).all()
    both = SO.filter_speckles(c.disp, 0, 0.5)[2]
    assert np.array_equal(both[0], SO.filter_speckles(c.disp[:1], 0, 0.5)[2][0])
    assert np.array_equal(both[1], SO.filter_speckles(c.disp[1:], 0, 0.5)[2][0])
    # deterministic
    assert np.array_equal(SO.blobs(H, W, 37).disp, SO.blobs.__wrapped__(H, W, 37).disp)


def test_largest_case_is_quick():
    import time
    c = SO.serpentine(96, 1030)
    t = time.time()
    size = SO.filter_speckles(c.disp, 0, 0.5)[2]
    took = time.time() - t
    assert (size[c.info["path"][None]] == c.info["size"]).all()
    assert took < 5.0, took                                              # about a second; a slow host gets slack


# ---------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------
def _args(**kw):
    a = _lib.SpeckleArgs()
    a.disp, a.valid, a.out, a.keep, a.size, a.workspace = 64, 4096, 8192, 16384, 32768, 65536
    a.B, a.H, a.W, a.max_size, a.max_diff, a.new_val, a.flags = 1, 8, 8, 4, 1.0, 0.0, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_speckle_abi_refusals(hip_lib):
    """Every refusal happens before a launch: the pointers are fake."""
    call = lambda **kw: hip_lib.dsm_speckle_filter(ctypes.byref(_args(**kw)), None)
    assert hip_lib.dsm_speckle_filter(None, None) == -1
    assert call(disp=None) == -1 and call(workspace=None) == -1
    assert call(out=None, keep=None, size=None) == -1                       # nothing asked for
    for name in ("B", "H", "W"):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    assert call(max_size=-1) == -1
    for md in (-1.0, -0.0001, float("nan"), float("inf"), -float("inf")):
        assert call(max_diff=md) == -1, md
    for flags in (1, -1, 256):
        assert call(flags=flags) == -1, flags
    for name in ("disp", "out", "size", "workspace"):
        assert call(**{name: 66}) == -4, name                               # a float or int that is not 4-byte aligned
    assert call(B=1 << 11, H=1 << 10, W=1 << 10) == -2                      # B * H * W = 2^31
    assert call(B=1, H=1 << 16, W=1 << 15) == -2
    assert call(B=1 << 12, H=1 << 10, W=1 << 10) == -2
    assert call(B=0, H=1 << 20, W=1 << 20) == -1                            # the argument checks come first
    assert call(B=1 << 11, H=1 << 10, W=1 << 10, max_size=-1) == -1


def test_speckle_workspace_bytes(hip_lib):
    w = hip_lib.dsm_speckle_workspace_bytes
    assert w(1, 1, 1) == 8 and w(2, 540, 960) == 2 * 540 * 960 * 8
    assert w(0, 4, 4) == 0 and w(1, -1, 4) == 0 and w(1, 4, 0) == 0 and w(-2, -2, 4) == 0
    assert w(1 << 11, 1 << 10, 1 << 10) == 8 << 31                          # size_t arithmetic


def test_struct_size_matches_the_header():
    with open(os.path.join(ROOT, "include", "dsmnet_hip.h")) as fh:
        header = fh.read()
    said = int(re.search(r"sizeof\(dsm_speckle_args\) == (\d+)", header).group(1))
    assert ctypes.sizeof(_lib.SpeckleArgs) == said == 80
    assert _lib.SpeckleArgs.disp.offset == 0 and _lib.SpeckleArgs.workspace.offset == 40
    assert _lib.SpeckleArgs.B.offset == 48 and _lib.SpeckleArgs.flags.offset == 72
    assert int(re.search(r"#define DSM_ABI_VERSION (\d+)", header).group(1)) == 7
    assert "dsm_speckle_filter" in _lib.SIGNATURES and "dsm_speckle_workspace_bytes" in _lib.SIGNATURES


# ---------------------------------------------------------------------------------------------------
# Python entry points without a device
# ---------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    from dsmnet_amd import postprocess
    d, m = torch.ones(1, 1, 4, 6), torch.ones(1, 1, 4, 6, dtype=torch.bool)
    for fn in (lambda: cv.filter_speckles(d, 3, 1.0), lambda: cv.filter_speckles(d[:, 0], 3, 1.0, valid=m[:, 0]),
               lambda: cv.filter_speckles(d, 0, 0.0, want=("size",)),
               lambda: postprocess.remove_speckles(d, 3, 1.0), lambda: postprocess.remove_speckles(d, 3, 1.0, valid=m)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    assert cv.Speckle._fields == ("out", "keep", "size")


def test_bad_arguments_are_refused_before_anything_else():
    d, m = torch.ones(1, 1, 4, 6), torch.ones(1, 1, 4, 6, dtype=torch.bool)
    for bad in (d, m.to(torch.int32), m.to(torch.int8)):
        with pytest.raises(TypeError):
            cv.filter_speckles(d, 3, 1.0, valid=bad)
    for fn in (lambda: cv.filter_speckles(d, 3, 1.0, valid=m[:, 0]),             # shape mismatch
               lambda: cv.filter_speckles(d, 3, 1.0, valid=m[..., :5]),
               lambda: cv.filter_speckles(d, -1, 1.0),
               lambda: cv.filter_speckles(d, 2.5, 1.0),
               lambda: cv.filter_speckles(d, 3, float("nan")),
               lambda: cv.filter_speckles(d, 3, float("inf")),
               lambda: cv.filter_speckles(d, 3, -0.5),
               lambda: cv.filter_speckles(d, 3, 1.0, want=()),
               lambda: cv.filter_speckles(d, 3, 1.0, want=("out", "mask")),
               lambda: cv.filter_speckles(d, 3, 1.0, want=("out", "out"))):
        with pytest.raises(ValueError):
            fn()

    class Stub(torch.nn.Module):
        def forward(self, imL, imR):
            return [0], [imL[:, :1]]

    from dsmnet_amd import postprocess
    with pytest.raises(ValueError, match="pair"):
        postprocess.left_right_check(Stub(), torch.ones(1, 3, 4, 6), torch.ones(1, 3, 4, 6), speckle=200)


def test_deploy_and_submit_parsers():
    for mod in (deploy, submit):
        ap = mod.build_parser()
        assert ap.parse_args([]).speckle is None
        a = ap.parse_args(["--speckle", "200", "1.0", "--lr_check"])
        assert a.speckle == [200.0, 1.0] and a.lr_check is True
        assert deploy.speckle_args(a.speckle) == (200, 1.0) and isinstance(deploy.speckle_args(a.speckle)[0], int)
        with pytest.raises(SystemExit):
            ap.parse_args(["--speckle", "200"])                          # both values are needed
    assert deploy.speckle_args(None) is None and deploy.speckle_args([0.0, 0.0]) == (0, 0.0)
    a = deploy.build_parser().parse_args(["--speckle", "200", "1", "--lr_check", "--fill", "--encode", "kitti16",
                                          "--confidence", "--peak"])
    assert a.speckle == [200.0, 1.0] and a.fill and a.encode == "kitti16" and a.confidence and a.peak
    # refused before anything is loaded: values the filter has no meaning for, and what was refused before
    for argv, what in ((["--speckle", "-1", "1"], "SIZE"), (["--speckle", "2.5", "1"], "SIZE"),
                       (["--speckle", "nan", "1"], "SIZE"), (["--speckle", "200", "-1"], "DIFF"),
                       (["--speckle", "200", "inf"], "DIFF"), (["--speckle", "200", "nan"], "DIFF")):
        for mod in (deploy, submit):
            with pytest.raises(SystemExit, match=what):
                mod.main(argv)
    with pytest.raises(SystemExit, match="--fill needs --lr_check"):
        deploy.main(["--speckle", "200", "1", "--fill"])                 # the fill is the check's, not the filter's
    with pytest.raises(SystemExit, match="--peak cannot be combined with --lr_check"):
        deploy.main(["--speckle", "200", "1", "--peak", "--lr_check"])
