"""GPU: the speckle filter (csrc/speckle.hip; costvolume.filter_speckles, postprocess.remove_speckles,
left_right_check(speckle=), submit(speckle=)) against tests/speckle_oracle.py.

Everything is exact: ``keep`` and ``size`` are compared with ``torch.equal``, ``out`` bit for bit through its
int32 view.  There is no tolerance anywhere.

The kernels label tiles of TH x TW = 16 x 64 pixels (a wave per row), so the shapes are those around one,
two and four tiles in each direction -- TH - 1, TH, TH + 1 = 15, 16, 17 and TW - 1, TW, TW + 1 = 63, 64, 65
are in the lists, as are their doubles -- plus the degenerate 1 and 2, and 96 x 1030 for many tiles with
W % 4 != 0.  ``cross`` and ``horseshoe`` are placed from TH and TW."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

from tests import speckle_oracle as SO

pytestmark = pytest.mark.gpu

TH, TW = 16, 64
HEIGHTS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 65)
WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
# every height and every width twice: height i with widths i and i + 5
SHAPES = sorted({(HEIGHTS[i], WIDTHS[(i + s) % 12]) for i in range(12) for s in (0, 5)}) + [(96, 1030)]
MAX_DIFFS = (0.0, 0.5, 1.0)
NEW_VALS = (0.0, -1.0)


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


def same(a, b):
    """Bit for bit (NaN-safe: compares the representation)."""
    if a.dtype == torch.bool:
        return torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def planted_size(H, W):
    return max(1, min(37, H * W // 4))


@functools.lru_cache(maxsize=None)
def sizes_of(key, md):
    """The oracle's (size, node) of a named case: computed once, shared, never modified."""
    c = case(key)
    _, keep, size = SO.filter_speckles(c.disp, 0, md, valid=c.valid)
    return size, keep


@functools.lru_cache(maxsize=None)
def case(key):
    name, H, W = key[:3]
    if name == "blobs":
        return SO.blobs(H, W, planted_size(H, W))
    if name == "holes":
        return SO.holes(H, W, planted_size(H, W))
    if name == "holes_plain":
        c = SO.holes(H, W, planted_size(H, W))
        return c._replace(disp=c.info["plain"])
    if name in ("serpentine", "spiral", "checker", "uniform", "pair"):
        return getattr(SO, name)(H, W)
    if name == "ramp":
        return SO.ramp(H, W, key[3], key[4])
    if name == "cross":
        return SO.cross(H, W, key[3], key[4])
    if name == "horseshoe":
        return SO.horseshoe(H, W, key[3], key[4], down=key[5])
    raise KeyError(name)


def expected(key, md, max_size, new_val):
    c = case(key)
    size, node = sizes_of(key, md)
    keep = node & (size > max_size)
    return np.where(keep, c.disp, np.float32(new_val)).astype(np.float32), keep, size


def run(cv, key, md, max_size, new_val=0.0, want=("out", "keep", "size")):
    c = case(key)
    d = torch.from_numpy(c.disp).cuda()
    v = None if c.valid is None else torch.from_numpy(c.valid).cuda()
    before = d.clone()
    got = cv.filter_speckles(d, max_size, md, valid=v, new_val=new_val, want=want)
    torch.cuda.synchronize()
    assert same(d, before)                                               # the input is not written
    return got


def check(cv, key, md, max_size, new_val=0.0):
    got = run(cv, key, md, max_size, new_val)
    out, keep, size = expected(key, md, max_size, new_val)
    what = (key, md, max_size, new_val)
    assert got.size.dtype == torch.int32 and got.keep.dtype == torch.bool and got.out.dtype == torch.float32
    assert torch.equal(got.size.cpu(), torch.from_numpy(size)), what
    assert torch.equal(got.keep.cpu(), torch.from_numpy(keep)), what
    assert same(got.out.cpu(), torch.from_numpy(out)), what
    return got


def keys_at(H, W):
    """Every generator at one shape; cross and horseshoe where tiles meet (or as near as the shape allows)."""
    keys = [("blobs", H, W), ("holes", H, W), ("pair", H, W), ("serpentine", H, W), ("spiral", H, W),
            ("checker", H, W), ("uniform", H, W), ("ramp", H, W, 0.5, True), ("ramp", H, W, 0.5, False),
            ("ramp", H, W, 0.25, True), ("ramp", H, W, 1.0, False),
            ("cross", H, W, min(TH, H - 1), min(TW, W - 1))]
    if W > TW and H >= 3:
        keys.append(("horseshoe", H, W, min(TH - 2, H - 3), TW, False))      # the arms straddle a tile row too
    if H > TH and W >= 3:
        keys.append(("horseshoe", H, W, TH, min(TW - 2, W - 3), True))
    return keys


@pytest.mark.parametrize("H,W", SHAPES, ids=lambda v: str(v))
def test_every_generator_at_shape(cv, H, W):
    turn = itertools.count(H + W)
    for key in keys_at(H, W):
        c = case(key)
        if c.max_diff is not None:
            mds = (c.max_diff,)
        elif key[0] in ("blobs", "holes", "pair"):
            mds = MAX_DIFFS                                              # the texture makes all three differ
        else:
            mds = (MAX_DIFFS[next(turn) % 3],)
        for md in mds:
            for max_size in sorted({0, 1, planted_size(H, W), H * W - 1, H * W}):
                check(cv, key, md, max_size, NEW_VALS[next(turn) % 2])
    c, p = case(("blobs", H, W)), planted_size(H, W)
    assert len(c.info["planted"]) == 2 or H < 17 or W < 32               # both planted regions fit in the larger maps
    if len(c.info["planted"]) == 2:                                      # one goes, one stays
        assert [n for _, n in c.info["planted"]] == [p, p + 1]
        keep = run(cv, ("blobs", H, W), 0.5, p).keep.cpu().numpy()
        assert not keep[c.disp == 1000].any() and keep[c.disp == 2000].all()


def test_holes_values_under_invalid_pixels_are_never_used(cv):
    for H, W in ((17, 65), (33, 129)):
        for md in MAX_DIFFS:
            a = check(cv, ("holes", H, W), md, 5)
            b = check(cv, ("holes_plain", H, W), md, 5)
            assert all(same(x, y) for x, y in zip(a, b))
            assert bool(torch.isfinite(a.out).all()) and int(a.keep.sum()) < a.keep.numel()
            assert md < 1.0 or int(a.keep.sum()) > 0                     # the case is not empty


@pytest.mark.parametrize("H,W", ((65, 257), (96, 1030)))
def test_long_paths(cv, H, W):
    """The deepest trees: one region along a path through every tile."""
    for name in ("serpentine", "spiral"):
        c = case((name, H, W))
        n = c.info["size"]
        got = check(cv, (name, H, W), 0.5, n - 1, -1.0)
        path = torch.from_numpy(c.info["path"][None])
        assert bool((got.size.cpu()[path] == n).all()) and torch.equal(got.keep.cpu(), path)
        assert not run(cv, (name, H, W), 1.0, n, want=("keep",)).keep.any()


@pytest.mark.parametrize("H,W", ((33, 129), (96, 1030)))
def test_cross_and_horseshoe_where_tiles_meet(cv, H, W):
    nty, ntx = -(-H // TH), -(-W // TW)
    corners = {(TH, TW), ((nty - 1) * TH, (ntx - 1) * TW)}               # interior; at the last, partial tile
    for cy, cx in sorted(corners):
        for dy, dx in ((0, 0), (-1, -1), (0, -1), (-1, 0)):              # each of the four pixels at the corner
            key = ("cross", H, W, cy + dy, cx + dx)
            n = case(key).info["size"]
            for max_size in (n - 1, n):
                got = check(cv, key, 0.5, max_size)
            assert not got.keep.cpu()[torch.from_numpy(case(key).disp == 5)].any()   # at max_size = n it goes
            assert int(got.keep.sum()) >= H * W - n - 1                  # at the image's corner it cuts one pixel off
        for key in (("horseshoe", H, W, cy - 2, cx, False), ("horseshoe", H, W, min(cy, H - 3), cx, False),
                    ("horseshoe", H, W, cy, cx - 2, True), ("horseshoe", H, W, cy, min(cx, W - 3), True)):
            for max_size in (8, 9):
                got = check(cv, key, 1.0, max_size, -1.0)
            assert int(got.keep.sum()) == H * W - 9
            nine = torch.from_numpy(case(key).disp == 9)
            assert bool((run(cv, key, 0.0, 0, want=("size",)).size.cpu()[nine] == 9).all())


def test_each_output_alone(cv):
    for key, md, ms in ((("holes", 17, 65), 0.5, 5), (("blobs", 33, 129), 1.0, 37)):
        full = run(cv, key, md, ms, -1.0)
        for n in range(1, 4):
            for names in itertools.combinations(cv.Speckle._fields, n):
                got = run(cv, key, md, ms, -1.0, want=names)
                for f in cv.Speckle._fields:
                    if f in names:
                        assert same(getattr(got, f), getattr(full, f)), (names, f)
                    else:
                        assert getattr(got, f) is None, (names, f)
    d = torch.ones(1, 4, 4, device="cuda")
    for bad in ((), ("out", "mask")):
        with pytest.raises(ValueError):
            cv.filter_speckles(d, 1, 1.0, want=bad)


@pytest.mark.parametrize("H,W", ((16, 64), (17, 63)))
def test_base_offset_by_one_element(cv, H, W):
    """disp at data_ptr() % 16 == 4, valid at an odd byte address."""
    key = ("holes", H, W)
    c = case(key)
    buf = torch.empty(c.disp.size + 1, device="cuda")
    d = buf[1:].view(c.disp.shape)
    d.copy_(torch.from_numpy(c.disp))
    vbuf = torch.empty(c.valid.size + 1, device="cuda", dtype=torch.bool)
    v = vbuf[1:].view(c.valid.shape)
    v.copy_(torch.from_numpy(c.valid))
    assert d.data_ptr() % 16 == 4 and d.is_contiguous() and v.data_ptr() % 2 == 1 and v.is_contiguous()
    got = cv.filter_speckles(d, 5, 0.5, valid=v, want=cv.Speckle._fields)
    for a, b in zip(got, expected(key, 0.5, 5, 0.0)):
        assert same(a.cpu(), torch.from_numpy(b))


def test_map_ranks_and_mask_dtypes(cv):
    key = ("holes", 17, 65)
    c = case(key)
    want = [torch.from_numpy(a) for a in expected(key, 0.5, 5, 0.0)]
    d = torch.from_numpy(c.disp).cuda()
    vb = torch.from_numpy(c.valid).cuda()
    vu = torch.from_numpy(c.valid.astype(np.uint8) * 255).cuda()
    for v in (vb, vu):
        got3 = cv.filter_speckles(d, 5, 0.5, valid=v, want=cv.Speckle._fields)
        got4 = cv.filter_speckles(d.unsqueeze(1), 5, 0.5, valid=v.unsqueeze(1), want=cv.Speckle._fields)
        for a3, a4, b in zip(got3, got4, want):
            assert a3.shape == (1, 17, 65) and a4.shape == (1, 1, 17, 65)
            assert same(a3.cpu(), b) and same(a4[:, 0].cpu(), b)
    # B = 2 as (B,1,H,W)
    key = ("pair", 33, 65)
    got = cv.filter_speckles(torch.from_numpy(case(key).disp).cuda().unsqueeze(1), 9, 0.5, want=cv.Speckle._fields)
    for a, b in zip(got, expected(key, 0.5, 9, 0.0)):
        assert a.shape == (2, 1, 33, 65) and same(a[:, 0].cpu(), torch.from_numpy(b))
    from dsmnet_amd.postprocess import remove_speckles
    out, keep = remove_speckles(d, 5, 0.5, valid=vb)
    assert same(out.cpu(), want[0]) and torch.equal(keep.cpu(), want[1])
    with pytest.raises(ValueError):
        cv.filter_speckles(d.unsqueeze(1), 5, 0.5, valid=vb)
    with pytest.raises(TypeError):
        cv.filter_speckles(d, 5, 0.5, valid=d)


def test_dirty_workspace(cv):
    """uniform, then checker of the same shape at once: the allocator hands the same block back."""
    H, W = 33, 129
    for first, second in ((("uniform", H, W), ("checker", H, W)), (("checker", H, W), ("uniform", H, W))):
        run(cv, first, 0.5, 1)
        check(cv, second, 0.5, 1)
        check(cv, second, 0.5, H * W - 1)


def test_three_runs_give_the_same_bits(cv):
    key = ("blobs", 96, 1030)
    runs = [run(cv, key, 0.5, 37, -1.0) for _ in range(3)]
    for r in runs[1:]:
        assert all(same(a, b) for a, b in zip(r, runs[0]))
    for a, b in zip(runs[0], expected(key, 0.5, 37, -1.0)):
        assert same(a.cpu(), torch.from_numpy(b))


def test_replayed_graph_follows_its_inputs(cv):
    H, W = 33, 129
    first, second = ("holes", H, W), ("serpentine", H, W)
    static_d = torch.from_numpy(case(first).disp).cuda()
    static_v = torch.from_numpy(case(first).valid).cuda()

    def step():
        return cv.filter_speckles(static_d, 9, 0.5, valid=static_v, new_val=-1.0, want=cv.Speckle._fields)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    seen = []
    for key in (second, first, second):
        c = case(key)
        static_d.copy_(torch.from_numpy(c.disp))
        static_v.copy_(torch.ones(c.disp.shape, dtype=torch.bool) if c.valid is None else torch.from_numpy(c.valid))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, expected(key, 0.5, 9, -1.0)):
            assert same(a.cpu(), torch.from_numpy(b)), key
        seen.append(out.size.cpu().clone())
    assert not torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2])


# ---------------------------------------------------------------------------------------------------
# the users' entry points
# ---------------------------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    """A fixed, asymmetric, piecewise-constant function of the two images (levels 0.5 apart), in the return
    convention ``kind`` names -- the pattern of test_lrcheck_gpu.py's stub."""

    def __init__(self, kind="bchw"):
        super(Stub, self).__init__()
        self.kind, self.calls = kind, 0

    @staticmethod
    def fn(imL, imR):
        return torch.floor((3.0 + 2.0 * imL[:, 0:1] + imR[:, 1:2] - 0.5 * imL[:, 2:3] * imR[:, 0:1]) * 2.0) * 0.5

    def forward(self, imL, imR, mode="test"):
        self.calls += 1
        d = self.fn(imL, imR)
        if self.kind == "lr":
            return d, self.fn(imR.flip(-1), imL.flip(-1)).flip(-1)
        return [0], [d[:, 0] if self.kind == "bhw" else d]


@pytest.mark.parametrize("kind", ("bchw", "bhw", "lr"))
def test_left_right_check_with_speckle(cv, kind):
    from dsmnet_amd.postprocess import left_right_check
    g = torch.Generator().manual_seed(79)
    imL, imR = torch.rand(2, 3, 18, 70, generator=g).cuda(), torch.rand(2, 3, 18, 70, generator=g).cuda()
    model = Stub(kind)
    plain = left_right_check(model, imL, imR, threshold=1.25)
    assert sorted(plain) == ["dispL", "dispR", "filledL", "filledR", "maskL", "maskR", "weightL", "weightR"]
    res = left_right_check(model, imL, imR, threshold=1.25, speckle=(3, 0.5))
    assert sorted(res) == sorted(list(plain) + ["keepL", "keepR"])
    for k in plain:
        if not k.startswith("filled"):
            assert same(res[k], plain[k]), k                             # the check's own results are untouched
    for side, flip in (("L", False), ("R", True)):
        d, mask, keep = res["disp" + side], res["mask" + side], res["keep" + side]
        if flip:                                                         # the right view is filtered mirrored
            d, mask, keep = d.flip(-1), mask.flip(-1), keep.flip(-1)
        plane = lambda t: t.cpu().numpy().reshape(2, 18, 70)
        want = SO.filter_speckles(plane(d), 3, 0.5, valid=plane(mask))[1]
        assert keep.dtype == torch.bool and keep.shape == d.shape
        assert np.array_equal(plane(keep), plane(mask) & want)
        assert 0 < int(keep.sum()) < int(mask.sum()) < mask.numel()      # the filter removed something
        filled = cv.fill_background(d.contiguous(), keep.contiguous())
        assert same(res["filled" + side], filled.flip(-1) if flip else filled)
    assert sorted(left_right_check(model, imL, imR, fill=False, speckle=(3, 0.5))) == \
        ["dispL", "dispR", "keepL", "keepR", "maskL", "maskR", "weightL", "weightR"]


def _read(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


def test_submit_with_speckle(cv, tmp_path):
    from dsmnet_amd import transforms
    from dsmnet_amd.datasets import Dataset_stereo
    from dsmnet_amd.submit import submit
    from tests.dataset_trees import write_kitti
    root = str(tmp_path / "kitti")
    samples = write_kitti(root, sizes=((19, 45),) * 2, seed=9)
    sub = os.path.join(root, "data_scene_flow", "training")
    names = ["%06d_10.png" % i for i in range(2)]
    ds = Dataset_stereo(*[[os.path.join(sub, folder, n) for n in names] for folder in ("image_2", "image_3", "disp_occ_0")])
    out = str(tmp_path / "submit" / "speckle")
    submit(Stub().cuda(), ds, out, batch_size=2, pad_multiple=16, formats=("u16",), speckle=(3, 0.5))
    out_lr = str(tmp_path / "submit" / "speckle_lr")
    submit(Stub().cuda(), ds, out_lr, batch_size=2, pad_multiple=16, formats=("u16",), lr_check=True, speckle=(3, 0.5))
    norm = transforms.Stereo_normalize()
    for i, (imL, imR, _) in enumerate(samples):
        chw = lambda a: torch.from_numpy(a.astype(np.float32).transpose(2, 0, 1)[None] / np.float32(255.0))
        seen = norm(torch.cat([chw(imL), chw(imR)], 1).contiguous().cuda())
        seen = torch.nn.functional.pad(seen, (0, 3, 13, 0))              # 19 x 45 to multiples of 16: top, right
        pred = Stub.fn(seen[:, :3], seen[:, 3:6])
        keep = SO.filter_speckles(pred.cpu().numpy(), 3, 0.5)[1][0, 0, 13:, :45]
        q = _read(os.path.join(out, "u16", names[i]))
        assert q.shape == (19, 45) and np.array_equal(q == 0, ~keep) and 0 < keep.sum() < keep.size
        # with the check: among the consistent pixels
        predR = Stub.fn(seen[:, 3:6].flip(-1), seen[:, :3].flip(-1))
        mask = cv.lr_check(pred, predR, want=("mask",)).mask.cpu().numpy()
        keep = (mask & SO.filter_speckles(pred.cpu().numpy(), 3, 0.5, valid=mask)[1])[0, 0, 13:, :45]
        q = _read(os.path.join(out_lr, "u16", names[i]))
        assert np.array_equal(q == 0, ~keep)
