"""GPU: the left-right check and the hole fill (csrc/lrcheck.hip; costvolume.lr_check, fill_background,
postprocess.left_right_check) against tests/lrcheck_oracle.py.

``wrap`` and ``weight`` are held to 4 * E_ref of the float64 restatement, E_ref being the reference's OWN
float32 error against it, stored per case in the fixture: the device evaluates the same float32 formulas,
but the compiler may contract multiply-adds and order the four taps' sum differently, a few ulps of the
same quantities that make up E_ref.  ``mask`` must be EXACTLY equal: the fixture keeps every delta 1e-3 away
from the threshold (and from 1 and 3) and every sample position 1e-3 away from 0 and W - 1, and
1e-3 >= 8 * E_ref.  ``masked`` is ``disp * mask`` bit for bit.  The fill selects and takes fminf of float32
values, which is exact: it must equal the numpy loops bit for bit.

Shapes are the smallest that reach each branch: the golden cases cover W % 4 != 0 (63, 65, 257, 1030), the
vector path (64), one tile and several, B = 2; the fill runs at the widths around a wave (63, 64, 65) and a
256-column chunk (256, 257), several chunks (1030) and the degenerate 1 and 2."""
import functools
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests import lrcheck_oracle as LO
from tests.conftest import GOLDEN
from tests.test_lrcheck import CASES, ROWS

pytestmark = pytest.mark.gpu

FIELDS = ("wrap", "weight", "mask", "masked")


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(GOLDEN, "golden_lrcheck.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(z["meta"]).decode())
    return d


@functools.lru_cache(maxsize=None)
def case(name):
    """(disp, other, kwargs, e_ref) on the CPU; computed once and never modified."""
    fx = golden()
    c = fx["meta"]["cases"][name]
    kw = {"delt": float(fx[name + ".delt"]), "factor": c["factor"], "threshold": c["threshold"]}
    return torch.from_numpy(fx[name + ".disp"]), torch.from_numpy(fx[name + ".other"]), kw, fx[name + ".e_ref"]


@functools.lru_cache(maxsize=None)
def oracle(name):
    disp, other, kw, _ = case(name)
    return LO.lr_check(disp, other, **kw)


@functools.lru_cache(maxsize=None)
def device_result(name):
    """The full result of a golden case on the device, on the CPU: the yardstick of the bit-for-bit tests."""
    from dsmnet_amd import costvolume
    disp, other, kw, _ = case(name)
    r = costvolume.lr_check(disp.cuda(), other.cuda(), **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in r)


def same(a, b):
    """Bit for bit (NaN-safe: compares the representation)."""
    if a.dtype == torch.bool:
        return torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(cv, name):
    disp, other, kw, (e_wrap, e_weight) = case(name)
    want = oracle(name)
    got = cv.LRCheck(*device_result(name))
    assert got.wrap.dtype == torch.float32 and got.mask.dtype == torch.bool and got.mask.shape == disp.shape
    err_wrap = float((got.wrap.double() - want.wrap).abs().max())
    err_weight = float((got.weight.double() - want.weight).abs().max())
    print("%s: wrap err %.3e (E_ref %.3e, bound %.3e)  weight err %.3e (E_ref %.3e, bound %.3e)  mask differs at %d"
          % (name, err_wrap, e_wrap, 4 * e_wrap, err_weight, e_weight, 4 * e_weight, int((got.mask != want.mask).sum())))
    assert err_wrap <= 4 * e_wrap
    assert err_weight <= 4 * e_weight
    assert torch.equal(got.mask, want.mask)
    assert same(got.masked, disp * got.mask)
    if disp.shape[0] == 2:                                   # a batch-stride error would need equal images
        assert not torch.equal(disp[0], disp[1]) and not torch.equal(got.wrap[0], got.wrap[1])


@pytest.mark.parametrize("name", CASES)
def test_right_frame_flag_is_the_mirrored_read(cv, name):
    disp, other, kw, _ = case(name)
    got = cv.lr_check(disp.cuda(), other.flip(-1).contiguous().cuda(), mirrored=False, **kw)
    for a, b in zip(got, device_result(name)):
        assert same(a.cpu(), b)


@pytest.mark.parametrize("name", ("c8x64f4", "c5x63"))
def test_base_offset_by_one_element(cv, name):
    """A base that is not 16-byte aligned: scalar loads, also where W % 4 == 0."""
    disp, other, kw, _ = case(name)
    shifted = []
    for t in (disp, other):
        buf = torch.empty(t.numel() + 1, device="cuda")
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        shifted.append(view)
    for a, b in zip(cv.lr_check(shifted[0], shifted[1], **kw), device_result(name)):
        assert same(a.cpu(), b)


@pytest.mark.parametrize("name", ("c8x64f4", "c4x257"))
def test_three_dimensional_maps(cv, name):
    disp, other, kw, _ = case(name)
    got = cv.lr_check(disp[:, 0].cuda(), other[:, 0].cuda(), **kw)
    for a, b in zip(got, device_result(name)):
        assert a.shape == disp[:, 0].shape and same(a.cpu(), b[:, 0])


@pytest.mark.parametrize("name", ("c8x64f4", "c5x63"))
def test_every_subset_of_want(cv, name):
    disp, other, kw, _ = case(name)
    d, o, full = disp.cuda(), other.cuda(), dict(zip(FIELDS, device_result(name)))
    for n in range(1, 5):
        for names in itertools.combinations(FIELDS, n):
            got = cv.lr_check(d, o, want=names, **kw)
            for f in FIELDS:
                if f in names:
                    assert same(getattr(got, f).cpu(), full[f]), (names, f)
                else:
                    assert getattr(got, f) is None, (names, f)
    for bad in ((), ("wrap", "delta")):
        with pytest.raises(ValueError):
            cv.lr_check(d, o, want=bad)


def test_known_scene(cv):
    dL, dR = (t.cuda() for t in LO.known_scene())
    left = cv.lr_check(dL, dR, mirrored=False)
    right = cv.lr_check(dR.flip(-1).contiguous(), dL)        # in the mirrored frame (loss.py:452)
    LO.check_known_scene(left.mask, right.mask.flip(-1))
    filled = cv.fill_background(dL, left.mask)
    assert float(filled[0, 0, 3, 33:39].max()) == 4.0        # the band is background, not the box
    assert torch.equal(filled[left.mask], dL[left.mask])


# ---------------------------------------------------------------------------------------------------
# fill
# ---------------------------------------------------------------------------------------------------
def run_fill(cv, disp, mask):
    """numpy (B,H,W) -> the device's fill as numpy, and the oracle's."""
    d, m = torch.from_numpy(disp).cuda(), torch.from_numpy(mask).cuda()
    before = d.clone()
    got = cv.fill_background(d, m)
    torch.cuda.synchronize()
    assert same(d.cpu(), before.cpu()) and got.dtype == torch.float32 and got.shape == d.shape
    return got.cpu().numpy(), LO.fill_background(disp, mask)


def identical(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_fill_hand_written_rows(cv):
    for name in sorted(ROWS):
        v, m, want = ROWS[name]
        got, ref = run_fill(cv, np.array([[v]], np.float32), np.array([[m]], bool))
        assert identical(got, ref) and np.array_equal(got, np.array([[want]], np.float32)), name
    e, z, N = [np.nan] * 3, [0] * 3, np.nan
    disp = np.array([[e, e, [4, N, 6], e, e, [N, 5, N], e]], np.float32)
    mask = np.array([[z, z, [1, 0, 1], z, z, [0, 1, 0], z]], bool)
    want = np.array([[[4, 4, 6], [4, 4, 6], [4, 4, 6], [4, 4, 5], [4, 4, 5], [5, 5, 5], [5, 5, 5]]], np.float32)
    got, ref = run_fill(cv, disp, mask)
    assert identical(got, ref) and np.array_equal(got, want)                      # empty rows: top, middle, bottom
    got, ref = run_fill(cv, np.full((1, 3, 5), N, np.float32), np.zeros((1, 3, 5), bool))
    assert identical(got, ref) and not got.any()                                  # an empty image


def poisoned(rng, B, H, W, p):
    """Random values and validity; NaN and Inf written into every invalid pixel."""
    disp = (rng.random((B, H, W), dtype=np.float32) * 60).astype(np.float32)
    mask = rng.random((B, H, W)) < p
    bad = np.where(rng.random((B, H, W)) < 0.5, np.float32(np.nan), np.float32(np.inf))
    return np.where(mask, disp, bad).astype(np.float32), mask


@pytest.mark.parametrize("W", (1, 2, 63, 64, 65, 256, 257, 1030))
def test_fill_widths(cv, W):
    rng = np.random.default_rng(600 + W)
    for H, p in ((1, 0.3), (2, 0.05), (5, 0.6)):
        disp, mask = poisoned(rng, 2, H, W, p)
        if H == 5:
            mask[0, 2] = False                                                    # an empty row between filled ones
            mask[1] = False                                                       # B = 2 with one image empty
        got, ref = run_fill(cv, disp, mask)
        assert np.isfinite(got).all(), (W, H)
        assert identical(got, ref), (W, H)
        assert identical(got[mask], disp[mask])
        if H == 5:
            assert not got[1].any()


def test_fill_runs_across_waves_and_chunks(cv):
    """Invalid runs placed on the boundaries the kernel carries values across: (valid columns, width)."""
    layouts = {
        "across a 64-lane boundary": ((60, 70), 128),
        "a whole wave": ((60, 130), 200),
        "across a 256-column chunk": ((250, 262), 300),
        "a whole chunk": ((10, 600), 1030),
        "from the first column over two chunks": ((515,), 1030),
        "to the last column over two chunks": ((3,), 700),
        "lane 63 and lane 0 of neighbouring waves": ((63, 64, 191, 320), 400),
    }
    for what, (cols, W) in layouts.items():
        disp = np.full((1, 2, W), np.nan, np.float32)
        mask = np.zeros((1, 2, W), bool)
        for i, c in enumerate(cols):
            mask[0, 0, c], disp[0, 0, c] = True, 9.0 - 2.5 * i                    # row 1 stays empty
        got, ref = run_fill(cv, disp, mask)
        assert np.isfinite(got).all() and identical(got, ref), what
        assert identical(got[0, 1], got[0, 0]), what
        rising = disp.copy()
        for i, c in enumerate(cols):
            rising[0, 0, c] = 1.0 + 2.5 * i                                       # the other side is the smaller one
        got, ref = run_fill(cv, rising, mask)
        assert identical(got, ref), what


def test_fill_four_dimensional_and_uint8(cv):
    rng = np.random.default_rng(7)
    disp, mask = poisoned(rng, 2, 3, 70, 0.4)
    ref = LO.fill_background(disp, mask)
    d = torch.from_numpy(disp).cuda().unsqueeze(1)
    for m in (torch.from_numpy(mask).cuda().unsqueeze(1), torch.from_numpy(mask.astype(np.uint8) * 255).cuda().unsqueeze(1)):
        got = cv.fill_background(d, m)
        assert got.shape == (2, 1, 3, 70) and identical(got[:, 0].cpu().numpy(), ref)
    with pytest.raises(ValueError):
        cv.fill_background(d, torch.from_numpy(mask).cuda())
    with pytest.raises(TypeError):
        cv.fill_background(d, d)


# ---------------------------------------------------------------------------------------------------
# graph capture, left_right_check
# ---------------------------------------------------------------------------------------------------
def test_replayed_graph_follows_its_inputs(cv):
    a = case("c4x257")[:2]
    b = (a[0].flip(0) + 0.25, a[1].flip(0))                  # other inputs of the same shape
    static = [t.cuda() for t in a]

    def step():
        r = cv.lr_check(static[0], static[1])
        return r, cv.fill_background(static[0], r.mask)      # a linear chain: one launch, then two

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, filled = step()
    seen = []
    for inputs in (b, a):
        for s, t in zip(static, inputs):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = cv.lr_check(inputs[0].cuda(), inputs[1].cuda())
        for x, y in zip(out, eager):
            assert same(x.cpu(), y.cpu())
        assert same(filled.cpu(), cv.fill_background(inputs[0].cuda(), eager.mask).cpu())
        seen.append(out.wrap.cpu().clone())
    assert not torch.equal(seen[0], seen[1])                 # the outputs followed the inputs


class Stub(torch.nn.Module):
    """A fixed, asymmetric function of the two images in the return convention ``kind`` names."""

    def __init__(self, kind):
        super(Stub, self).__init__()
        self.kind, self.calls = kind, 0

    @staticmethod
    def fn(imL, imR):
        return 3.0 + 2.0 * imL[:, 0:1] + imR[:, 1:2] - 0.5 * imL[:, 2:3] * imR[:, 0:1]

    def forward(self, imL, imR):
        self.calls += 1
        assert not self.training and not torch.is_grad_enabled()
        d = self.fn(imL, imR)
        if self.kind == "lr":                                # gcnet_LR: (oL, oR), each in its own frame
            return d, self.fn(imR.flip(-1), imL.flip(-1)).flip(-1)
        return [0], [d[:, 0] if self.kind == "bhw" else d]


@pytest.mark.parametrize("kind", ("bchw", "bhw", "lr"))
def test_left_right_check_with_a_stub(cv, kind):
    from dsmnet_amd.postprocess import left_right_check
    g = torch.Generator().manual_seed(77)
    imL, imR = torch.rand(2, 3, 6, 70, generator=g).cuda(), torch.rand(2, 3, 6, 70, generator=g).cuda()
    model = Stub(kind).train()
    res = left_right_check(model, imL, imR, threshold=0.75)
    assert model.calls == (1 if kind == "lr" else 2)
    # by hand: the left map from the pair, the right one from the mirrored, swapped pair, in the mirrored frame
    dL, dRm = Stub.fn(imL, imR), Stub.fn(imR.flip(-1), imL.flip(-1))
    if kind == "bhw":
        dL, dRm = dL[:, 0], dRm[:, 0]
    left = cv.lr_check(dL, dRm, threshold=0.75)
    right = cv.lr_check(dRm, dL, threshold=0.75)
    want = {"dispL": dL, "dispR": dRm.flip(-1), "maskL": left.mask, "maskR": right.mask.flip(-1),
            "weightL": left.weight, "weightR": right.weight.flip(-1),
            "filledL": cv.fill_background(dL, left.mask), "filledR": cv.fill_background(dRm, right.mask).flip(-1)}
    assert sorted(res) == sorted(want)
    for k in sorted(want):
        assert res[k].shape == dL.shape and same(res[k].cpu(), want[k].cpu()), k
    assert res["maskL"].dtype == torch.bool and 0 < int(res["maskL"].sum()) < res["maskL"].numel()
    assert sorted(left_right_check(model, imL, imR, fill=False)) == ["dispL", "dispR", "maskL", "maskR", "weightL", "weightR"]


def test_left_right_check_with_a_real_model(cv):
    from dsmnet_amd.models import model_create_by_name
    from dsmnet_amd.postprocess import left_right_check
    torch.manual_seed(0)
    model = model_create_by_name("dispnetcorr", 192).cuda()
    g = torch.Generator().manual_seed(78)
    imL, imR = torch.rand(1, 3, 64, 128, generator=g).cuda(), torch.rand(1, 3, 64, 128, generator=g).cuda()
    res = left_right_check(model, imL, imR)
    assert sorted(res) == ["dispL", "dispR", "filledL", "filledR", "maskL", "maskR", "weightL", "weightR"]
    for k, v in res.items():
        assert tuple(v.shape) == (1, 1, 64, 128), k
        assert v.dtype == (torch.bool if k.startswith("mask") else torch.float32), k
        assert k.startswith("mask") or bool(torch.isfinite(v).all()), k
