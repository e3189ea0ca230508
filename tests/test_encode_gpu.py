"""GPU: ``costvolume.encode_disparity`` (csrc/encode.hip) against tests/encode_oracle.py, byte for byte,
over the alignment and tail cases of its vector paths; ``submit.submit`` end to end; ``deploy``'s flags."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import encode_oracle as EO
from tests.test_encode import error_rows, hand_rows

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 5, 63), (1, 3, 65), (2, 4, 257), (1, 6, 1030)]
ALL = ("u16", "u8", "rgb", "err")
SUBSETS = [c for r in range(1, 5) for c in itertools.combinations(ALL, r)]


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


def frame(shape, seed=0):
    """disp, gt, mask of one shape: ties, saturation, holes, masked and non-finite pixels mixed in."""
    rng = np.random.RandomState(seed + shape[2])
    d = (rng.rand(*shape) * 200.0 - 4.0).astype(np.float32)
    d[rng.rand(*shape) < 0.1] = np.float32(rng.randint(0, 600)) / np.float32(512.0)      # u16 ties
    d[rng.rand(*shape) < 0.05] += np.float32(0.5)
    d[rng.rand(*shape) < 0.03] = np.nan
    d[rng.rand(*shape) < 0.02] = np.inf
    d[rng.rand(*shape) < 0.02] = -np.inf
    d[rng.rand(*shape) < 0.02] = 300.0
    g = (d + rng.randn(*shape).astype(np.float32) * np.float32(4.0)).astype(np.float32)
    g[~np.isfinite(g)] = 7.0
    g[rng.rand(*shape) < 0.2] = 0.0
    g[rng.rand(*shape) < 0.02] = -1.0
    m = (rng.rand(*shape) > 0.15).astype(np.uint8) * np.uint8(rng.randint(1, 255))       # non-zero = valid
    return d, g, m


def windows(shape):
    """The full frame, and odd-offset windows whose w % 4 takes 0, 1, 2, 3 (as far as the frame allows)."""
    B, H, W = shape
    out = [None]
    y0 = 1 if H > 2 else 0
    for r in range(4):
        w = ((W - 1) // 4) * 4 + r
        while w > W - 1:
            w -= 4
        if w >= 1:
            out.append((y0, 1, H - y0 - (1 if H > 3 else 0), w))
    return out


def same(got, want):
    for k in want:
        g = got[k].cpu()
        g = g.view(torch.int16).numpy().view(np.uint16) if g.dtype == torch.uint16 else g.numpy()
        assert g.shape == want[k].shape and g.dtype == want[k].dtype, (k, g.shape, g.dtype)
        assert np.array_equal(g, want[k]), "%s: %d bytes differ" % (k, int((g != want[k]).sum()))
    assert set(got) == set(want)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_output_window_flip_and_subset_matches_the_oracle(cv, shape):
    d, g, m = frame(shape)
    td, tg, tm = torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(m).cuda()
    for window in windows(shape):
        for flip in (False, True):
            want = EO.encode(d, g, m, window, flip, ALL, None)
            fixed = EO.encode(d, g, m, window, flip, ("rgb",), (3.0, 150.0))
            unmasked = EO.encode(d, g, None, window, flip, ALL, None)
            same(cv.encode_disparity(td, tg, tm, window, flip, ALL), want)
            same(cv.encode_disparity(td, None, tm, window, flip, ("rgb",), (3.0, 150.0)), fixed)
            same(cv.encode_disparity(td, tg, None, window, flip, ALL), unmasked)
            for sub in SUBSETS[:-1]:
                got = cv.encode_disparity(td, tg if "err" in sub else None, tm, window, flip, sub)
                same(got, {k: want[k] for k in sub})


def test_flip_is_encoding_the_flipped_tensors(cv):
    shape = (2, 5, 63)
    d, g, m = [torch.from_numpy(a).cuda() for a in frame(shape, 1)]
    window = (1, 3, 4, 58)
    a = cv.encode_disparity(d, g, m, window, True, ALL)
    mirrored = (1, 63 - 3 - 58, 4, 58)
    b = cv.encode_disparity(d.flip(-1).contiguous(), g.flip(-1).contiguous(), m.flip(-1).contiguous(), mirrored, False, ALL)
    for k in ALL:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


def test_four_dim_maps_bool_masks_and_an_offset_base(cv):
    shape = (2, 4, 257)
    d, g, m = frame(shape, 2)
    want = EO.encode(d, g, m, None, False, ALL, None)
    td, tg = torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda()
    tb = torch.from_numpy(m != 0).cuda()
    same(cv.encode_disparity(td.unsqueeze(1), tg.unsqueeze(1), tb.unsqueeze(1), want=ALL), want)
    # the same maps one element into their storage: 4-byte aligned only, the mask at an odd address
    off = lambda t: torch.cat([t.flatten()[:1], t.flatten()])[1:].view(t.shape)
    od, og, om = off(td), off(tg), off(tb)
    assert od.data_ptr() % 16 == 4 and om.data_ptr() % 4 == 1 and od.is_contiguous()
    same(cv.encode_disparity(od, og, om, want=ALL), want)
    same(cv.encode_disparity(od, og, om, (1, 1, 3, 255), True, ALL), EO.encode(d, g, m, (1, 1, 3, 255), True, ALL, None))


def test_auto_range_across_blocks(cv):
    """(2,70,1030), window rows 1..68 and columns 3..1026: 68 * 256 groups = 68 blocks of the range launch.
    The minimum sits in the first block's pixels, the maximum in the last block's; more extreme values
    just outside the window, and NaN, +-Inf and masked extremes inside it, must not move the range."""
    B, H, W = 2, 70, 1030
    window = (1, 3, 68, 1024)
    rng = np.random.RandomState(5)
    d = (rng.rand(B, H, W) * 50.0 + 20.0).astype(np.float32)
    m = np.ones((B, H, W), np.uint8)
    d[0, 1, 5] = 11.5                                        # first block of image 0
    d[0, 68, 1020] = 97.25                                   # last block of image 0
    d[0, 0, 5] = d[0, 1, 2] = d[0, 69, 9] = -400.0           # outside: above, left, below
    d[0, 1, 1027] = d[0, 69, 1029] = 900.0                   # outside: right, below
    d[0, 30, 30], d[0, 30, 31], d[0, 30, 32] = np.nan, np.inf, -np.inf
    d[0, 40, 40], d[0, 40, 41] = -77.0, 555.0                # masked extremes
    m[0, 40, 40] = m[0, 40, 41] = 0
    d[1, 35, 500] = 3.0                                      # image 1: its own range, extremes mid-image
    d[1, 36, 501] = 120.0
    assert EO.auto_range(EO._window(d, window, False), EO._window(m, window, False)) == [(11.5, 97.25), (3.0, 120.0)]
    td, tm = torch.from_numpy(d).cuda(), torch.from_numpy(m).cuda()
    for flip in (False, True):
        same(cv.encode_disparity(td, None, tm, window, flip, ("rgb",)), EO.encode(d, None, m, window, flip, ("rgb",)))
    # an all-NaN image is black, the other image keeps its colours
    d[0] = np.nan
    got = cv.encode_disparity(torch.from_numpy(d).cuda(), None, tm, window, False, ("rgb",))
    same(got, EO.encode(d, None, m, window, False, ("rgb",)))
    assert not got["rgb"][0].any() and got["rgb"][1].any()


def test_auto_range_past_the_block_cap(cv):
    """(1,260,1030): 260 * 258 groups want 263 blocks, the range launch has 256 per image and strides.  The
    extremes sit in the groups only a block's second step reaches."""
    rng = np.random.RandomState(6)
    d = (rng.rand(1, 260, 1030) * 50.0 + 20.0).astype(np.float32)
    d[0, 259, 1029] = 7.5                                    # the last group: block 6, second step
    d[0, 254, 16] = 140.0                                    # group 254 * 258 + 4 = 65536: block 0, second step
    assert EO.auto_range(d) == [(7.5, 140.0)]
    td = torch.from_numpy(d).cuda()
    same(cv.encode_disparity(td, want=("rgb",)), EO.encode(d, want=("rgb",)))
    same(cv.encode_disparity(td, want=("rgb",), flip=True), EO.encode(d, flip=True, want=("rgb",)))


def test_fixed_range_clamps_and_degenerate_range(cv):
    lut = EO.header_lut()
    d = torch.tensor([[[-5.0, 0.0, 0.99, 1.0, 2.0, 3.0, 50.0, float("nan"), 2.999]]]).cuda()
    got = cv.encode_disparity(d, want=("rgb",), vrange=(1.0, 3.0))["rgb"][0, 0].cpu().numpy()
    want = [lut[0]] * 4 + [lut[128], lut[255], lut[255], [0, 0, 0], lut[255]]
    assert np.array_equal(got, np.array(want, np.uint8))
    got = cv.encode_disparity(d, want=("rgb",), vrange=(2.0, 2.0))["rgb"][0, 0].cpu().numpy()
    assert (got[[0, 1, 2, 3, 4, 5, 6, 8]] == lut[0]).all() and not got[7].any()
    with pytest.raises(ValueError, match="vrange"):
        cv.encode_disparity(d, want=("rgb",), vrange=(3.0, 1.0))
    with pytest.raises(ValueError, match="window"):
        cv.encode_disparity(d, window=(0, 0, 1, 10))
    with pytest.raises(ValueError, match="want"):
        cv.encode_disparity(d, want=())
    with pytest.raises(ValueError, match="gt"):
        cv.encode_disparity(d, want=("err",))


def test_hand_written_rows(cv):
    d, want16, want8 = hand_rows()
    got = cv.encode_disparity(torch.from_numpy(d).cuda().view(1, 1, -1), want=("u16", "u8"))
    same(got, {"u16": want16[None, None], "u8": want8[None, None]})
    d, g, colours = error_rows()
    m = np.ones_like(d, dtype=np.uint8)
    m[3] = 0                                                  # a masked pixel is not scored
    colours[3] = 0
    got = cv.encode_disparity(torch.from_numpy(d).cuda().view(1, 1, -1), torch.from_numpy(g).cuda().view(1, 1, -1),
                              torch.from_numpy(m).cuda().view(1, 1, -1), want=("err",))
    same(got, {"err": colours[None, None]})


def test_replayed_graph_follows_its_inputs(cv):
    shape = (2, 4, 257)
    a = frame(shape, 3)
    b = (np.ascontiguousarray(a[0][::-1]) + np.float32(0.25), np.ascontiguousarray(a[1][::-1]), np.ascontiguousarray(a[2][::-1]))
    static = [torch.from_numpy(t).cuda() for t in a]
    window = (1, 1, 3, 254)

    def step():                                              # two launches: the range, then the rows
        return cv.encode_disparity(static[0], static[1], static[2], window, False, ALL)

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
    for inputs in (b, a):
        for s, t in zip(static, inputs):
            s.copy_(torch.from_numpy(t))
        graph.replay()
        torch.cuda.synchronize()
        same(out, EO.encode(inputs[0], inputs[1], inputs[2], window, False, ALL, None))
        seen.append(out["rgb"].cpu().clone())
    assert not torch.equal(seen[0], seen[1])                 # the outputs followed the inputs


# ----------------------------------------------------------------------------
# submit, end to end
# ----------------------------------------------------------------------------
class Stub(torch.nn.Module):
    """A fixed per-pixel function of the two images in the factory's return convention, so that padding
    the input changes nothing inside the un-padded frame."""

    def __init__(self):
        super(Stub, self).__init__()
        self.calls = 0

    @staticmethod
    def fn(imL, imR):
        return (imL[:, 0:1] * 3.0 + imR[:, 1:2] * 2.0 - imL[:, 2:3]).abs() * 2.5 + 0.125

    def forward(self, imL, imR, mode="test"):
        self.calls += 1
        return None, [self.fn(imL, imR)]


def _read(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


def test_submit_end_to_end_on_a_stub_model(cv, tmp_path, capsys):
    from dsmnet_amd import train, transforms
    from dsmnet_amd.datasets import Dataset_stereo
    from dsmnet_amd.submit import submit
    from tests.dataset_trees import write_kitti
    root = str(tmp_path / "kitti")
    samples = write_kitti(root, sizes=((19, 45),) * 4, seed=7)
    sub = os.path.join(root, "data_scene_flow", "training")
    names = ["%06d_10.png" % i for i in range(4)]
    ds = Dataset_stereo(*[[os.path.join(sub, folder, n) for n in names] for folder in ("image_2", "image_3", "disp_occ_0")])
    model = Stub().cuda()
    out = str(tmp_path / "submit" / "kitti_stub")
    data = submit(model, ds, out, batch_size=2, pad_multiple=16, formats=("u16", "viridis", "error"), vrange=None)
    assert model.calls == 2 and data["filename"] == names and len(data["time"]) == 4
    printed = capsys.readouterr().out.splitlines()
    assert len(printed) == 5 and printed[0].startswith("submit: 000000_10.png | time:")
    norm = transforms.Stereo_normalize()
    for i, (imL, imR, disp16) in enumerate(samples):
        chw = lambda a: torch.from_numpy(a.astype(np.float32).transpose(2, 0, 1)[None] / np.float32(255.0))
        gt = torch.from_numpy(disp16.astype(np.float32) / np.float32(256.0))[None, None]
        batch = torch.cat([chw(imL), chw(imR), gt], 1).cuda()
        seen = norm(batch[:, :6].clone())
        pred = Stub.fn(seen[:, :3], seen[:, 3:6]).cpu().numpy()
        want = EO.encode(pred, gt.numpy(), None, None, False, ("u16", "rgb", "err"), None)
        stem = names[i][:-4]
        assert np.array_equal(_read(os.path.join(out, "u16", stem + ".png")), want["u16"][0])
        assert np.array_equal(_read(os.path.join(out, "viridis", stem + ".png")), want["rgb"][0])
        assert np.array_equal(_read(os.path.join(out, "error", stem + ".png")), want["err"][0])
        m = train.evaluate_step(Stub().cuda(), batch, augment=norm, per_image=True)
        assert data["D1"][i] == m["d1"].item() and data["epe"][i] == m["epe"].item()
    # a second call prints from the .pkl without a forward
    again = submit(model, ds, out, batch_size=2, pad_multiple=16, formats=("u16", "viridis", "error"))
    assert model.calls == 2 and again == data
    assert capsys.readouterr().out.splitlines()[:4] == printed[:4]
    # lr_check: the rejected pixels are 0 in u16 (the stub's two views disagree almost everywhere)
    out2 = str(tmp_path / "submit" / "kitti_lr")
    submit(Stub().cuda(), ds, out2, batch_size=4, pad_multiple=16, formats=("u16",), lr_check=True)
    q = _read(os.path.join(out2, "u16", "000000_10.png"))
    assert q.shape == (19, 45) and (q == 0).any()


def test_submit_shape_plumbing_with_a_real_model(cv, tmp_path):
    from dsmnet_amd.datasets import Dataset_stereo
    from dsmnet_amd.models import model_create_by_name
    from dsmnet_amd.submit import submit
    from tests.dataset_trees import write_kitti
    root = str(tmp_path / "kitti")
    write_kitti(root, sizes=((64, 128),) * 2, seed=8)
    sub = os.path.join(root, "data_scene_flow", "training")
    names = ["%06d_10.png" % i for i in range(2)]
    ds = Dataset_stereo(*[[os.path.join(sub, folder, n) for n in names] for folder in ("image_2", "image_3", "disp_occ_0")])
    torch.manual_seed(0)
    model = model_create_by_name("dispnetcorr", 192).cuda()
    out = str(tmp_path / "real")
    data = submit(model, ds, out, batch_size=2, pad_multiple=64, formats=("u16", "u8", "viridis", "error"), vrange=(0.0, 64.0))
    assert len(data["D1"]) == 2 and np.isfinite(data["epe"]).all()
    assert _read(os.path.join(out, "u16", "000001_10.png")).shape == (64, 128)
    assert _read(os.path.join(out, "u8", "000001_10.png")).dtype == np.uint8
    assert _read(os.path.join(out, "error", "000000_10.png")).shape == (64, 128, 3)


# ----------------------------------------------------------------------------
# deploy's flags
# ----------------------------------------------------------------------------
def test_deploy_flags(cv, tmp_path):
    import matplotlib.pyplot as plt
    from oracle import models as OM
    from dsmnet_amd import deploy, img_rw
    from dsmnet_amd.models import model_create_by_name
    sd = OM.init_state("dispnetcorr", 0)
    w = str(tmp_path / "w.pkl")
    torch.save({"state_dict": sd}, w)
    rng = np.random.default_rng(2)
    imgL = rng.integers(0, 256, (256, 512, 3), dtype=np.uint8)
    imgR = np.roll(imgL, -5, axis=1)
    pl, pr = str(tmp_path / "L.png"), str(tmp_path / "R.png")
    img_rw.imwrite(pl, imgL)
    img_rw.imwrite(pr, imgR)
    model = deploy.load_weights(model_create_by_name("dispnetcorr", 192), w)
    disp = deploy.disp_predict(model.eval().cuda(), imgL, imgR)
    base = ["--net", "dispnetcorr", "--path_weight", w, "--path_left", pl, "--path_right", pr]
    # no new flag: the bytes plt.imsave writes
    plain, ref = str(tmp_path / "plain.png"), str(tmp_path / "ref.png")
    deploy.main(base + ["--out", plain])
    plt.imsave(ref, disp)
    assert open(plain, "rb").read() == open(ref, "rb").read()
    # kitti16 reads back as rint(d * 256)
    k16 = str(tmp_path / "k16.png")
    deploy.main(base + ["--out", k16, "--encode", "kitti16"])
    assert np.array_equal(_read(k16), EO.u16(disp[None])[0])
    # viridis over a fixed range, and the error picture against a ground-truth file
    gt = (disp + rng.standard_normal(disp.shape).astype(np.float32)).astype(np.float32)
    pg, vir = str(tmp_path / "gt.pfm"), str(tmp_path / "vir.png")
    img_rw.save_pfm(pg, gt)
    deploy.main(base + ["--out", vir, "--encode", "viridis", "--vrange", "0", "40", "--error_map", "--path_disp_gt", pg])
    assert np.array_equal(_read(vir), EO.rgb(disp[None], None, (0.0, 40.0))[0])
    assert np.array_equal(_read(str(tmp_path / "vir_err.png")), EO.err(disp[None], gt[None])[0])
    with pytest.raises(SystemExit):
        deploy.main(base + ["--vrange", "0", "1"])
