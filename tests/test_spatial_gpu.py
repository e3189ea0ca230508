"""GPU: the fused spatial augmentation (csrc/spatial.hip, dsmnet_amd.transforms) against the numpy
restatement with explicit records, the whole Stereo_Spatial / Stereo_train pipelines against the
fixture written from the reference (same seeds), launch count, host synchronisation, argument
errors, and one supervised training step fed by Stereo_train.

Crop-only outputs must be bit-equal.  Resize bound: |got - want| <= 4 * 2^-23 * M, M = the largest
magnitude among the pixel's four taps in output units (after the shift add, times scale_rand, or
/ 255).  Against the fp32 restatement the kernel's only freedom would be FMA contraction in the
two lerps (one rounding of a term <= M each) plus the final multiply or divide; the factor 4
leaves about 2x.  The kernel is compiled without contraction (measured: bit-equal,
profiles/spatial.md)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import spatial_oracle as SO
from tests.conftest import Golden

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23


def _frames(B, H, W, C, seed):
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 256, size=(B, H, W, C)).astype(np.float32)
    for c in range(6, C):
        d = (rng.rand(B, H, W) * 220 - 20).astype(np.float32)          # negatives .. 200
        d[rng.rand(B, H, W) < 0.25] = 0.0                               # exact zeros
        x[..., c] = d
    return x


def _resize_record(shift, ws, hs, w, h, out_hw, scale_rand):
    return (shift, ws, hs, w, h, 1, scale_rand, 1.0 / (float(out_hw[1]) / w), 1.0 / (float(out_hw[0]) / h))


def _run(x, records, hw, channels=6):
    from dsmnet_amd import costvolume as cv
    xd = torch.from_numpy(x).cuda()
    out = cv.stereo_spatial(xd, records, hw, channels)
    assert tuple(out.shape) == (x.shape[0], x.shape[3]) + tuple(hw) and out.is_contiguous()
    assert torch.equal(xd.cpu(), torch.from_numpy(x))                   # the input is not modified
    return out.cpu().numpy()


def _within(got, x, records, hw, channels=6):
    want = SO.restate_batch(x, records, hw, channels)
    err = np.abs(got.astype(np.float64) - want)
    bound = 4 * EPS * SO.tap_bound_batch(x, records, hw, channels)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.max() > 0 else 0.0
    print("  max err %.3e, worst err / bound %.3f, bit-equal %s" % (err.max(), worst, np.array_equal(got, want)))
    assert (err <= bound).all(), (err.max(), worst)
    return err.max()


@pytest.mark.parametrize("C", [6, 7, 8])
@pytest.mark.parametrize("H0,W0", [(9, 13), (5, 7), (12, 40)])
def test_crop_only_is_a_bit_exact_gather(hip_lib, C, H0, W0):
    x = _frames(2, H0, W0, C, 10 * C + H0)
    n = 0
    for h, w in ((1, 1), (H0, W0), (H0 - 1, W0 - 2), (2, W0 - 1), (H0, 3)):
        for shift in sorted({0, 1, W0 - w}):
            if shift > W0 - w:
                continue
            # image 0 touches the right and bottom edges of the shifted frame, image 1 the origin
            records = [(shift, W0 - shift - w, H0 - h, w, h, 0, 1.0, 1.0, 1.0),
                       (shift, 0, 0, w, h, 0, 1.0, 1.0, 1.0)]
            channels = 6 if n % 2 == 0 else 0
            got = _run(x, records, (h, w), channels)
            assert np.array_equal(got, SO.restate_batch(x, records, (h, w), channels)), (h, w, shift)
            n += 1
    assert n >= 11


@pytest.mark.parametrize("C", [6, 7, 8])
def test_resize_explicit_records(hip_lib, C):
    x = _frames(2, 12, 40, C, 30 + C)
    for (h, w), hw, shifts, s in (((7, 11), (10, 16), (0, 3), 1.37),        # upscale, 16/11 and 10/7
                                  ((11, 37), (6, 16), (3, 0), 0.43),       # downscale, 16/37 and 6/11
                                  ((2, 2), (5, 7), (1, 38), 2.9),          # clamping at all four borders
                                  ((5, 1), (7, 4), (39, 0), 1.0 / 1.3),    # 1-pixel-wide window
                                  ((1, 9), (3, 5), (2, 2), 1.11),          # 1-pixel-high window
                                  ((12, 40), (12, 40), (0, 0), 0.97)):     # same size: every weight is 0
        records = [_resize_record(shifts[0], 40 - shifts[0] - w, 12 - h, w, h, hw, s),
                   _resize_record(shifts[1], 0, 0, w, h, hw, s)]
        for channels in (6, 0):
            _within(_run(x, records, hw, channels), x, records, hw, channels)


def test_batch_above_the_record_cap_and_unaligned_bases(hip_lib):
    """50 images: launches of 48 and 2.  Both bases are 4 bytes past a 16-byte boundary; the
    elements before and after the output stay untouched.  Crop and resize records alternate."""
    from dsmnet_amd import _lib
    from dsmnet_amd import costvolume as cv
    B, H0, W0, C, hw = 50, 5, 7, 7, (3, 4)
    assert B > _lib.DSM_SPATIAL_MAX_RECORDS
    x = _frames(B, H0, W0, C, 50)
    records = [(b % 3, b % 2, b % 3, 4, 3, 0, 1.0, 1.0, 1.0) if b % 2 == 0 else
               _resize_record(b % 4, b % 3, b % 2, 2, 2, hw, 1.0 + b / 100.0) for b in range(B)]
    want = SO.restate_batch(x, records, hw)
    xbuf = torch.zeros(x.size + 1, device="cuda")
    xd = xbuf[1:].view(x.shape)
    xd.copy_(torch.from_numpy(x))
    assert xd.data_ptr() % 16 == 4
    got = cv.stereo_spatial(xd, records, hw).cpu().numpy()                  # unaligned input
    assert np.array_equal(got[::2], want[::2])
    ybuf = torch.full((want.size + 2,), -7.0, device="cuda")               # unaligned output, C ABI
    recs = (_lib.SpatialRecord * B)()
    for r, t in zip(recs, records):
        r.shift, r.ws, r.hs, r.w, r.h, r.resize, r.scale_rand, r.scale_x, r.scale_y = t
    rc = hip_lib.dsm_stereo_spatial(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(ybuf[1:].data_ptr()), recs, B,
                                    B, C, H0, W0, hw[0], hw[1], 6,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert ybuf[0].item() == -7.0 and ybuf[-1].item() == -7.0 and xbuf[0].item() == 0.0
    assert np.array_equal(ybuf[1:-1].cpu().numpy().reshape(want.shape), got)
    _within(got, x, records, hw)


@pytest.mark.parametrize("case", ["crop_a", "crop_b", "crop_c", "scale_a", "scale_b", "scale_c", "scale_big_c"])
def test_stereo_spatial_against_the_fixture(hip_lib, case):
    from dsmnet_amd import transforms as T
    gold = Golden("spatial")
    meta = gold.meta["cases"][case]
    x, want = gold["frames." + meta["frames"]], gold[case + ".out"]
    t = T.Stereo_Spatial(list(meta["size_crop"]), meta["scale_delt"], meta["shift_max"])
    xd = torch.from_numpy(x).cuda()
    np.random.seed(meta["seed"])
    out = t(xd)
    assert float(np.random.rand()) == float(gold[case + ".next_rand"])
    assert torch.equal(xd.cpu(), torch.from_numpy(x))
    got = out.cpu().numpy()
    assert got.shape == want.shape
    if meta["scale_delt"] == 0:
        assert np.array_equal(got, want)
    else:
        records = [tuple(int(v) for v in r[:6]) + tuple(r[6:]) for r in gold[case + ".records"].tolist()]
        err = np.abs(got.astype(np.float64) - want)
        print("  %s max err %.3e, bit-equal %s" % (case, err.max(), np.array_equal(got, want)))
        assert (err <= 4 * EPS * SO.tap_bound_batch(x, records, want.shape[2:])).all(), err.max()
    np.random.seed(meta["seed"])                                            # one frame: (C, h, w), same draws
    one = T.Stereo_Spatial(list(meta["size_crop"]), meta["scale_delt"], meta["shift_max"])(xd[0])
    assert torch.equal(one, out[0])


@pytest.mark.parametrize("case", ["crop_a", "scale_a"])
def test_stereo_train_against_the_fixture(hip_lib, case):
    """Spatial launch + colour launch.  Lighting draws on the batch's device, so the colour half
    is compared with the reference's steps restated with torch ops on the device under the same
    seed, applied to the fixture's Stereo_Spatial output (the colour kernel's 1e-5 bound)."""
    from dsmnet_amd import transforms as T
    gold = Golden("spatial")
    meta = gold.meta["cases"][case]
    x, spatial = gold["frames." + meta["frames"]], gold[case + ".out"]
    t = T.Stereo_train(list(meta["size_crop"]), meta["scale_delt"], meta["shift_max"])
    np.random.seed(meta["seed"])
    torch.manual_seed(21)
    out = t(torch.from_numpy(x).cuda())
    after = (float(np.random.rand()), torch.rand(1).item(), torch.rand(1, device="cuda").item())
    torch.manual_seed(21)
    want = SO.lighting_normalize_torch(torch.from_numpy(spatial).cuda())
    assert after == (float(gold[case + ".next_rand"]), torch.rand(1).item(), torch.rand(1, device="cuda").item())
    assert torch.isfinite(out).all()
    err = (out[:, :6] - want[:, :6]).abs().max().item()
    assert err <= 1e-5, err
    records = [tuple(int(v) for v in r[:6]) + tuple(r[6:]) for r in gold[case + ".records"].tolist()]
    bound = 4 * EPS * SO.tap_bound_batch(x, records, spatial.shape[2:])[:, 6:]
    assert (np.abs(out[:, 6:].cpu().numpy().astype(np.float64) - spatial[:, 6:]) <= bound).all()


def test_to_tensor_and_eval(hip_lib):
    from dsmnet_amd import transforms as T
    x = _frames(2, 9, 13, 7, 60)
    xd = torch.from_numpy(x).cuda()
    ident = [(0, 0, 0, 13, 9, 0, 1.0, 1.0, 1.0)] * 2
    want = SO.restate_batch(x, ident, (9, 13))
    assert np.array_equal(want[:, 6], x[..., 6]) and np.array_equal(want[:, 0], x[..., 0] / np.float32(255))
    assert np.array_equal(T.Stereo_ToTensor()(xd).cpu().numpy(), want)
    assert np.array_equal(T.ToTensor_numpy()(xd[1]).cpu().numpy(), want[1])
    ev = T.Stereo_eval()(xd)
    ref = torch.from_numpy(want).cuda()
    T.Stereo_normalize()(ref)
    assert torch.equal(ev, ref)
    np.random.seed(1)
    raw = T.Spatial_stereo([8, 6], 0, 3)(xd)                                # no ToTensor: no / 255
    np.random.seed(1)
    recs, hw, channels = T.Compose([T.Spatial_stereo([8, 6], 0, 3)]).plan_spatial(2, 9, 13)
    assert channels == 0 and np.array_equal(raw.cpu().numpy(), SO.restate_batch(x, recs, hw, 0))


def test_no_host_synchronisation_and_one_launch_per_batch(hip_lib):
    from torch.profiler import ProfilerActivity, profile
    from dsmnet_amd import transforms as T
    xd = torch.from_numpy(_frames(4, 40, 72, 7, 70)).cuda()
    sp, tr = T.Stereo_Spatial([48, 32], 0.4, 8), T.Stereo_train([48, 32], 0, 8)
    sp(xd), tr(xd)                                   # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a, b = sp(xd), tr(xd)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    for t, total in ((sp, 1), (tr, 6)):              # Stereo_train: 4 normal_ draws, spatial, colour
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            t(xd)
            torch.cuda.synchronize()
        kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        assert len([n for n in kernels if "stereo_spatial_kernel" in n]) == 1, kernels
        assert len(kernels) == total, kernels


def test_argument_errors(hip_lib):
    from dsmnet_amd import _lib
    from dsmnet_amd import costvolume as cv
    from dsmnet_amd import transforms as T
    recs = [(1, 2, 1, 8, 6, 0, 1.0, 1.0, 1.0)] * 2
    x = torch.rand(2, 9, 13, 7, device="cuda")
    assert cv.stereo_spatial(x, recs, (6, 8)).shape == (2, 7, 6, 8)
    with pytest.raises(ValueError):
        cv.stereo_spatial(x.double(), recs, (6, 8))
    with pytest.raises(ValueError):
        cv.stereo_spatial(torch.rand(2, 7, 9, 13, device="cuda"), recs, (6, 8))            # CHW batch
    with pytest.raises(ValueError):
        cv.stereo_spatial(torch.rand(2, 9, 13, 8, device="cuda")[..., :7], recs, (6, 8))   # strided view
    with pytest.raises(ValueError):
        cv.stereo_spatial(torch.rand(2, 9, 26, 7, device="cuda")[:, :, ::2], recs, (6, 8))
    for C in (5, 9):
        with pytest.raises(ValueError):
            cv.stereo_spatial(torch.rand(2, 9, 13, C, device="cuda"), recs, (6, 8))
    with pytest.raises(ValueError):
        cv.stereo_spatial(x, recs[:1], (6, 8))
    with pytest.raises(ValueError):
        cv.stereo_spatial(x, recs, (6, 8), to_tensor_channels=3)
    with pytest.raises(_lib.DsmnetHipError):
        cv.stereo_spatial(x, [(1, 5, 1, 8, 6, 0, 1.0, 1.0, 1.0)] * 2, (6, 8))               # window past the edge
    with pytest.raises(ValueError):
        T.Stereo_Spatial([8, 6], 0, 3)(torch.rand(2, 7, 9, 13, device="cuda"))
    with pytest.raises(ValueError):
        T.Stereo_Spatial([8, 6], 0, 3)(x.double())
    with pytest.raises(ValueError, match="width"):
        T.Stereo_train([12, 6], 0, 3)(x)                                                    # 13 - 2 < 12


def test_one_training_step_on_stereo_train(hip_lib):
    from dsmnet_amd import train
    from dsmnet_amd import transforms as T
    from dsmnet_amd.models import model_create_by_name
    g = torch.Generator().manual_seed(3)
    left = torch.rand(2, 200, 400, 3, generator=g) * 255
    disp = torch.full((2, 200, 400, 1), 6.0)
    disp[:, :, :6] = 0
    frames = torch.cat([left, torch.roll(left, -6, dims=2), disp], 3).contiguous().cuda()
    assert frames.shape == (2, 200, 400, 7)
    np.random.seed(4)
    torch.manual_seed(0)
    t = T.Stereo_train(size_crop=[384, 192], scale_delt=0, shift_max=8)
    batch = t(frames)
    assert batch.shape == (2, 7, 192, 384)
    model = model_create_by_name("dispnetcorr", 192).cuda()
    lf = train.losses("supervised", model.count_levels, 37)
    lf.Weight_Adjust_levels(10)
    opt = train.make_optimizer(model, lr=1e-4)
    before = [p.detach().clone() for p in model.parameters()]
    loss, d1, epe = train.train_step(model, opt, lf, batch)
    assert np.isfinite(loss) and loss > 0 and np.isfinite(d1) and np.isfinite(epe)
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    assert all(torch.isfinite(p).all() for p in model.parameters())
