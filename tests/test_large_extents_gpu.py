"""GPU: every entry point a large batch reaches, with tensors that cross 2 GiB and 4 GiB, against float64.

The kernels address memory with 32-bit quantities (buffer descriptors, per-lane byte offsets, an out-of-range marker
at 2^31) and the host code switches kernels on byte extents (tests/test_extent_plans.py pins those guards without a
GPU).  An addressing bug in this range is silent -- a buffer load past a truncated extent returns zeros, a wrapped
offset reads memory that belongs to something else -- so every case here is built to make it visible:

* tensors are filled on the GPU from a seeded generator with unit-scale data of mean 0.5 (zeros stand out), and every
  batch item is a copy of item 0: ``y[b]`` must agree with ``y[0]`` over the WHOLE tensor (compared on the GPU, item by
  item), and float64 *windows* (tests/extents.py: first / last voxel, both sides of every 2^31 / 2^32 / 2^33 byte
  boundary of input, output and residual, seeded random places) catch what is wrong in all items alike;
* the name of the launched plan is the case's (tests/test_conv_plans_gpu.py ``launch``);
* the band is the project's own: ``check_band`` -- 2e-4 absolute for the fp32-input names, the mode's (max, rms) pair
  grown by sqrt(Cin / 64) for the split / z-sliding / transposed-split names, relative to the largest value and the
  rms of the reference windows; twice that for ``y[b]`` against ``y[0]``;
* ``y_amax`` (fp16 modes, Cout >= 32) equals ``y.abs().max()`` exactly, with the maximum planted through the residual
  on the last voxel's last channel (of every item, so that the items stay copies).

Each case holds only its own tensors and frees them; its id ends in its peak of device memory (the convolution
cases) or its docstring states it.  Streaming entry points (BatchNorm, relayout, absmax, the concatenation volume,
the weight gradient) follow the convolution cases with references of their own."""
import time

import pytest
import torch
import torch.nn.functional as F

from tests import extents as E
from tests.helpers import seeded
from tests.test_conv3d_gpu import TOL
from tests.test_conv_plans_gpu import F16_MODES, check_band, is_split, launch
from tests.test_f16_gpu import precision
from tests.test_zs_gpu import LIMITS

pytestmark = pytest.mark.gpu
CL3D = torch.channels_last_3d
PLANTED = 1000.0
ULP_PLANTED = 2.0 ** -14           # of an fp32 value in [512, 1024)


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


def fill(shape, seed, mean=0.5, copies=True):
    """A (B, C, D, H, W) tensor in NDHWC memory: N(mean, 1) from a seeded device generator; every item a copy of
    item 0 (``copies``)."""
    t = torch.empty(shape, device="cuda", dtype=torch.float32, memory_format=CL3D if len(shape) == 5 else torch.channels_last)
    v = t.permute(0, 2, 3, 4, 1) if len(shape) == 5 else t.permute(0, 2, 3, 1)
    g = torch.Generator(device="cuda").manual_seed(seed)
    if copies:
        v[0].normal_(mean, 1.0, generator=g)
        if shape[0] > 1:
            v[1:] = v[0]
    else:
        v.normal_(mean, 1.0, generator=g)
    return t


def weights(row, seed):
    """He-scaled weights (fan-out) and the scale / shift of a folded BatchNorm, as tests/test_conv_plans_gpu.py."""
    wshape = ((row.cin, row.cout) if row.tr else (row.cout, row.cin)) + (3, 3, 3)
    w = seeded(seed + 1, *wshape, scale=(2.0 / (27 * row.cout)) ** 0.5)
    return w, seeded(seed + 2, row.cout).abs() + 0.5, seeded(seed + 3, row.cout)


def crop(t, win):
    b, (z0, z1), (y0, y1), (x0, x1) = win
    return t[b:b + 1, :, z0:z1, y0:y1, x0:x1].cpu().double()


def band_abs(row, ref_max):
    """The case's band as an absolute error, for the whole-tensor comparison and the planted element."""
    if not is_split(row):
        return TOL
    return LIMITS[row.mode][0] * max(1.0, row.cin / 64.0) ** 0.5 * ref_max


def start_peak():
    """Device memory other tests of the session still hold: a case's peak is counted on top of it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return torch.cuda.memory_allocated()


def peak_gib(base):
    return (torch.cuda.max_memory_allocated() - base) / E.GIB


@pytest.mark.parametrize("i", range(len(E.BIG_CASES)), ids=lambda i: E.big_id(E.BIG_CASES[i]))
def test_a_launch_across_2_and_4_gib_against_float64_windows(cv, i):
    big = E.BIG_CASES[i]
    row = big.row
    seed = 9000 + 10 * i
    x = res = y = fL = fR = feats = d = None
    t0 = time.time()
    base = start_peak()
    try:
        w, sc, sh = weights(row, seed)
        if row.vol:
            fL = fill((row.B, row.cin // 2, row.size[1], row.size[2]), seed)
            fR = fill((row.B, row.cin // 2, row.size[1], row.size[2]), seed + 4)
            feats = (fL, fR)
            fetch = E.volume_fetch(fL[:1], fR[:1])             # every item is item 0
            fetch_x = lambda b, box: fetch(0, box)
        else:
            x = fill((row.B, row.cin) + tuple(row.size), seed)
            assert x.numel() * 4 == E.nbytes(row.B, row.cin, row.size)
            fetch_x = E.tensor_fetch(x)
        rd = E.res_dims(big)
        planted = rd is not None and row.cout >= 32
        if rd is not None:
            res = fill((row.B, row.cout) + rd, seed + 5)
            if planted:
                res.permute(0, 2, 3, 4, 1)[:, -1, -1, -1, -1] = PLANTED
        y = launch(cv, row, x, w, sc, sh, res, 1, feats, record=False)
        ydims = (row.B,) + E.y_dims(big)
        assert tuple(y.shape) == (row.B, row.cout) + ydims[1:]
        assert y.numel() * 4 == E.nbytes(row.B, row.cout, ydims[1:])

        # ---- float64 windows
        wins = E.case_windows(big)
        assert len(wins) >= 6 and E.window_values(row, wins) >= 20000
        got, want = [], []
        for label, win in wins:
            ref = E.windowed_reference(row, row.size, fetch_x, w, sc, sh,
                                       None if res is None else E.tensor_fetch(res), 1, win)
            g = crop(y, win)
            print("WIN %-7s %s max |err| %.3e of max |ref| %.3e" % (label, win, (g - ref).abs().max().item(),
                                                                   ref.abs().max().item()))
            got.append(g.reshape(-1))
            want.append(ref.reshape(-1))
        if planted:                                            # the last element of the "last" window ...
            pg, pw = got[1][-1].item(), want[1][-1].item()
            got[1][-1] = want[1][-1] = 0.0                     # ... stays out of the band's largest value and rms
        got, want = torch.cat(got), torch.cat(want)
        # ---- every item against item 0, the whole tensor (measured before anything is asserted: a failure shows both)
        lim = 2 * band_abs(row, want.abs().max().item())
        diffs = []
        for b in range(1, row.B):
            d = (y[b] - y[0]).abs().max().item()
            diffs.append(d)
        print("ITEMS max |y[b] - y[0]| %s (<= %.3e)" % (["%.3e" % v for v in diffs], lim))
        if planted:
            assert pw > 900.0 and abs(pg - pw) <= band_abs(row, want.abs().max().item()) + ULP_PLANTED, (pg, pw)
        check_band(row, got, want)
        for b, d in enumerate(diffs):
            assert d <= lim, "item %d differs from item 0 by %.3e (> %.3e)" % (b + 1, d, lim)

        # ---- y_amax
        if row.mode in F16_MODES and row.cout >= 32:
            amax = max(y[b].abs().max().item() for b in range(row.B))
            assert y._dsm_amax.item() == amax
            if planted:
                assert amax == y[-1, -1, -1, -1, -1].item() and amax > 900.0
        torch.cuda.synchronize()
        print("CASE %s: %.1f s, peak %.2f GiB" % (E.big_id(big), time.time() - t0, peak_gib(base)))
        assert peak_gib(base) <= big.gib <= 28.0, peak_gib(base)
    finally:
        del x, res, y, fL, fR, feats, d
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- BatchNorm
def channel_sums64(t, fn=None):
    """Per-channel float64 sums of a (B, C, D, H, W) NDHWC tensor (of ``fn(chunk)``), reduced plane by plane."""
    v = t.permute(0, 2, 3, 4, 1)
    acc = None
    for b in range(v.shape[0]):
        for z in range(v.shape[1]):
            c = v[b, z].double()
            outs = fn(c, b, z) if fn is not None else (c,)
            sums = [o.sum(dim=(0, 1)) for o in outs]
            acc = sums if acc is None else [a + s for a, s in zip(acc, sums)]
    return acc


def bn_windows(dims, seed):
    """Windows of a (B, D, H, W) volume: first, last, the 2^31 / 2^32 boundaries at 32 channels, two random."""
    big = E.Big(E.R("bn", "f16x2", 32, 32, dims[1:], B=dims[0]), None, 0.0)
    return [(l, w) for l, w in E.case_windows(big, seed) if not l.startswith("x@")]


def test_bn_add_relu3d_forward_at_4_gib(cv):
    """4.08 GiB flat (no crop: one linear index for y and out), ReLU.  Peak 8.5 GiB.

    Bounds as tests/test_bn3d_gpu.py: out 2e-5 max(1, |out|), statistics and affine values 1e-5; the float64
    statistics are reduced on the GPU plane by plane over ALL items, which differ here: a statistics pass whose index
    wrapped and read earlier items again would not reproduce them."""
    C, dims = 32, (4,) + E.ITEM32
    y = out = aff = None
    base = start_peak()
    try:
        y = fill((dims[0], C) + dims[1:], 41, mean=0.3, copies=False).requires_grad_(True)
        gamma, beta = (seeded(2, C).abs() + 0.5).cuda(), seeded(3, C).cuda()
        rm0, rv0 = seeded(5, C), seeded(6, C).abs() + 0.5
        rm, rv = rm0.cuda(), rv0.cuda()
        out = cv.bn_add_relu3d(y, gamma, beta, None, rm, rv, 2, 0.1, 1e-5)
        assert tuple(out.shape) == tuple(y.shape)
        nn = y.numel() // C
        s, ss = channel_sums64(y.detach(), lambda c, b, z: (c, c * c))
        mean, var = (s / nn).cpu(), (ss / nn - (s / nn) ** 2).cpu()
        invstd = 1.0 / (var + 1e-5).sqrt()
        scale = gamma.double().cpu() * invstd
        shift = beta.double().cpu() - mean * scale
        aff = out.grad_fn.saved_tensors[2].double().cpu().view(4, C)
        for name, got, ref in (("scale", aff[0], scale), ("shift", aff[1], shift), ("mean", aff[2], mean),
                               ("invstd", aff[3], invstd), ("running_mean", rm.double().cpu(), 0.9 * rm0.double() + 0.1 * mean),
                               ("running_var", rv.double().cpu(), 0.9 * rv0.double() + 0.1 * var * nn / (nn - 1))):
            err = (got - ref).abs().max().item()
            print("BN4 %s err %.3e" % (name, err))
            assert err <= 1e-5 * max(1.0, ref.abs().max().item()), (name, err)
        for label, win in bn_windows(dims, 1):
            ref = (crop(y.detach(), win) * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)).relu()
            err = (crop(out.detach(), win) - ref).abs().max().item()
            assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (label, err)
        print("BN4 peak %.2f GiB" % peak_gib(base))
        assert peak_gib(base) <= 8.6
    finally:
        del y, out, aff
        torch.cuda.empty_cache()


def test_bn_add_relu3d_forward_and_backward_at_3_gib_with_a_shorter_residual(cv):
    """y 3.06 GiB (three items that differ), the residual one voxel shorter in z, y and x: the coordinate-decomposing
    path of every kernel, and item 2 puts the corner of y, the residual, the output and the cotangent past 2^31 bytes
    (with two items byte 2^31 of y lies in the last plane of item 1, outside the corner, and the smaller tensors stay
    under 2^31 altogether).  ReLU after the addition; backward with a dense cotangent.  Peak under 19 GiB.

    Forward bounds as above.  Backward as tests/test_bn3d_gpu.py: 5e-5 max(1, |reference|) for dy and dres (windows)
    and for dgamma and dbeta (float64 sums over the whole corner, reduced on the GPU plane by plane).  The ReLU mask
    of the reference is the kernel's own ``out > 0`` (``out`` is checked against float64 first)."""
    C, dims = 32, (3,) + E.ITEM32
    rdims = tuple(v - 1 for v in E.ITEM32)
    y = res = out = gout = dy = dres = aff = None
    base = start_peak()
    try:
        y = fill((dims[0], C) + dims[1:], 51, mean=0.3, copies=False).requires_grad_(True)
        res = fill((dims[0], C) + rdims, 52, mean=-0.2, copies=False).requires_grad_(True)
        assert 4 * res.numel() > 2 ** 31 and E.nbytes(2, C, E.ITEM32) > 2 ** 31
        gamma = (seeded(2, C).abs() + 0.5).cuda().requires_grad_(True)
        beta = seeded(3, C).cuda().requires_grad_(True)
        rm0, rv0 = seeded(5, C), seeded(6, C).abs() + 0.5
        rm, rv = rm0.cuda(), rv0.cuda()
        out = cv.bn_add_relu3d(y, gamma, beta, res, rm, rv, 1, 0.1, 1e-5)
        assert tuple(out.shape) == (dims[0], C) + rdims
        nn = y.numel() // C
        s, ss = channel_sums64(y.detach(), lambda c, b, z: (c, c * c))
        mean, var = (s / nn).cpu(), (ss / nn - (s / nn) ** 2).cpu()
        invstd = 1.0 / (var + 1e-5).sqrt()
        scale = gamma.detach().double().cpu() * invstd
        shift = beta.detach().double().cpu() - mean * scale
        aff = out.grad_fn.saved_tensors[2].double().cpu().view(4, C)
        for name, got, ref in (("scale", aff[0], scale), ("shift", aff[1], shift), ("mean", aff[2], mean),
                               ("invstd", aff[3], invstd), ("running_mean", rm.double().cpu(), 0.9 * rm0.double() + 0.1 * mean),
                               ("running_var", rv.double().cpu(), 0.9 * rv0.double() + 0.1 * var * nn / (nn - 1))):
            err = (got - ref).abs().max().item()
            print("BN3 %s err %.3e" % (name, err))
            assert err <= 1e-5 * max(1.0, ref.abs().max().item()), (name, err)
        view = lambda t: t.view(1, -1, 1, 1, 1)
        odims = (dims[0],) + rdims
        wins = bn_windows(odims, 2)
        for label, win in wins:
            ref = (crop(y.detach(), win) * view(scale) + view(shift) + crop(res.detach(), win)).relu()
            err = (crop(out.detach(), win) - ref).abs().max().item()
            assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (label, err)
        # ---- backward
        gout = fill((dims[0], C) + rdims, 53, mean=0.1, copies=False)
        dy, dgamma, dbeta, dres = torch.autograd.grad(out, [y, gamma, beta, res], gout)
        assert tuple(dy.shape) == tuple(y.shape) and tuple(dres.shape) == tuple(res.shape)
        yv = y.detach().permute(0, 2, 3, 4, 1)
        mean_d, invstd_d = mean.cuda(), invstd.cuda()

        def terms(g, b, z):                                   # g: plane (H', W', C) of gout as float64
            gm = g * (out.detach().permute(0, 2, 3, 4, 1)[b, z] > 0)
            xhat = (yv[b, z, :rdims[1], :rdims[2]].double() - mean_d) * invstd_d
            return gm, gm * xhat
        sg, sgx = [t.cpu() for t in channel_sums64(gout, terms)]
        for name, got, ref in (("dbeta", dbeta, sg), ("dgamma", dgamma, sgx)):
            err = (got.double().cpu() - ref).abs().max().item()
            print("BN3 %s err %.3e of %.3e" % (name, err, ref.abs().max().item()))
            assert err <= 5e-5 * max(1.0, ref.abs().max().item()), (name, err)
        mg, mgx = sg / nn, sgx / nn
        ywins = bn_windows(dims, 3)                            # of y: planes, rows and columns outside the corner included
        for label, win in ywins:
            yc = crop(y.detach(), win)
            b, (z0, z1), (y0, y1), (x0, x1) = win
            gm = torch.zeros_like(yc)
            zc, hc, wc = (min(hi, n) - lo for (lo, hi), n in zip(win[1:], rdims))
            if zc > 0 and hc > 0 and wc > 0:
                cwin = (b, (z0, z0 + zc), (y0, y0 + hc), (x0, x0 + wc))
                gm[:, :, :zc, :hc, :wc] = crop(gout, cwin) * (crop(out.detach(), cwin) > 0)
                err = (crop(dres, cwin) - gm[:, :, :zc, :hc, :wc]).abs().max().item()
                assert err <= 5e-5 * max(1.0, gm.abs().max().item()), ("dres", label, err)
            xhat = (yc - view(mean)) * view(invstd)
            ref = view(scale) * (gm - view(mg) - xhat * view(mgx))
            err = (crop(dy, win) - ref).abs().max().item()
            assert err <= 5e-5 * max(1.0, ref.abs().max().item()), ("dy", label, err)
        print("BN3 peak %.2f GiB" % peak_gib(base))
        assert peak_gib(base) <= 19.0
    finally:
        del y, res, out, gout, dy, dres, aff
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- relayout, absmax
def test_the_relayout_at_4_gib_is_a_permutation_in_both_directions(cv):
    """``to_channels_last_3d`` / ``to_contiguous_3d`` on 4.08 GiB against torch's own permute-copy, ``torch.equal``
    over the whole tensor, item by item.  Peak 13.4 GiB."""
    x = ndhwc = back = ref = None
    base = start_peak()
    try:
        x = torch.empty((4, 32) + E.ITEM32, device="cuda")
        x.normal_(0.5, 1.0, generator=torch.Generator(device="cuda").manual_seed(61))
        ndhwc = cv.to_channels_last_3d(x)
        assert ndhwc.is_contiguous(memory_format=CL3D) and ndhwc.data_ptr() != x.data_ptr()
        for b in range(4):
            ref = x[b:b + 1].contiguous(memory_format=CL3D)
            assert torch.equal(ndhwc[b:b + 1], ref), b
        del ref
        ref = None
        back = cv.to_contiguous_3d(ndhwc)
        assert back.is_contiguous() and back.data_ptr() != ndhwc.data_ptr()
        for b in range(4):
            assert torch.equal(back[b], x[b]), b
        assert peak_gib(base) <= 13.4
    finally:
        del x, ndhwc, back, ref
        torch.cuda.empty_cache()


@pytest.mark.parametrize("n", [2 ** 29 + 3, 2 ** 30 + 5, 2 ** 31 + 7], ids=["2GiB+3", "4GiB+5", "8GiB+7"])
def test_absmax_finds_a_negative_extreme_at_the_last_element(cv, n):
    """``dsm_absmax`` over 2^29 + 3, 2^30 + 5 and 2^31 + 7 floats (a ragged tail past the 16-byte quads; the last
    index past 2^31), the extreme planted negative at the last element.  Peak 8 GiB + one chunk."""
    x = None
    try:
        x = torch.empty(n, device="cuda")
        x.normal_(0.5, 1.0, generator=torch.Generator(device="cuda").manual_seed(71))
        x[-1] = -77.0
        want = max(c.abs().max().item() for c in x.split(2 ** 28))
        assert want == 77.0
        assert cv.absmax(x).item() == want
        x[-1] = 0.25
        x[n // 2 + 1] = -66.0
        assert cv.absmax(x).item() == 66.0
    finally:
        del x
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- concatenation volume
def torch_volume_item(fL, fR, b, D, mask_left):
    """Item b of the concatenation volume, built with torch on the GPU: (2C, D, H, W)."""
    C, H, W = fL.shape[1:]
    ref = torch.zeros((2 * C, D, H, W), device=fL.device)
    for d in range(D):
        ref[:C, d, :, d if mask_left else 0:] = fL[b, :, :, d if mask_left else 0:]
        ref[C:, d, :, d:] = fR[b, :, :, :W - d]
    return ref


def test_concat_volume_forward_writes_4_gib(cv):
    """(4, 32, 24, 353, 1010) NDHWC, 4.08 GiB, the left half masked as PSMNet's; copies, so ``torch.equal`` with a
    torch-built volume, item by item on the GPU.  Peak 6.3 GiB."""
    fL = fR = vol = ref = None
    base = start_peak()
    try:
        B, C, (D, H, W) = 4, 16, E.ITEM32
        fL = fill((B, C, H, W), 81, copies=False).contiguous()
        fR = fill((B, C, H, W), 82, copies=False).contiguous()
        vol = cv.concat_volume(fL, fR, D, True)
        assert vol.numel() * 4 == E.nbytes(4, 32, E.ITEM32) > 2 ** 32
        for b in range(B):
            ref = torch_volume_item(fL, fR, b, D, True)
            assert torch.equal(vol[b], ref), b
        assert peak_gib(base) <= 6.4
    finally:
        del fL, fR, vol, ref
        torch.cuda.empty_cache()


def test_concat_volume_backward_reads_2_gib(cv):
    """gvol (2, 32, 24, 353, 1010), 2.04 GiB: dfL / dfR against float64 masked sums over the planes, reduced on the
    GPU.  Bound: a sum of D fp32 terms in any order is within D 2^-24 sum |terms| of the exact one.  Peak 4.4 GiB."""
    fL = fR = vol = g = dfL = dfR = wantL = wantR = absL = absR = None
    try:
        B, C, (D, H, W) = 2, 16, E.ITEM32
        fL = torch.zeros((B, C, H, W), device="cuda", requires_grad=True)
        fR = torch.zeros((B, C, H, W), device="cuda", requires_grad=True)
        vol = cv.concat_volume(fL, fR, D, False)
        g = fill((B, 2 * C, D, H, W), 91, copies=False)
        dfL, dfR = torch.autograd.grad(vol, [fL, fR], g)
        wantL = torch.zeros((B, C, H, W), device="cuda", dtype=torch.float64)
        wantR, absL, absR = torch.zeros_like(wantL), torch.zeros_like(wantL), torch.zeros_like(wantL)
        for d in range(D):
            gl, gr = g[:, :C, d].double(), g[:, C:, d, :, d:].double()
            wantL += gl
            absL += gl.abs()
            wantR[:, :, :, :W - d] += gr
            absR[:, :, :, :W - d] += gr.abs()
        u = D * 2.0 ** -24
        assert bool(((dfL.double() - wantL).abs() <= u * absL).all())
        assert bool(((dfR.double() - wantR).abs() <= u * absR).all())
        assert wantL.abs().max().item() > 1.0 and wantR.abs().max().item() > 1.0
    finally:
        del fL, fR, vol, g, dfL, dfR, wantL, wantR, absL, absR
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- weight gradient, dX
def test_conv3d_gradients_with_x_and_g_at_2_gib(cv):
    """32 -> 32 stride 1 through ``Conv3dFunction.backward``: x dense (2.04 GiB), g zero except inside three windows
    (first voxel, both sides of 2^31 bytes, last voxel).  dW is then a float64 sum over those windows only -- any
    offset that wraps for x, for g or for both changes it -- and dX is non-zero only within one voxel of them.
    Bound: 1e-4 of the largest reference entry (tests/test_bwd_ranges_gpu.py, f16x2).  Peak 10.3 GiB."""
    row = E.R("wgrad", "f16x2", 32, 32, E.ITEM32, B=2)
    big = E.Big(row, None, 0.0)
    x = g = dx = y = None
    base = start_peak()
    try:
        x = fill((row.B, 32) + E.ITEM32, 101)
        g = torch.zeros((row.B, 32) + E.ITEM32, device="cuda").contiguous(memory_format=CL3D)
        wins = [w for l, w in E.case_windows(big) if l in ("first", "last", "y@2^31")]
        assert len(wins) == 3
        gen = torch.Generator().manual_seed(102)
        gw = []
        for b, (z0, z1), (y0, y1), (x0, x1) in wins:
            gw.append(torch.randn((1, 32, z1 - z0, y1 - y0, x1 - x0), generator=gen, dtype=torch.float64).float())
            g[b:b + 1, :, z0:z1, y0:y1, x0:x1] = gw[-1].cuda()
        w = seeded(103, 32, 32, 3, 3, 3, scale=(2.0 / (27 * 32)) ** 0.5)
        wg = w.cuda().requires_grad_(True)
        xg = x.requires_grad_(True)
        with precision(cv, "f16x2"):
            y = cv.conv3d(xg, wg)
            dx, dw = torch.autograd.grad(y, [xg, wg], g)
        y = None
        torch.cuda.synchronize()
        # dW: float64 autograd on the windows' input crops
        wd = w.double().requires_grad_(True)
        total = 0.0
        for win, gwin in zip(wins, gw):
            xc, _ = E.padded_crop(row, E.ITEM32, E.tensor_fetch(x.detach()), win)
            total = total + (F.conv3d(xc, wd) * gwin.double()).sum()
        want_dw, = torch.autograd.grad(total, wd)
        err = (dw.double().cpu() - want_dw).abs().max().item() / want_dw.abs().max().item()
        print("WGRAD dW rel err %.3e" % err)
        assert err <= 1e-4, err
        # dX: windows one voxel larger than g's, then nothing else
        wt = w.flip(2, 3, 4).transpose(0, 1).contiguous()
        one, zero = torch.ones(32), torch.zeros(32)
        worst, ref_max = 0.0, 0.0
        grown = []
        for b, *box in wins:
            gbox = (b,) + tuple((max(lo - 1, 0), min(hi + 1, n)) for (lo, hi), n in zip(box, E.ITEM32))
            grown.append(gbox)
            ref = E.windowed_reference(row, E.ITEM32, E.tensor_fetch(g), wt, one, zero, None, 0, gbox)
            worst = max(worst, (crop(dx, gbox) - ref).abs().max().item())
            ref_max = max(ref_max, ref.abs().max().item())
        print("WGRAD dX rel err %.3e" % (worst / ref_max))
        assert worst <= 1e-4 * ref_max, worst / ref_max
        for b, (z0, z1), (y0, y1), (x0, x1) in grown:
            dx[b:b + 1, :, z0:z1, y0:y1, x0:x1] = 0.0
        assert dx.abs().sum().item() == 0.0
        assert peak_gib(base) <= 10.3
    finally:
        del x, g, dx, y
        torch.cuda.empty_cache()
