"""CPU: the rules of ``dsm_disp_encode`` as tests/encode_oracle.py restates them -- against
``plt.imsave``, matplotlib's table and hand-written rows -- every refusal of the entry point through
ctypes (nothing is launched), ``submit.ResultWriter`` on host arrays and ``submit``'s resume path."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

from dsmnet_amd import _lib
from tests import encode_oracle as EO

F = np.float32


# ----------------------------------------------------------------------------
# the oracle itself
# ----------------------------------------------------------------------------
def _imsave_rgb(a):
    plt = pytest.importorskip("matplotlib.pyplot")
    from PIL import Image
    buf = io.BytesIO()
    plt.imsave(buf, a, format="png")
    buf.seek(0)
    return np.array(Image.open(buf).convert("RGB"))


@pytest.mark.parametrize("shape", [(37, 53), (64, 128), (5, 7)])
def test_auto_range_rgb_is_plt_imsave(shape):
    """Byte for byte on these maps.  Not a general identity: matplotlib divides in float64 by the unrounded
    range, the rule in fp32, and on a random 384 x 1280 map 5 of 1,474,560 bytes differ."""
    rng = np.random.RandomState(shape[0])
    a = (rng.rand(*shape) * 191.0 - 3.0).astype(np.float32)
    assert np.array_equal(EO.rgb(a[None])[0], _imsave_rgb(a))


def test_constant_map_is_entry_zero_as_plt_imsave():
    a = np.full((6, 9), 17.25, np.float32)
    got = EO.rgb(a[None])[0]
    assert np.array_equal(got, _imsave_rgb(a))
    assert (got == EO.header_lut()[0]).all()


def test_committed_table_is_matplotlibs():
    lut = EO.header_lut()
    assert lut.shape == (256, 3)
    assert tuple(lut[0]) == (68, 1, 84) and tuple(lut[128]) == (32, 144, 140) and tuple(lut[255]) == (253, 231, 36)
    mpl = pytest.importorskip("matplotlib")
    want = (np.asarray(mpl.colormaps["viridis"].colors) * 255).astype(np.uint8)
    assert np.array_equal(lut, want)


def hand_rows():
    """(disp, expected u16, expected u8) of hand-written values."""
    d = [F(1) / F(512), F(3) / F(512), F(5) / F(512), F(7) / F(512),         # q = 0.5, 1.5, 2.5, 3.5: ties to even
         F(300.0), F(-1.0), F(0.0), F(np.nan), F(np.inf), F(-np.inf),
         F(0.5), F(1.5), F(2.5), F(254.5), F(255.5), F(1000.0), F(-0.5), F(10.25)]
    u16 = [1, 2, 2, 4, 65535, 1, 1, 0, 0, 0, 128, 384, 640, 65152, 65408, 65535, 1, 2624]
    u8 = [0, 0, 0, 0, 255, 0, 0, 0, 255, 0, 0, 2, 2, 254, 255, 255, 0, 10]
    return np.array(d, np.float32), np.array(u16, np.uint16), np.array(u8, np.uint8)


def error_rows():
    """(disp, gt, expected colours), written by hand.

    Arm 1 of the fminf (e / 3 is the smaller: gt < 60): gt = 32, d = 32 - 3 * edge, so e = 3/16 ... 48 and
    n = e / 3 are exact and n sits exactly on each of the nine edges: the upper bin.  One ulp less of e
    (d = 0 and gt = e, so that the subtraction cannot round it away): the lower bin.
    Arm 2 ((e / gt) / 0.05f is the smaller: gt > 60): gt = 128, e = 1/4 ... 64 in powers of two, so
    n = e / 6.4 = 0.039 ... 10 walks through bins 0 ... 8; and the one edge this arm reaches exactly:
    gt = 64, e = 16 * 0.05f * 64 (d = 64 - e is exact: 2^24 - 13421773 units of 2^-18), n = 16."""
    C = EO.ERR_COLOURS
    d, g, c = [], [], []
    for k in range(9):
        e = F(3.0) * F(2.0 ** (k - 4))
        d += [F(32.0) - e, F(0.0)]
        g += [F(32.0), np.nextafter(e, F(0))]
        c += [C[k + 1], C[k]]
    for k in range(9):
        d.append(F(128.0) - F(2.0 ** (k - 2)))
        g.append(F(128.0))
        c.append(C[k])
    e16 = F(0.05) * F(16.0 * 64.0)
    d += [F(64.0) - e16, F(64.0) - np.nextafter(e16, F(0))]
    g += [F(64.0)] * 2
    c += [C[9], C[8]]
    # holes, a non-finite ground truth, non-finite predictions on scored pixels
    d += [F(5.0), F(5.0), F(5.0), F(np.nan), F(np.inf), F(-np.inf), F(7.0)]
    g += [F(0.0), F(-2.0), F(np.nan), F(9.0), F(9.0), F(9.0), F(np.inf)]
    c += [[0, 0, 0]] * 3 + [C[9]] * 3 + [[0, 0, 0]]
    return np.array(d, np.float32), np.array(g, np.float32), np.array(c, np.uint8)


def test_hand_written_u16_and_u8_rows():
    d, want16, want8 = hand_rows()
    assert np.array_equal(EO.u16(d[None, None])[0, 0], want16)
    assert np.array_equal(EO.u8(d[None, None])[0, 0], want8)
    mask = np.zeros_like(d, dtype=np.uint8)
    assert not EO.u16(d[None, None], mask[None, None]).any() and not EO.u8(d[None, None], mask[None, None]).any()


def test_error_bins_on_every_edge():
    d, g, want = error_rows()
    got = EO.err(d[None, None], g[None, None])[0, 0]
    assert np.array_equal(got, want)
    # the first arm's rows by hand: e = 3/16 exactly is n = 1/16, the second bin
    assert np.abs(g[0] - d[0]) == F(3.0) / F(16.0) and tuple(got[0]) == (69, 117, 180) and tuple(got[1]) == (49, 54, 149)
    # both arms are taken
    e = np.abs(g - d)
    with np.errstate(all="ignore"):
        first = e / F(3.0) < (e / g) / F(0.05)
    assert first[:18].all() and not first[18:29].any()
    assert np.abs(g[27] - d[27]) == F(0.05) * F(1024.0)      # the second arm's exact edge: e survives gt - d
    # n = 1 is D1's step: the outlier colour starts there
    assert np.abs(g[8] - d[8]) == F(3.0) and tuple(got[8]) == (254, 224, 144) and tuple(got[9]) == (224, 243, 248)


def test_fixed_range_clamps():
    d = np.array([[[-5.0, 0.0, 0.99, 1.0, 2.0, 3.0, 50.0, np.nan]]], np.float32)
    lut = EO.header_lut()
    got = EO.rgb(d, vrange=(1.0, 3.0))[0, 0]
    assert [tuple(p) for p in got] == [tuple(lut[0])] * 4 + [tuple(lut[128]), tuple(lut[255]), tuple(lut[255]), (0, 0, 0)]
    assert (EO.rgb(d[:, :, :7], vrange=(2.0, 2.0)) == lut[0]).all()


# ----------------------------------------------------------------------------
# refusals: each returns its code, nothing is launched (the pointers are not memory)
# ----------------------------------------------------------------------------
def _args(**kw):
    a = _lib.EncodeArgs()
    a.disp, a.u16 = 0x10000, 0x20000
    a.B, a.Hs, a.Ws, a.y0, a.x0, a.h, a.w = 1, 8, 12, 1, 2, 6, 9
    a.vmin, a.vmax = 0.0, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


REFUSALS = [
    ("null disp", dict(disp=None), -1),
    ("all outputs null", dict(u16=None), -1),
    ("err without gt", dict(err=0x30000), -1),
    ("auto-range rgb without a workspace", dict(rgb=0x30000, flags=_lib.DSM_ENCODE_AUTO_RANGE), -1),
    ("B = 0", dict(B=0), -1),
    ("Hs = 0", dict(Hs=0), -1),
    ("Ws < 0", dict(Ws=-3), -1),
    ("h = 0", dict(h=0), -1),
    ("w = 0", dict(w=0), -1),
    ("window above the frame", dict(y0=-1), -1),
    ("window left of the frame", dict(x0=-1), -1),
    ("window past the bottom", dict(y0=3), -1),
    ("window past the right", dict(x0=4), -1),
    ("vmin NaN", dict(rgb=0x30000, vmin=float("nan")), -1),
    ("vmax Inf", dict(rgb=0x30000, vmax=float("inf")), -1),
    ("vmax < vmin", dict(rgb=0x30000, vmin=2.0, vmax=1.0), -1),
    ("unknown flag", dict(flags=4), -1),
    ("u16 overlaps disp", dict(u16=0x10000 + 8 * 12 * 4 - 2), -1),
    ("rgb overlaps gt", dict(rgb=0x30000, gt=0x30000 + 6 * 9 * 3 - 1, err=0x40000), -1),
    ("u8 overlaps mask", dict(u8=0x50000, mask=0x50000 - 8 * 12 + 1), -1),
    ("workspace overlaps disp", dict(rgb=0x30000, workspace=0x10000 + 4, flags=_lib.DSM_ENCODE_AUTO_RANGE), -1),
    ("disp not 4-byte aligned", dict(disp=0x10002), -4),
    ("gt not 4-byte aligned", dict(gt=0x30001, err=0x40000), -4),
    ("u16 not 2-byte aligned", dict(u16=0x20001), -4),
    ("2^31 source elements", dict(B=2, Hs=32768, Ws=32768, disp=0x10, u16=1 << 40), -2),
]


@pytest.mark.parametrize("why,change,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_return_codes(hip_lib, why, change, code):
    assert hip_lib.dsm_disp_encode(ctypes.byref(_args(**change)), None) == code, why


def test_null_args_and_workspace_size(hip_lib):
    assert hip_lib.dsm_disp_encode(None, None) == -1
    assert ctypes.sizeof(_lib.EncodeArgs) == 104
    assert hip_lib.dsm_disp_encode_workspace_bytes(0, 4, 4) == 0
    assert hip_lib.dsm_disp_encode_workspace_bytes(1, 1, 1) == 8
    assert hip_lib.dsm_disp_encode_workspace_bytes(2, 70, 1030) == 2 * 71 * 8      # 70 * 258 groups in blocks of 256
    assert hip_lib.dsm_disp_encode_workspace_bytes(3, 384, 1280) == 3 * 256 * 8    # capped at 256 blocks per image


def test_encode_disparity_refuses_cpu_tensors():
    from dsmnet_amd import costvolume as cv
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.encode_disparity(torch.zeros(1, 4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.encode_disparity(torch.zeros(1, 1, 4, 8), gt=torch.zeros(1, 1, 4, 8), want=("err",))


# ----------------------------------------------------------------------------
# ResultWriter on host arrays, submit's resume path
# ----------------------------------------------------------------------------
def test_result_writer_round_trips_host_arrays(tmp_path):
    from PIL import Image
    from dsmnet_amd.datasets import Dataset_stereo
    from dsmnet_amd.submit import ResultWriter
    rng = np.random.RandomState(3)
    u16 = rng.randint(0, 65536, size=(3, 19, 45)).astype(np.uint16)
    rgb = rng.randint(0, 256, size=(3, 19, 45, 3)).astype(np.uint8)
    u8 = torch.from_numpy(rng.randint(0, 256, size=(3, 19, 45)).astype(np.uint8))      # a CPU tensor is a host array
    names = ["000000_10.png", "000001_10.png", "sub/000002_10.jpg"]
    writer = ResultWriter(str(tmp_path / "out"), threads=3)
    writer.write({"u16": u16, "viridis": rgb}, names)
    writer.write({"u8": u8}, names)
    writer.close()
    stems = ["000000_10", "000001_10", "000002_10"]
    for i, stem in enumerate(stems):
        with Image.open(str(tmp_path / "out" / "u16" / (stem + ".png"))) as im:
            assert im.mode == "I;16" and np.array_equal(np.array(im), u16[i])
        assert np.array_equal(np.array(Image.open(str(tmp_path / "out" / "viridis" / (stem + ".png")))), rgb[i])
        assert np.array_equal(np.array(Image.open(str(tmp_path / "out" / "u8" / (stem + ".png")))), u8[i].numpy())
    # the dataset layer reads the 16-bit file back as q / 256
    left = [str(tmp_path / "out" / "viridis" / (s + ".png")) for s in stems]
    disp = [str(tmp_path / "out" / "u16" / (s + ".png")) for s in stems]
    ds = Dataset_stereo(left, left, disp, disp_png="kitti")
    for i in range(3):
        sample, _ = ds[i]
        assert sample.dtype == np.float32 and np.array_equal(sample[:, :, 6], u16[i].astype(np.float32) / F(256.0))


def test_result_writer_surfaces_a_worker_error_in_close(tmp_path):
    from dsmnet_amd.submit import ResultWriter
    writer = ResultWriter(str(tmp_path / "out"), threads=2)
    good = np.zeros((1, 4, 5), np.uint16)
    bad = np.zeros((1, 4, 5), np.float64)                    # no PNG holds float64: the worker fails
    writer.write({"u16": good}, ["a.png"])
    writer.write({"u16": bad}, ["b.png"])
    writer.write({"u16": good}, ["c.png"])                   # the writer goes on
    with pytest.raises(Exception):
        writer.close()
    assert os.path.exists(str(tmp_path / "out" / "u16" / "a.png")) and os.path.exists(str(tmp_path / "out" / "u16" / "c.png"))
    with pytest.raises(ValueError, match="file names"):
        ResultWriter(str(tmp_path / "out2")).write({"u16": good}, ["a.png", "b.png"])


class _NeverCalled(torch.nn.Module):
    def forward(self, *a, **k):
        raise AssertionError("the resume path runs no forward")


def test_submit_prints_from_an_existing_result_file(tmp_path, capsys):
    from dsmnet_amd.submit import submit
    out = str(tmp_path / "kitti_stub")
    data = {"filename": ["000000_10.png", "000001_10.png"], "time": [0.25, 0.75], "D1": [1.5, 2.5], "epe": [0.5, 1.0]}
    torch.save(data, out + ".pkl")
    assert submit(_NeverCalled(), None, out) == data
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "submit: 000000_10.png | time:  0.250, D1:  1.500, epe:  0.500"
    assert lines[1] == "submit: 000001_10.png | time:  0.750, D1:  2.500, epe:  1.000"
    assert [float(v) for v in lines[2].split()] == [0.5, 2.0, 0.75]
    assert not os.path.exists(out)                           # nothing was written
    # without ground truth: the time alone
    torch.save({"filename": ["a.png"], "time": [0.5], "D1": [], "epe": []}, out + "2.pkl")
    submit(_NeverCalled(), None, out + "2")
    assert capsys.readouterr().out.splitlines() == ["submit: a.png | time:  0.500", "0.5"]


def test_submit_refuses_unknown_formats(tmp_path):
    from dsmnet_amd.submit import submit
    with pytest.raises(ValueError, match="formats"):
        submit(_NeverCalled(), None, str(tmp_path / "x"), formats=("png",))
