"""CPU: the C ABI of dsm_stereo_spatial_raw (csrc/frames.hip).  The struct's size, the header's
constants against the binding's, and every refusal through ``dsm_stereo_spatial_raw_plan``, the
twin that runs the launch's checks and launches nothing -- so a wrong acceptance cannot touch a
device.  Pointers are made-up addresses: nothing is dereferenced but the source and record arrays."""
import ctypes
import os
import re

import pytest

from dsmnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -4
RAW, Y = 1 << 20, 1 << 30                   # made-up, 4-byte aligned device addresses
HS, WS, H0, W0, H, W = 13, 37, 11, 33, 6, 8
PLANE = HS * WS


def _call(lib, C=8, B=2, n_recs=None, raw=RAW, y=Y, raw_bytes=None, src=None, rec=None, hw0=(H0, W0), hw=(H, W),
          channels=6, srcs_null=False, recs_null=False):
    """A valid call (two images; u16 disparities at even offsets) with the given changes; ``src`` /
    ``rec`` are dicts of fields to overwrite in the LAST image's source / record."""
    fmt = (src or {}).get("disp_format", _lib.DSM_DISP_U16)
    elem = {_lib.DSM_DISP_F32: 4, _lib.DSM_DISP_U8: 1}.get(fmt, 2)
    per = 6 * PLANE + 2 * elem * PLANE + 16
    per += -per % 4
    srcs = (_lib.FrameSource * B)()
    recs = (_lib.SpatialRecord * B)()
    for i in range(B):
        s, r, at = srcs[i], recs[i], i * per
        s.imL, s.imR = at, at + 3 * PLANE
        s.dispL = at + 6 * PLANE + (-(6 * PLANE) % 4)
        s.dispR = s.dispL + elem * PLANE + (-(elem * PLANE) % 4)
        s.Hs, s.Ws, s.y0, s.x0, s.flip, s.disp_format = HS, WS, 2, 3, i % 2, fmt
        r.shift, r.ws, r.hs, r.w, r.h, r.resize = 2, 1, 1, hw[1], hw[0], 0
        r.scale_rand = r.scale_x = r.scale_y = 1.0
    for k, v in (src or {}).items():
        setattr(srcs[B - 1], k, v)
    for k, v in (rec or {}).items():
        setattr(recs[B - 1], k, v)
    if raw_bytes in ("exact", "short"):         # up to the end of the last plane, or one byte less
        raw_bytes = srcs[B - 1].dispR + elem * PLANE - (raw_bytes == "short")
    return lib.dsm_stereo_spatial_raw_plan(
        ctypes.c_void_p(raw), B * per if raw_bytes is None else raw_bytes, None if srcs_null else srcs,
        ctypes.c_void_p(y), None if recs_null else recs, B if n_recs is None else n_recs, B, C, hw0[0], hw0[1],
        hw[0], hw[1], channels)


def test_struct_and_constants_match_the_header(hip_lib):
    assert ctypes.sizeof(_lib.FrameSource) == 64
    assert ctypes.sizeof(_lib.FrameSource) + ctypes.sizeof(_lib.SpatialRecord) == 112
    assert [f[0] for f in _lib.FrameSource._fields_] == ["imL", "imR", "dispL", "dispR", "Hs", "Ws", "y0", "x0",
                                                         "flip", "disp_format", "pad_"]
    header = open(os.path.join(ROOT, "include", "dsmnet_hip.h")).read()
    for name in ("DSM_DISP_F32", "DSM_DISP_U16_256", "DSM_DISP_U16", "DSM_DISP_U8", "DSM_FRAMES_MAX_RECORDS"):
        value = int(re.search(r"#define %s\s+(\d+)" % name, header).group(1))
        assert getattr(_lib, name) == value, name
    assert (_lib.DSM_DISP_F32, _lib.DSM_DISP_U16_256, _lib.DSM_DISP_U16, _lib.DSM_DISP_U8) == (0, 1, 2, 3)
    assert _lib.DSM_FRAMES_MAX_RECORDS == 32
    assert hip_lib.dsm_abi_version() == 7
    assert int(re.search(r"#define DSM_ABI_VERSION (\d+)", header).group(1)) == 7


def test_valid_calls_are_accepted(hip_lib):
    for C in (6, 7, 8):
        for fmt in (_lib.DSM_DISP_F32, _lib.DSM_DISP_U16_256, _lib.DSM_DISP_U16, _lib.DSM_DISP_U8):
            assert _call(hip_lib, C=C, src={"disp_format": fmt}) == OK, (C, fmt)
    assert _call(hip_lib, C=6, src={"dispL": -1, "dispR": -1}) == OK            # absent planes are not looked at
    assert _call(hip_lib, C=7, src={"dispR": -1}) == OK
    assert _call(hip_lib, src={"imL": 1, "imR": 3 * PLANE + 2}) == OK            # RGB at odd offsets
    assert _call(hip_lib, src={"y0": HS - H0, "x0": WS - W0}) == OK              # the frame touches both far edges
    assert _call(hip_lib, channels=0) == OK
    assert _call(hip_lib, raw_bytes="exact") == OK
    assert _call(hip_lib, hw=(5, 7), rec={"resize": 1, "w": 20, "h": 9, "scale_x": 20 / 7.0, "scale_y": 9 / 5.0}) == OK


@pytest.mark.parametrize("why,kwargs", [
    ("raw null", dict(raw=0)),
    ("y null", dict(y=0)),
    ("sources null", dict(srcs_null=True)),
    ("records null", dict(recs_null=True)),
    ("C = 5", dict(C=5)),
    ("C = 9", dict(C=9)),
    ("n_recs != B", dict(n_recs=1)),
    ("B = 0", dict(B=0, n_recs=0)),
    ("C = 7 without dispL", dict(C=7, src={"dispL": -1})),
    ("C = 8 without dispL", dict(C=8, src={"dispL": -1})),
    ("C = 8 without dispR", dict(C=8, src={"dispR": -1})),
    ("unknown disp_format", dict(src={"disp_format": 4})),
    ("negative disp_format", dict(src={"disp_format": -1})),
    ("flip = 2", dict(src={"flip": 2})),
    ("flip = -1", dict(src={"flip": -1})),
    ("y0 < 0", dict(src={"y0": -1})),
    ("x0 < 0", dict(src={"x0": -1})),
    ("frame below the file", dict(src={"y0": HS - H0 + 1})),
    ("frame right of the file", dict(src={"x0": WS - W0 + 1})),
    ("Hs = 0", dict(src={"Hs": 0})),
    ("imL before raw", dict(src={"imL": -1})),
    ("raw one byte short", dict(raw_bytes="short")),
    ("imR past the end", dict(src={"imR": 1 << 40})),
    ("dispL past the end", dict(src={"dispL": 1 << 40})),
    ("dispR offset overflows", dict(src={"dispR": (1 << 63) - 2})),
    ("to_tensor_channels = 3", dict(channels=3)),
    ("shift = W0", dict(rec={"shift": W0})),
    ("shift < 0", dict(rec={"shift": -1})),
    ("window past the shifted frame", dict(rec={"ws": W0 - 2 - W + 1})),
    ("window below the frame", dict(rec={"hs": H0 - H + 1})),
    ("crop window not h x w", dict(rec={"w": W - 1})),
    ("resize = 2", dict(rec={"resize": 2})),
    ("scale_x = 0", dict(rec={"resize": 1, "scale_x": 0.0})),
    ("scale_y = nan", dict(rec={"resize": 1, "scale_y": float("nan")})),
    ("scale_rand = inf", dict(rec={"resize": 1, "scale_rand": float("inf")})),
])
def test_refused_arguments(hip_lib, why, kwargs):
    assert _call(hip_lib, **kwargs) == ARG, why


@pytest.mark.parametrize("why,kwargs", [
    ("y at 2 mod 4", dict(y=Y + 2)),
    ("u16 dispL at an odd offset", dict(src={"dispL": 6 * PLANE + 1})),
    ("u16 planes at an odd address", dict(raw=RAW + 1)),
    ("f32 dispL at 2 mod 4", dict(src={"disp_format": 0, "dispL": 6 * PLANE + (-(6 * PLANE) % 4) + 2})),
    ("f32 dispR at 1 mod 4", dict(C=8, src={"disp_format": 0, "dispR": 1})),
])
def test_refused_alignment(hip_lib, why, kwargs):
    assert _call(hip_lib, **kwargs) == ALIGN, why
    if "raw" in kwargs:                                  # an odd base is fine for bytes
        assert _call(hip_lib, src={"disp_format": _lib.DSM_DISP_U8}, **kwargs) == OK
        assert _call(hip_lib, C=6, **kwargs) == OK


def test_refused_sizes(hip_lib):
    """One plane, one fp32 frame or one output image of 2^31 bytes or more."""
    big = 1 << 40
    # a 26755 x 26755 RGB plane is 3 * 715.8e6 B >= 2^31; a frame of 11 x 33 inside it is fine otherwise
    assert _call(hip_lib, B=1, C=6, raw_bytes=big, src={"Hs": 26755, "Ws": 26755}) == UNSUPPORTED
    assert _call(hip_lib, B=1, C=6, raw_bytes=big, src={"Hs": 26754, "Ws": 26754}) == OK
    # a float32 disparity plane of 23171^2 * 4 B >= 2^31 whose RGB planes are still below it
    f32 = dict(disp_format=0, imL=0, imR=1 << 31, dispL=1 << 32, dispR=1 << 34)
    assert _call(hip_lib, B=1, C=7, raw_bytes=big, src=dict(f32, Hs=23171, Ws=23171)) == UNSUPPORTED
    assert _call(hip_lib, B=1, C=7, raw_bytes=big, src=dict(f32, Hs=23170, Ws=23170)) == OK
    assert _call(hip_lib, B=1, C=6, raw_bytes=big, src=dict(f32, Hs=23171, Ws=23171)) == OK     # not read
    # the fp32 frame: 8192 x 8192 x 8 x 4 B = 2^31
    src = dict(Hs=8200, Ws=8200, y0=0, x0=0, imL=0, imR=1 << 28, dispL=1 << 29, dispR=1 << 30)
    rec = dict(shift=0, ws=0, hs=0)
    assert _call(hip_lib, B=1, C=8, raw_bytes=big, src=src, rec=rec, hw0=(8192, 8192)) == UNSUPPORTED
    assert _call(hip_lib, B=1, C=8, raw_bytes=big, src=src, rec=rec, hw0=(8192, 8191)) == OK
    # the output image: 8192 x 8192 x 8 x 4 B = 2^31 from a small window
    up = dict(rec, resize=1, w=W, h=H, scale_x=W / 8192.0, scale_y=H / 8192.0)
    assert _call(hip_lib, B=1, C=8, rec=up, hw=(8192, 8192)) == UNSUPPORTED
    assert _call(hip_lib, B=1, C=8, rec=up, hw=(8192, 8191)) == OK
