"""Every answer of the convolution planner and of the packed-size queries as text, for a diff between two builds
(``DSM_LIB_PATH`` selects the library):  python scripts/dump_conv_plans.py OUT.  For a host WITHOUT a GPU: where the
plan refuses, the line also carries the code of ``dsm_conv3d_fwd``, which returns before any HIP call.
One line per argument set (rc, launch code, plan name, workspace bytes), with ``x_amax`` set and null."""
import ctypes
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsmnet_amd import _lib                                                      # noqa: E402
from tests import test_conv_plans as P, test_extent_plans as X                    # noqa: E402
from tests.test_conv2d_k5_plans import k5_args                                    # noqa: E402
from tests.test_wide2d_plans import wide_args                                     # noqa: E402


def points():
    yield from (a for a, _ in P.sweep())
    yield from (P.row_args(r) for r in P.CASES)
    yield from (P.make_args(m, ci, co, size, 1, s, 0, k, dil, fl) for m, ci, co, size, s, k, dil, fl in P.REFUSED)
    yield from (X.build(mode, ci, co, size, **kw) for _, mode, ci, co, size, kw in X.EXTENT_ROWS)
    for row, bad in itertools.product([("f16x2", 24, 64, (11, 37)), ("f16", 16, 32, (11, 37), 1, 1, 0, 3, 2),
                                       ("f16x2", 64, 64, (3, 11, 37))], ("y", "w_packed", "relu")):
        a = P.make_args(*row)                  # competing refusals: misaligned or out of range on top of the row's own
        setattr(a, bad, 8)
        yield a
    sizes = [(1, 1), (7, 35), (12, 40), (24, 80), (96, 320), (8, 1186), (190, 2033), (1024, 1024)]
    for mode, hw, B, ks in itertools.product(P.PREC, sizes, (1, 2, 5), (0, 1, 5, 63)):
        fl = ks << _lib.DSM_CONV_KSPLIT_SHIFT                  # the wide, transposed wide and 5x5 builders
        for ci, co, s in itertools.product((16, 48, 256, 1024, 2048), (256, 384, 512, 1024), (1, 2)):
            yield wide_args(ci, co, s, mode, hw, B=B, flags=fl)
            yield X.build(mode, ci, co, hw, out=(2 * hw[0] - (B & 1), 2 * hw[1]), B=B, flags=fl)
        for ci, co, s in itertools.product((16, 24, 64, 128), (64, 128, 256), (1, 2)):
            yield k5_args(ci, co, hw, mode, stride=s, B=B, flags=fl)


lib, buf = _lib.load(), ctypes.create_string_buffer(96)
with open(sys.argv[1], "w") as out:
    for a, amax in itertools.product(points(), (16, None)):
        a.x_amax = amax
        rc = lib.dsm_conv3d_plan(ctypes.byref(a), buf, 96)
        fwd = lib.dsm_conv3d_fwd(ctypes.byref(a), None) if rc else 0
        out.write("%d %d %s %d\n" % (rc, fwd, buf.value.decode(), lib.dsm_conv3d_workspace_bytes(ctypes.byref(a))))
    for ci, co, (kd, k) in itertools.product(range(16, 1025, 16), (1, 32, 64, 128, 256, 512, 1024),
                                             ((1, 1), (1, 3), (3, 3), (1, 5), (3, 1))):
        out.write("%d %d %d %d: %d %d\n" % (ci, co, kd, k, lib.dsm_conv_packed_weight_bytes(ci, co, kd, k),
                                            lib.dsm_conv3d_packed_weight_bytes(ci, co, 0)))
text = open(sys.argv[1], "rb").read()
print("%d lines, sha256 %s" % (text.count(b"\n"), hashlib.sha256(text).hexdigest()))
