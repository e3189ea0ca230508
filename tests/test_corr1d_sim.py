"""CPU: Corr1d with a similarity argument (``dsm_corr1d_sim_*``, ``costvolume.corr1d(sim=...)``,
``util_conv.Corr1d(simfun=nn.CosineSimilarity(dim=1))``) and the tiled data gradient's dispatch.

* the float64 restatement (tests/corr1d_sim_oracle.py) equals the golden written from the reference's own
  ``Corr1d`` (tests/golden/make_goldens_corr_sim.py);
* the module accepts the cosine similarity and refuses every other callable;
* header, binding and library agree on the new symbols;
* both plan queries send every row of the table below to the branch it names, and a sweep over both sides of
  every threshold finds no other name; plan and launch refuse the same arguments with the same codes.

``SIM_CASES`` is the single source of the rows: tests/test_corr1d_sim_gpu.py runs them on the GPU.  It starts
from ``tests.test_dispatch_plans.CORR_CASES`` (every forward branch) and adds the eligibility limits of the
tiled backward.  Pointers here are fake addresses; a plan query never dereferences them."""
import collections
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from dsmnet_amd import _lib
from tests import corr1d_sim_oracle as CS
from tests import test_dispatch_plans as T
from tests.helpers import seeded
from tests.test_abi import declared_symbols

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_corr_sim.npz")
NEW_SYMBOLS = ["dsm_corr1d_sim_fwd", "dsm_corr1d_sim_fwd_plan", "dsm_corr1d_sim_bwd", "dsm_corr1d_sim_bwd_plan",
               "dsm_corr1d_sim_workspace_bytes"]

# fwd: the name dsm_corr1d_plan gives the row (cosine: with "cos:" in front); bwd: the dot-product name
# (cosine: "prep+" in front of the kernel).
Sim = collections.namedtuple("Sim", "shape D s k offset fwd bwd")
_BWD_OF_CORR_CASES = [
    "bwd_tile<1>", "bwd_tile<1>", "bwd_tile<1>", "bwd_tile<1>", "bwd_tile<1>",
    "bwd_tile<1>",                       # D = 96: the top of the tiled backward
    "bwd_naive",                         # D = 97
    "box3+bwd_tile<2>", "bwd_tile<2>", "box3+bwd_tile<2>",
    "bwd_tile<2>",                       # C = 160: five channel chunks (the forward's window does not fit; this one's does)
    "bwd_tile<1>",                       # C = 20: a partial chunk
    "bwd_tile<1>",                       # C = 40: a whole and a partial chunk
    "bwd_naive", "bwd_naive", "bwd_naive",   # D = 128, 129, 200
    "bwd_naive",                         # W % 4 != 0 at stride 2
    "box3+bwd_naive",                    # misaligned fL, fR (the cotangent and the workspace are aligned: box3)
]
assert len(_BWD_OF_CORR_CASES) == len(T.CORR_CASES)
SIM_CASES = [Sim(c.shape, c.D, c.s, c.k, c.offset, c.plan, b) for c, b in zip(T.CORR_CASES, _BWD_OF_CORR_CASES)] + [
    Sim((1, 8, 2, 40), 5, 3, 1, False, "generic", "bwd_naive"),             # stride 3
    Sim((1, 8, 2, 30), 9, 1, 1, False, "fwd<1>scalar", "bwd_naive"),        # W % 4 != 0 at stride 1
    Sim((1, 16, 2, 40), 5, 1, 5, False, "tile<1,1>+box", "box+bwd_tile<1>"),  # k = 5: the general box filter
    Sim((2, 24, 2, 136), 95, 2, 1, False, "fwd<2>vec", "bwd_tile<2>"),      # Dp = 96 at stride 2: the largest LDS image (115 KB)
]
BWD_KERNELS = {"bwd_tile<1>", "bwd_tile<2>", "bwd_naive"}
BWD_PREFIXES = {"", "box3+", "box+"}


def case_id(c):
    return "%s-D%d-s%d-k%d%s" % ("x".join(map(str, c.shape)), c.D, c.s, c.k, "-offset" if c.offset else "")


def expected(case, sim):
    """(forward name, backward name) of a row for ``sim``."""
    if sim == "dot":
        return case.fwd, case.bwd
    head, sep, kern = case.bwd.rpartition("+")
    return "cos:" + case.fwd, head + sep + "prep+" + kern


def plans(case, sim, flags=0):
    from dsmnet_amd import costvolume as cv
    B, C, H, W = case.shape
    p = T._ptr(T.A16)
    f = T._ptr(T.OFF4 if case.offset else T.A16)
    fwd = cv.corr1d_sim_fwd_plan_name(f, f, p, p if case.k > 1 else None, p if sim == "cosine" else None,
                                      B, C, H, W, case.D, case.s, case.k, sim)
    need_ws = case.k > 1 or sim == "cosine"
    bwd = cv.corr1d_sim_bwd_plan_name(p, f, f, p if sim == "cosine" else None, p if sim == "cosine" else None, p, p,
                                      p if need_ws else None, B, C, H, W, case.D, case.s, case.k, sim, flags=flags)
    return fwd, bwd


# ------------------------------------------------------------------------------ the restatement --
def _golden():
    z = np.load(GOLDEN, allow_pickle=False)
    return z, json.loads(bytes(z["meta"]).decode())


def test_restatement_equals_the_reference_golden():
    z, meta = _golden()
    assert os.path.getsize(GOLDEN) <= 256 * 1024
    assert [c["tag"] for c in meta["cases"]] == ["k1_s1_D9", "k3_s2_D5", "k1_s1_D30", "degenerate_k1_s1_D9"]
    for c in meta["cases"]:
        fL, fR = torch.from_numpy(z[c["inputs"] + ".fL"]), torch.from_numpy(z[c["inputs"] + ".fR"])
        assert fL.dtype == torch.float64 and tuple(fL.shape) == (2, 16, 3, 24)
        cot = seeded(meta["seeds"]["cot"], 2, c["D"], 3, 24).double()
        out, gL, gR = CS.with_grads(fL, fR, cot, c["D"], c["s"], c["k"], meta["eps"])
        assert out.dtype == torch.float64
        assert (out - torch.from_numpy(z[c["tag"] + ".out"])).abs().max().item() <= 1e-12
        for mine, name in ((gL, ".dL"), (gR, ".dR")):
            ref = torch.from_numpy(z[c["tag"] + name])
            assert torch.isfinite(mine).all()
            # (the degenerate case holds entries of 1e8: relative to the largest entry there)
            assert (mine - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


def test_degenerate_golden_is_degenerate():
    z, meta = _golden()
    fL, fR = torch.from_numpy(z["degenerate_inputs.fL"]), torch.from_numpy(z["degenerate_inputs.fR"])
    rL, rR = CS.make_degenerate(torch.from_numpy(z["inputs.fL"]).clone(), torch.from_numpy(z["inputs.fR"]).clone())
    assert torch.equal(fL, rL) and torch.equal(fR, rR)
    out = torch.from_numpy(z["degenerate_k1_s1_D9.out"])
    assert out[0, :, 0, 3].abs().max().item() == 0.0            # a zero left vector: exactly 0, not NaN
    assert out[0, 0, 1, 5].item() == 0.0
    assert 0 < fL[0, :, 1, 7].norm().item() < 1e-8
    assert torch.from_numpy(z["degenerate_k1_s1_D9.dL"]).abs().max().item() > 1e7
    # the restatement follows F.cosine_similarity of the installed torch: each norm clamped on its own
    ref = nn.CosineSimilarity(dim=1)(fL, fR)
    assert (CS.corr1d_cosine(fL, fR, 1)[:, 0] - ref).abs().max().item() <= 1e-12


# ------------------------------------------------------------------------------------ the module --
def test_module_accepts_cosine_similarity_and_keeps_eps():
    from dsmnet_amd.models.util_conv import Corr1d
    m = Corr1d(3, 2, 41, simfun=nn.CosineSimilarity(dim=1, eps=1e-6))
    assert (m.sim, m.eps, m.kernel_size, m.stride, m.D) == ("cosine", 1e-6, 3, 2, 41)
    assert "CosineSimilarity" in repr(m) and "1e-06" in repr(m)
    assert Corr1d(1, 1, 41, simfun=nn.CosineSimilarity(dim=1)).eps == 1e-8
    d = Corr1d(1, 1, 41)
    assert d.sim == "dot" and "simfun" not in repr(d)
    assert list(m.state_dict()) == []


@pytest.mark.parametrize("simfun", [nn.CosineSimilarity(dim=2), lambda a, b: (a * b).sum(1), nn.PairwiseDistance()],
                         ids=["cosine-dim2", "lambda", "pairwise"])
def test_module_refuses_other_similarities(simfun):
    from dsmnet_amd.models.util_conv import Corr1d
    with pytest.raises(NotImplementedError):
        Corr1d(1, 1, 9, simfun=simfun)


def test_op_refuses_cpu_tensors_and_unknown_similarities():
    from dsmnet_amd import costvolume as cv
    a, b = torch.zeros(1, 4, 2, 8), torch.zeros(1, 4, 2, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.corr1d(a, b, 3, sim="cosine")
    with pytest.raises(ValueError):
        cv.corr1d(a, b, 3, sim="l2")
    assert cv.get_option("corr1d_tiled_bwd") is False


# --------------------------------------------------------------------------------------- the ABI --
def test_header_binding_and_exports_agree_on_the_new_symbols(hip_lib):
    syms = declared_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in syms and name in _lib.SIGNATURES and hasattr(raw, name), name
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "dsmnet_hip.h")).read()
    assert "DSM_SIM_DOT = 0, DSM_SIM_COSINE = 1" in header and "#define DSM_CORR_BWD_NAIVE 1" in header
    assert (_lib.DSM_SIM_DOT, _lib.DSM_SIM_COSINE, _lib.DSM_CORR_BWD_NAIVE) == (0, 1, 1)
    assert hip_lib.dsm_abi_version() == 7


def test_workspace_bytes(hip_lib):
    ws = hip_lib.dsm_corr1d_sim_workspace_bytes
    r = lambda n: (n + 255) // 256 * 256
    B, C, H, W, D = 2, 16, 3, 72, 41
    m, t = r(B * D * H * W * 4), r(2 * B * H * W * 4)
    assert ws(B, C, H, W, D, 1, 0) == 0
    assert ws(B, C, H, W, D, 3, 0) == m
    assert ws(B, C, H, W, D, 1, 1) == m + t
    assert ws(B, C, H, W, D, 3, 1) == 2 * m + t
    assert ws(0, C, H, W, D, 3, 1) == 0


# ------------------------------------------------------------------------------------- the plans --
@pytest.mark.parametrize("sim", ["dot", "cosine"])
@pytest.mark.parametrize("case", SIM_CASES, ids=case_id)
def test_case_lands_on_its_branches(hip_lib, case, sim):
    assert plans(case, sim) == expected(case, sim)
    # flags bit 0: the naive kernel, whatever the row is eligible for
    forced = plans(case, sim, _lib.DSM_CORR_BWD_NAIVE)[1]
    assert forced == expected(case, sim)[1].replace("bwd_tile<%d>" % case.s, "bwd_naive")


def test_dot_rows_agree_with_the_old_plan_query(hip_lib):
    for c in T.CORR_CASES:
        case = SIM_CASES[T.CORR_CASES.index(c)]
        assert plans(case, "dot")[0] == T.corr_plan(hip_lib, c) == c.plan


def test_the_table_reaches_every_branch(hip_lib):
    fk, fs, bk, bp = set(), set(), set(), set()
    for c in SIM_CASES:
        for sim in ("dot", "cosine"):
            fwd, bwd = plans(c, sim)
            assert fwd.startswith("cos:") == (sim == "cosine") and ("prep+" in bwd) == (sim == "cosine")
            k, plus, suffix = fwd[4 if sim == "cosine" else 0:].partition("+")
            fk.add(k)
            fs.add(plus + suffix)
            head, sep, kern = bwd.replace("prep+", "").rpartition("+")
            bk.add(kern)
            bp.add(head + sep)
    assert fk == T.CORR_KERNELS and fs == T.CORR_SUFFIXES
    assert bk == BWD_KERNELS and bp == BWD_PREFIXES


def test_plan_names_cover_the_whole_argument_space(hip_lib):
    """Both sides of every threshold of ``pick_corr`` / ``pick_corr_bwd`` (D, C, W, stride, box size, alignment of
    every pointer, the forcing flag, the similarity): no name outside the sets."""
    from dsmnet_amd import costvolume as cv
    p, q = T._ptr(T.A16), T._ptr(T.OFF4)
    fk, fs, bk, bp = set(), set(), set(), set()
    for D in (1, 11, 48, 49, 96, 97, 128, 129, 300):
        for C in (8, 16, 160, 400):
            for W in (30, 64):
                for s in (1, 2, 3):
                    for k in (1, 3, 5):
                        for sim in ("dot", "cosine"):
                            cos = sim == "cosine"
                            for bad in range(6):          # which pointer is misaligned (0: none)
                                fl, out, inv = (q if bad == 1 else p), (q if bad == 2 else p), (q if bad == 3 else p)
                                name = cv.corr1d_sim_fwd_plan_name(fl, p, out, p if k > 1 else None, inv if cos else None,
                                                                   1, C, 2, W, D, s, k, sim)
                                assert name.startswith("cos:") == cos
                                kern, plus, suffix = name[4 if cos else 0:].partition("+")
                                fk.add(kern)
                                fs.add(plus + suffix)
                                g, dl, ws = (q if bad == 3 else p), (q if bad == 4 else p), (q if bad == 5 else p)
                                for flags in (0, 1):
                                    name = cv.corr1d_sim_bwd_plan_name(g, fl, p, p if cos else None, p if cos else None,
                                                                       dl, p, ws if (k > 1 or cos) else None, 1, C, 2, W,
                                                                       D, s, k, sim, flags=flags)
                                    assert ("prep+" in name) == cos
                                    head, sep, kern = name.replace("prep+", "").rpartition("+")
                                    assert kern in BWD_KERNELS and (head + sep) in BWD_PREFIXES, name
                                    tile = (flags == 0 and s in (1, 2) and W % 4 == 0 and D <= 96 and bad not in (1, 4)
                                            and not (bad == 5 and (k > 1 or cos)) and not (bad == 3 and k == 1 and not cos))
                                    assert kern == ("bwd_tile<%d>" % s if tile else "bwd_naive"), (name, D, C, W, s, k, sim, bad)
                                    bk.add(kern)
                                    bp.add(head + sep)
    assert fk == T.CORR_KERNELS and fs == T.CORR_SUFFIXES
    assert bk == BWD_KERNELS and bp == BWD_PREFIXES


def test_plans_and_launches_return_the_same_error_codes(hip_lib):
    """Every refusal below comes from the shared selection code, before any launch: fake pointers are safe."""
    null, one, off = None, ctypes.c_void_p(T.A16), ctypes.c_void_p(T.OFF4)
    buf = ctypes.create_string_buffer(96)
    eps = 1e-8

    def fwd(fL, fR, out, raw, inv, B, C, H, W, D, s, k, sim, e, dtype=0):
        a = hip_lib.dsm_corr1d_sim_fwd_plan(fL, fR, out, raw, inv, B, C, H, W, D, s, k, sim, e, dtype, buf, 96)
        assert a != 0                       # (a launch is only ever asked for what the plan has refused)
        assert hip_lib.dsm_corr1d_sim_fwd(fL, fR, out, raw, inv, B, C, H, W, D, s, k, sim, e, dtype, null) == a
        return a

    def bwd(g, fL, fR, raw, inv, dL, dR, ws, B, C, H, W, D, s, k, sim, e, flags=0, dtype=0):
        a = hip_lib.dsm_corr1d_sim_bwd_plan(g, fL, fR, raw, inv, dL, dR, ws, B, C, H, W, D, s, k, sim, e, flags, dtype, buf, 96)
        assert a != 0
        assert hip_lib.dsm_corr1d_sim_bwd(g, fL, fR, raw, inv, dL, dR, ws, B, C, H, W, D, s, k, sim, e, flags, dtype, null) == a
        return a

    assert fwd(null, null, null, null, null, 1, 1, 1, 1, 1, 1, 1, 0, eps) == -1
    assert fwd(one, one, one, null, one, 1, 8, 4, 4, 4, 1, 2, 1, eps) == -1          # even k
    assert fwd(one, one, one, null, one, 1, 8, 4, 4, 4, 1, 3, 1, eps) == -1          # no raw map for k = 3
    assert fwd(one, one, one, null, one, 1, 8, 4, 4, 4, 1, 1, 1, eps, dtype=7) == -2  # dtype
    assert fwd(one, one, one, null, one, 1, 8, 4, 4, 4, 1, 1, 5, eps) == -1          # unknown similarity
    assert fwd(one, one, one, null, null, 1, 8, 4, 4, 4, 1, 1, 1, eps) == -1         # cosine without inv
    assert fwd(one, one, one, null, one, 1, 8, 4, 4, 4, 1, 1, 1, 0.0) == -1          # eps = 0
    assert fwd(one, one, one, null, one, 1, 8, 4, 4, 4, 1, 1, 1, float("nan")) == -1
    assert fwd(one, one, one, null, one, 1, 8, 65535, 40000, 4, 1, 1, 1, eps) == -2  # B H W = 2.6e9 pixels
    assert fwd(one, one, one, null, null, 1, 8, 65535, 40000, 4, 1, 1, 0, eps) == -2  # ... for the dot product too
    assert fwd(one, one, one, null, one, 1, 8, 4, 8, 4, 1 << 30, 1, 1, eps) == -2    # x + D stride wraps an int
    assert fwd(one, one, one, null, one, 1, 8, 70000, 4, 4, 1, 1, 1, eps) == -2      # H above the grid's limit
    assert hip_lib.dsm_corr1d_sim_fwd_plan(one, one, one, null, one, 1, 8, 4, 4, 4, 1, 1, 1, eps, 0, null, 96) == -1
    assert hip_lib.dsm_corr1d_sim_fwd_plan(one, one, one, null, null, 1, 8, 4, 4, 4, 1, 1, 0, 0.0, 0, buf, 96) == 0   # dot: eps unused
    assert buf.value == b"fwd<1>vec"

    assert bwd(null, one, one, one, one, one, one, one, 1, 8, 4, 4, 4, 1, 1, 1, eps) == -1
    assert bwd(one, one, one, one, one, null, one, one, 1, 8, 4, 4, 4, 1, 1, 1, eps) == -1       # no dfL
    assert bwd(one, one, one, null, one, one, one, one, 1, 8, 4, 4, 4, 1, 1, 1, eps) == -1       # cosine without the map
    assert bwd(one, one, one, one, null, one, one, one, 1, 8, 4, 4, 4, 1, 1, 1, eps) == -1       # ... without inv
    assert bwd(one, one, one, one, one, one, one, null, 1, 8, 4, 4, 4, 1, 1, 1, eps) == -1       # ... without workspace
    assert bwd(one, one, one, null, null, one, one, null, 1, 8, 4, 4, 4, 1, 3, 0, eps) == -1     # dot, k = 3, no workspace
    assert bwd(one, one, one, one, one, one, one, one, 1, 8, 4, 4, 4, 1, 1, 1, eps, flags=2) == -1
    assert bwd(one, one, one, one, one, one, one, one, 1, 8, 4, 4, 4, 1, 1, 3, eps) == -1        # similarity
    assert bwd(one, one, one, one, one, one, one, one, 1, 8, 4, 4, 4, 1, 1, 1, -1.0) == -1
    assert bwd(one, one, one, one, one, one, one, one, 1, 8, 4, 4, 4, 1, 1, 1, eps, dtype=7) == -2
    assert bwd(one, one, one, one, one, one, one, one, 1, 8, 65535, 40000, 4, 1, 1, 1, eps) == -2
    assert bwd(one, one, one, one, one, one, one, one, 1, 70000, 4, 4, 4, 1, 1, 1, eps) == -2    # B C above the grid's limit
    assert hip_lib.dsm_corr1d_sim_bwd_plan(one, one, one, null, null, one, one, null, 1, 8, 4, 4, 4, 1, 1, 0, eps, 0, 0, buf, 96) == 0
    assert buf.value == b"bwd_tile<1>"
    assert hip_lib.dsm_corr1d_sim_bwd_plan(one, off, one, null, null, one, one, null, 1, 8, 4, 4, 4, 1, 1, 0, eps, 0, 0, buf, 96) == 0
    assert buf.value == b"bwd_naive"
