"""Lifetime of the absolute-maximum slots of the fp16 convolution modes (``costvolume._AmaxArena``,
``amax_scope``, ``amax_of``, ``carry_amax``), on the host: the arena is plain torch and runs on the CPU.

A slot is a view of one per-device buffer that every outermost ``amax_scope`` zeroes and hands out again
from index 0, while tensors of the earlier scope (an input saved for backward, an output the caller kept)
still carry theirs as ``_dsm_amax``.  What is pinned: ``amax_of`` never serves such a slot -- it asks
``absmax`` for a fresh pass instead (``absmax`` is the one launch of this path; a recording stand-in
computes it with torch here, there is no GPU) -- and serves every slot that is still good without a pass."""
from contextlib import contextmanager

import pytest
import torch

from dsmnet_amd import costvolume as cv

CPU = torch.device("cpu")
META = torch.device("meta")


@contextmanager
def precision(mode):
    old = cv.set_option("conv_precision", mode)
    try:
        yield
    finally:
        cv.set_option("conv_precision", old)


@pytest.fixture
def f16x2():
    with precision("f16x2"):
        yield


@pytest.fixture
def passes(monkeypatch):
    """Stand-in for the ``dsm_absmax`` launch: records the tensors ``amax_of`` asks a fresh pass for."""
    asked = []

    def absmax(x):
        asked.append(x)
        slot = cv._ARENA.slot(x.device)
        slot.copy_(x.detach().abs().max().reshape(1))
        x._dsm_amax = slot
        return slot
    monkeypatch.setattr(cv, "absmax", absmax)
    return asked


def produced(value, shape=(4,)):
    """A tensor as a launch inside the current scope leaves it: max |t| = value, written to a fresh slot."""
    t = torch.full(shape, float(value))
    t._dsm_amax = cv._ARENA.slot(t.device)
    t._dsm_amax.fill_(float(value))
    return t


def test_a_slot_of_an_earlier_scope_is_not_served(f16x2, passes):
    with cv.amax_scope(CPU):
        a, b = produced(64.0), produced(3.0)
        assert cv.amax_of(a).item() == 64.0 and cv.amax_of(b).item() == 3.0
    assert cv.amax_of(a).item() == 64.0 and cv.amax_of(b).item() == 3.0      # the scope closed: still good
    assert passes == []
    with cv.amax_scope(CPU):
        c = produced(0.5)
        # the buffer was zeroed and its first slot handed to c: what a and b carry is c's maximum and zero
        assert a._dsm_amax.data_ptr() == c._dsm_amax.data_ptr()
        got_a, got_b, got_c = cv.amax_of(a), cv.amax_of(b), cv.amax_of(c)
        assert [id(t) for t in passes] == [id(a), id(b)]                      # recomputed; c's own is served
        assert (got_a.item(), got_b.item(), got_c.item()) == (64.0, 3.0, 0.5)
        assert got_a.data_ptr() != c._dsm_amax.data_ptr() and got_b.data_ptr() != got_a.data_ptr()
        assert cv.amax_of(a) is got_a and len(passes) == 2                    # one pass, then served again
    assert cv.amax_of(a).item() == 64.0 and cv.amax_of(c).item() == 0.5 and len(passes) == 2


def test_a_scope_that_takes_no_slot_still_ends_the_earlier_ones(f16x2, passes):
    with cv.amax_scope(CPU):
        a = produced(64.0)
    with cv.amax_scope(CPU):
        pass
    assert a._dsm_amax.item() == 0.0                  # what a stale read would give: scale 2^60 in the kernels
    assert cv.amax_of(a).item() == 64.0 and [id(t) for t in passes] == [id(a)]


def test_nested_scopes_share_the_outer_arena(f16x2, passes):
    with cv.amax_scope(CPU):
        a = produced(64.0)
        with cv.amax_scope(CPU):
            b = produced(3.0)
            assert b._dsm_amax.data_ptr() == a._dsm_amax.data_ptr() + 4     # the next slot of the same buffer
            assert cv.amax_of(a).item() == 64.0                              # entering zeroed nothing
        c = produced(0.5)                                                    # leaving did neither
        assert c._dsm_amax.data_ptr() == a._dsm_amax.data_ptr() + 8
        assert (cv.amax_of(a).item(), cv.amax_of(b).item(), cv.amax_of(c).item()) == (64.0, 3.0, 0.5)
    assert cv.amax_of(b).item() == 3.0
    assert passes == []


def test_slots_outside_any_scope_are_private_zeros_and_stay_good(f16x2, passes):
    with cv.amax_scope(CPU):
        inside = produced(9.0)
    s1, s2 = cv._ARENA.slot(CPU), cv._ARENA.slot(CPU)
    assert s1.item() == 0.0 and s2.item() == 0.0 and s1.data_ptr() != s2.data_ptr()
    buf = cv._ARENA.buf[("cpu", None)]
    assert not buf.data_ptr() <= s1.data_ptr() < buf.data_ptr() + 4 * buf.numel()
    g = torch.ones(3)                                # a gradient whose producer ran after the scope closed
    g._dsm_amax = s1
    s1.fill_(5.0)
    for _ in range(2):
        with cv.amax_scope(CPU):
            assert cv.amax_of(g) is s1 and s1.item() == 5.0
    assert cv.amax_of(g) is s1
    assert [id(t) for t in passes] == []
    assert cv.amax_of(inside).item() == 9.0 and [id(t) for t in passes] == [id(inside)]


def test_slot_2049_of_one_scope_is_a_private_scalar(f16x2, passes):
    n = cv._AmaxArena.SLOTS
    assert n == 2048
    with cv.amax_scope(CPU):
        slots = [cv._ARENA.slot(CPU) for _ in range(n)]
        buf = cv._ARENA.buf[("cpu", None)]
        assert [s.data_ptr() for s in slots] == [buf.data_ptr() + 4 * i for i in range(n)]
        extra = produced(7.0)
        assert not buf.data_ptr() <= extra._dsm_amax.data_ptr() < buf.data_ptr() + 4 * n
        buf.fill_(1.0)
        assert extra._dsm_amax.item() == 7.0
    with cv.amax_scope(CPU):
        assert cv.amax_of(extra).item() == 7.0 and passes == []              # private: nothing zeroed it


def test_carry_amax_hands_on_validity_with_the_slot(f16x2, passes):
    with cv.amax_scope(CPU):
        src = produced(64.0, (2, 4))
        view = cv.carry_amax(src[:1], src)
        assert view._dsm_amax is src._dsm_amax
        assert cv.amax_of(view) is src._dsm_amax and passes == []
        plain = cv.carry_amax(torch.ones(2), torch.ones(2))                  # no bound to hand on
        assert getattr(plain, "_dsm_amax", None) is None
        two = cv.carry_amax(torch.ones(2), src, produced(1.0))               # two sources: no single bound
        assert getattr(two, "_dsm_amax", None) is None
    with cv.amax_scope(CPU):
        late = cv.carry_amax(src[1:], src)            # carried after the source went stale: stale as well
        for t in (view, late):
            assert cv.amax_of(t).item() == 64.0
        assert [id(t) for t in passes] == [id(view), id(late)]


def test_a_scope_is_a_no_op_without_an_fp16_precision(passes):
    with precision("f16x2"):
        with cv.amax_scope(CPU):
            a = produced(64.0)
        for mode in ("bf16x3", "fp32"):
            with precision(mode):
                assert not cv.needs_amax()
                with cv.amax_scope(CPU) as scope:
                    assert scope.entered is False
                    s = cv._ARENA.slot(CPU)           # nothing opened: a private scalar
                    buf = cv._ARENA.buf[("cpu", None)]
                    assert not buf.data_ptr() <= s.data_ptr() < buf.data_ptr() + 4 * buf.numel()
        assert cv.amax_of(a).item() == 64.0 and a._dsm_amax.item() == 64.0 and passes == []


def test_depth_and_slot_counter_are_per_device(f16x2, passes):
    with cv.amax_scope(CPU):
        old = [produced(7.0) for _ in range(3)]
    with cv.amax_scope(META):
        m_old = [cv._ARENA.slot(META) for _ in range(3)]
        assert [s.storage_offset() for s in m_old] == [0, 1, 2]
        # only META's scope is open: a CPU slot asked for now belongs to no scope
        stray = cv._ARENA.slot(CPU)
        buf = cv._ARENA.buf[("cpu", None)]
        assert not buf.data_ptr() <= stray.data_ptr() < buf.data_ptr() + 4 * buf.numel()
        assert cv.amax_of(old[0]).item() == 7.0 and passes == []            # and CPU's arena is untouched
        with cv.amax_scope(CPU):
            # CPU's scope is an outermost one although META's is open: begun, zeroed, counted from 0
            first = cv._ARENA.slot(CPU)
            assert first.data_ptr() == buf.data_ptr() and first.item() == 0.0
            assert cv._ARENA.slot(CPU).data_ptr() == buf.data_ptr() + 4
            assert buf.abs().max().item() == 0.0
            assert cv.amax_of(old[1]).item() == 7.0 and [id(t) for t in passes] == [id(old[1])]
            assert cv._ARENA.valid(m_old[0])          # META's arena did not begin again
        assert cv._ARENA.slot(META).storage_offset() == 3
    with cv.amax_scope(CPU):
        with cv.amax_scope(META):                     # the other way round
            assert cv._ARENA.slot(META).storage_offset() == 0
            assert not cv._ARENA.valid(m_old[0])
    assert all(d == 0 for d in cv._ARENA.depth.values())


def test_an_exception_inside_a_scope_closes_it(f16x2):
    with pytest.raises(KeyError):
        with cv.amax_scope(CPU):
            with cv.amax_scope(CPU):
                raise KeyError("x")
    assert cv._ARENA.depth[("cpu", None)] == 0


def wide_layer_args():
    """``dsm_conv3d_args`` of a wide 2-D layer (3x3, 256 -> 256 channels), which every fp16 mode runs on a split
    kernel, with its input and output as CPU tensors."""
    from dsmnet_amd import _lib
    a = _lib.Conv3dArgs()
    a.B, a.Cin, a.Cout = 1, 256, 256
    a.Di, a.Hi, a.Wi = a.Do, a.Ho, a.Wo = 1, 4, 4
    a.stride, a.kd, a.k, a.dil = 1, 1, 3, 1
    return a, torch.full((1, 256, 4, 4), 3.0), torch.zeros(1, 256, 4, 4)


def test_the_mode_of_a_launch_is_an_argument_not_the_option(passes):
    """What ``WideConv2dReLUFunction.backward`` relies on: ``_set_precision``, ``_conv_flags``, ``_wgrad_precision``
    and ``needs_amax`` (the slot of ``bias_relu_bwd``) follow the mode they are given, and the option -- which
    other threads read -- is never written."""
    from dsmnet_amd import _lib
    with precision("bf16x3"):
        with cv.amax_scope(CPU):                                                # no fp16 mode: opens nothing
            a, x, y = wide_layer_args()
            keep = cv._set_precision(a, x, y, mode="f16x2")
            assert a.precision == _lib.DSM_PREC_F16X2 and a.x_amax and a.y_amax
            assert y._dsm_amax is keep[1] and a.y_amax == keep[1].data_ptr()
            assert a.x_amax == keep[0].data_ptr() and keep[0].item() == 3.0 and [id(t) for t in passes] == [id(x)]
            assert cv.needs_amax("f16") and not cv.needs_amax()
            g = torch.full((1, 256, 4, 4), 0.5)
            prec, xa, ga = cv._wgrad_precision(x, g, mode="f16")
            assert prec == _lib.DSM_PREC_F16 and xa is keep[0] and ga.item() == 0.5
            assert cv.get_option("conv_precision") == "bf16x3"
    with precision("fp32"):
        assert cv._conv_flags() & _lib.DSM_CONV_FP32_MFMA
        assert not cv._conv_flags(mode="f16x2") & _lib.DSM_CONV_FP32_MFMA
        assert cv.get_option("conv_precision") == "fp32"
    with precision("f16"):
        assert cv._conv_flags(mode="fp32") & _lib.DSM_CONV_FP32_MFMA and not cv._conv_flags()
        assert cv.get_option("conv_precision") == "f16"


@pytest.mark.parametrize("option", ["bf16x3", "fp32", "f16x2", "f16"])
def test_without_a_mode_every_launch_follows_the_option(option, passes):
    from dsmnet_amd import _lib
    want = {"f16x2": _lib.DSM_PREC_F16X2, "f16": _lib.DSM_PREC_F16}.get(option, _lib.DSM_PREC_F32)
    with precision(option), cv.amax_scope(CPU):
        a, x, y = wide_layer_args()
        g = torch.full((1, 256, 4, 4), 0.5)
        for mode in ({}, {"mode": None}):
            keep = cv._set_precision(a, x, y, **mode)
            prec, xa, ga = cv._wgrad_precision(x, g, **mode)
            flags = cv._conv_flags(**mode)
            assert a.precision == want and prec == want
            assert bool(flags & _lib.DSM_CONV_FP32_MFMA) == (option == "fp32")
            if want == _lib.DSM_PREC_F32:
                assert keep is None and xa is None and ga is None and not a.x_amax and not a.y_amax
                assert getattr(y, "_dsm_amax", None) is None and passes == []
            else:
                assert a.x_amax == keep[0].data_ptr() and a.y_amax == y._dsm_amax.data_ptr()
                assert xa is keep[0] and ga.item() == 0.5
        assert cv.needs_amax() == cv.needs_amax(None) == (want != _lib.DSM_PREC_F32)
