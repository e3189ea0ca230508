"""Absolute maxima that outlive their ``amax_scope``, on the GPU, in the fp16 convolution modes.

``Conv3dFunction`` / ``Conv2dFunction`` save their INPUT for backward, and autograd hands the same Python
object back, ``_dsm_amax`` included: the backward's weight-gradient (and, transposed, the data) kernels scale
the saved input by the power of two taken from that slot.  A forward of another batch in between begins the
arena again -- the slot is zeroed and refilled with ANOTHER tensor's maximum.  Every sequence here is
forward, forward, backward (gradient accumulation; a validation forward before ``backward()``) with each
forward in an ``amax_scope`` of its own, as ``PSMNet.forward`` / ``gcnet.forward`` open one; dX and dW of
the FIRST forward are held against float64 CPU autograd of the same layer to the bounds of
tests/test_train_f16_gpu.py: 1e-3 (``f16x2``) / 4e-3 (``f16``) of max(1, the largest reference entry).

What a stale slot does to dW without the generation check in ``amax_of`` (by the arithmetic of
``dsm_amax_exponent``: the operand is scaled so that the slot's value lands in [2^12, 2^13), fp16 ends at 2^16,
its smallest normal is 2^-14):
  sequence 1  the slot holds a maximum 2^12 too small: the saved input reaches ~2^25 -- inf, NaN in dW;
  sequence 2  the slot holds a maximum 2^30 too large: the saved input lands near 2^-17 -- dW almost zero;
  sequence 4  the slot holds zero: scale 2^60 -- inf, NaN in dW.

The second half pins ``absmax`` on tensors that are not dense float32 at an aligned address."""
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import maxerr, seeded

pytestmark = pytest.mark.gpu

TOL = {"f16x2": 1e-3, "f16": 4e-3}           # tests/test_train_f16_gpu.py: of max(1, max |reference|)
MODES = ["f16x2", "f16"]
# the smallest shapes of tests/test_train_f16_gpu.py: x shape, weight shape
LAYERS = {
    "conv3d": ((1, 32, 6, 12, 40), (32, 32, 3, 3, 3)),
    "deconv3d": ((1, 64, 3, 5, 17), (64, 32, 3, 3, 3)),
    "conv2d": ((2, 32, 40, 70), (32, 32, 3, 3)),
}
SMALL, LARGE = 2.0 ** -12, 2.0 ** 30         # both powers of two, a * 2^30 ~ 5e9 far inside fp32: float64 untouched


@pytest.fixture(scope="module")
def cv(hip_lib):
    from dsmnet_amd import costvolume
    return costvolume


@contextmanager
def precision(cv, mode):
    old = cv.set_option("conv_precision", mode)
    try:
        yield
    finally:
        cv.set_option("conv_precision", old)


def run_layer(cv, kind, x, w):
    if kind == "conv3d":
        return cv.conv3d(x, w, None, 1, False)
    if kind == "deconv3d":
        return cv.conv3d(x, w, None, 2, True)
    return cv.conv2d(x, w, 1, 1)


_REF = {}


def reference(kind):
    """(a, w, cot, dX, dW): float64 CPU autograd of the layer, computed once per layer and left unchanged."""
    if kind not in _REF:
        xs, ws = LAYERS[kind]
        a = seeded(1, *xs)
        w = seeded(2, *ws, scale=0.1)
        a64, w64 = a.double().requires_grad_(True), w.double().requires_grad_(True)
        if kind == "conv3d":
            y = F.conv3d(a64, w64, None, stride=1, padding=1)
        elif kind == "deconv3d":
            y = F.conv_transpose3d(a64, w64, None, stride=2, padding=1, output_padding=1)
        else:
            y = F.conv2d(a64, w64, None, stride=1, padding=1)
        cot = seeded(4, *y.shape)
        gx, gw = torch.autograd.grad(y, [a64, w64], cot.double())
        _REF[kind] = (a, w, cot, gx, gw)
    return _REF[kind]


def check(mode, what, got, ref):
    err, top = maxerr(got, ref), ref.abs().max().item()
    finite = bool(torch.isfinite(got).all())
    print("%s %s: max error %.3e of largest entry %.3e (%.2e relative), finite %s"
          % (mode, what, err, top, err / max(1.0, top), finite))
    assert finite, what
    assert err <= TOL[mode] * max(1.0, top), (what, err, top)


def dev(cv):
    return torch.device("cuda", torch.cuda.current_device())


def first_forwards_gradients(cv, kind, factor, safe, between="forward"):
    """dX, dW of forward(a) when forward(a * factor) under no_grad (``between`` = "forward") or a scope that
    takes no slot ("empty") comes before its backward (``safe``: after it, inside forward(a)'s own scope)."""
    a, w, cot, _, _ = reference(kind)
    ag, wg = a.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    bg, cg = (a * factor).cuda(), cot.cuda()
    grads = None
    with cv.amax_scope(dev(cv)):
        y = run_layer(cv, kind, ag, wg)
        if safe:
            grads = torch.autograd.grad(y, [ag, wg], cg)
    with cv.amax_scope(dev(cv)):
        if between == "forward":
            with torch.no_grad():
                yb = run_layer(cv, kind, bg, wg)
    if not safe:
        grads = torch.autograd.grad(y, [ag, wg], cg)
    if between == "forward":                   # the forward in between is itself right (linear in x)
        assert maxerr(yb, y.detach() * factor) <= 2 * TOL[cv.get_option("conv_precision")] * factor * max(
            1.0, y.abs().max().item())
    return grads


@pytest.mark.parametrize("safe", [False, True], ids=["fwd-fwd-bwd", "fwd-bwd-fwd"])
@pytest.mark.parametrize("factor", [SMALL, LARGE], ids=["seq1-b=a*2^-12", "seq2-b=a*2^30"])
@pytest.mark.parametrize("kind", sorted(LAYERS))
@pytest.mark.parametrize("mode", MODES)
def test_backward_after_a_forward_of_another_batch(cv, mode, kind, factor, safe):
    """Sequences 1 and 2: forward(a), forward(b) under no_grad, backward(a).  The slot a's saved input carries
    then holds max |b|: 2^12 too small (a scaled by it reaches ~2^25, past fp16: inf/NaN) or 2^30 too large
    (a lands near 2^-17, below fp16's smallest normal 2^-14: dW almost zero).  ``fwd-bwd-fwd`` is the order
    that was always safe, held to the same bound."""
    _, _, _, gx, gw = reference(kind)
    with precision(cv, mode):
        dx, dw = first_forwards_gradients(cv, kind, factor, safe)
    check(mode, "%s dX" % kind, dx, gx)
    check(mode, "%s dW" % kind, dw, gw)


@pytest.mark.parametrize("kind", sorted(LAYERS))
@pytest.mark.parametrize("mode", MODES)
def test_backward_after_a_scope_that_took_no_slot(cv, mode, kind):
    """Sequence 4: the scope in between launches nothing, but beginning it zeroes the arena: a zero maximum is
    scale 2^60 (``dsm_amax_exponent``), the saved input turns into fp16 infinities."""
    _, _, _, gx, gw = reference(kind)
    with precision(cv, mode):
        dx, dw = first_forwards_gradients(cv, kind, 1.0, False, between="empty")
    check(mode, "%s dX" % kind, dx, gx)
    check(mode, "%s dW" % kind, dw, gw)


@pytest.mark.parametrize("safe", [False, True], ids=["fwd-fwd-bwd-bwd", "fwd-bwd-fwd-bwd"])
@pytest.mark.parametrize("kind", sorted(LAYERS))
@pytest.mark.parametrize("mode", MODES)
def test_gradient_accumulation_over_two_forwards(cv, mode, kind, safe):
    """Sequence 3: forward(a), forward(b = a * 2^-12), then both backwards into the same ``.grad``: dW is the
    float64 sum dW(a) + dW(b) = dW(a) (1 + 2^-12) (the layer is linear in x), dX is the same for both."""
    a, w, cot, gx, gw = reference(kind)
    with precision(cv, mode):
        ag, wg = a.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
        bg, cg = (a * SMALL).cuda().requires_grad_(True), cot.cuda()
        with cv.amax_scope(dev(cv)):
            ya = run_layer(cv, kind, ag, wg)
            if safe:
                ya.backward(cg)
        with cv.amax_scope(dev(cv)):
            yb = run_layer(cv, kind, bg, wg)
            if safe:
                yb.backward(cg)
        if not safe:
            ya.backward(cg)
            yb.backward(cg)
    check(mode, "%s dX(a)" % kind, ag.grad, gx)
    check(mode, "%s dX(b)" % kind, bg.grad, gx)
    check(mode, "%s dW(a) + dW(b)" % kind, wg.grad, gw * (1.0 + SMALL))


_BN_REF = {}


def bn_reference():
    """BatchNorm3d (batch statistics) + residual + ReLU, then Conv3d 32 -> 32 on (1, 4, 8, 40), in float64."""
    if not _BN_REF:
        y0, res = seeded(11, 1, 32, 4, 8, 40), seeded(12, 1, 32, 4, 8, 40)
        gamma, beta = 1.0 + 0.2 * seeded(13, 32), 0.2 * seeded(14, 32)
        w = seeded(15, 32, 32, 3, 3, 3, scale=0.1)
        leaves = [t.double().requires_grad_(True) for t in (y0, res, gamma, beta, w)]
        h = torch.relu(F.batch_norm(leaves[0], None, None, leaves[2], leaves[3], True, 0.1, 1e-5) + leaves[1])
        out = F.conv3d(h, leaves[4], None, stride=1, padding=1)
        cot = seeded(16, *out.shape)
        grads = torch.autograd.grad(out, leaves, cot.double())
        _BN_REF.update(inputs=(y0, res, gamma, beta, w), cot=cot, grads=grads, out=out.detach())
    return _BN_REF


@pytest.mark.parametrize("safe", [False, True], ids=["fwd-fwd-bwd", "fwd-bwd-fwd"])
@pytest.mark.parametrize("mode", MODES)
def test_bn_epilogue_slot_feeding_a_convolution(cv, mode, safe):
    """Sequence 5: ``bn_add_relu3d`` writes the maximum of its output from its epilogue (``out_amax``) and the
    convolution behind it saves that output -- slot included -- for its weight gradient; the BN backward hands
    on ``dy_amax`` / ``dres_amax`` slots taken outside any scope.  forward(a), forward(b) under no_grad with
    the input scaled by 2^-12, backward(a); checked: the gradients of the convolution weight, of the BN input,
    of the residual, of gamma and beta.

    BatchNorm is scale-invariant (up to eps: the scaled batch's variance 2^-24 is below eps = 1e-5, so its
    output is ~13 times smaller, not 4096 times), so the stale slot here is off by a few binades only: this
    case pins the plumbing (``ctx``, ``out_amax``, ``dy_amax``, ``dres_amax`` through two autograd nodes and a
    recomputed maximum), it does not pin an overflow."""
    ref = bn_reference()
    y0, res, gamma, beta, w = ref["inputs"]
    with precision(cv, mode):
        leaves = [t.cuda().requires_grad_(True) for t in (y0, res, gamma, beta, w)]
        rm, rv = torch.zeros(32, device="cuda"), torch.ones(32, device="cuda")

        def forward(y, r):
            h = cv.bn_add_relu3d(y, leaves[2], leaves[3], r, rm, rv, 1, 0.1, 1e-5)
            return cv.conv3d(h, leaves[4], None, 1, False)
        grads = None
        with cv.amax_scope(dev(cv)):
            out = forward(leaves[0], leaves[1])
            if safe:
                grads = torch.autograd.grad(out, leaves, ref["cot"].cuda())
        with cv.amax_scope(dev(cv)), torch.no_grad():
            forward(leaves[0].detach() * SMALL, leaves[1].detach() * SMALL)
        if not safe:
            grads = torch.autograd.grad(out, leaves, ref["cot"].cuda())
    check(mode, "bn+conv output", out, ref["out"])
    for name, g, r in zip(("d BN input", "d residual", "d gamma", "d beta", "d conv weight"), grads, ref["grads"]):
        check(mode, name, g, r)


class _Names(object):
    def __init__(self, cv):
        self.cv, self.names = cv, []

    def __enter__(self):
        cv, names = self.cv, self.names

        class Timer(cv.LaunchTimer):
            def stop(self, name, start, work):
                names.append(name)
        cv.set_timer(Timer())
        return names

    def __exit__(self, *exc):
        self.cv.set_timer(None)
        return False


@pytest.mark.parametrize("mode", MODES)
def test_no_extra_launch_inside_one_scope_and_one_pass_when_stale(cv, mode):
    """One ``conv3d`` forward plus backward inside ONE scope is five launches of this library, as before slots
    carried a generation: the pass over x, the forward, the pass over dY, backward-data, the weight gradient.
    With the arena begun again before the backward there is exactly one more: the pass over the saved input,
    shared by backward-data and backward-weight."""
    a, w, cot, _, _ = reference("conv3d")
    with precision(cv, mode):
        for stale in (False, True):
            ag, wg = a.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
            with _Names(cv) as names:
                with cv.amax_scope(dev(cv)):
                    y = run_layer(cv, "conv3d", ag, wg)
                    with cv.amax_scope(dev(cv)):               # nested: shares the arena, ends nothing
                        pass
                    if not stale:
                        torch.autograd.grad(y, [ag, wg], cot.cuda())
                if stale:
                    with cv.amax_scope(dev(cv)):
                        pass
                    torch.autograd.grad(y, [ag, wg], cot.cuda())
                torch.cuda.synchronize()
            assert names[0] == "absmax_kernel" and "wgrad" in names[-1], names
            assert sum(n == "absmax_kernel" for n in names) == (3 if stale else 2), names
            assert len(names) == (6 if stale else 5), names


# ------------------------------------------------------------------------------------------------ absmax --
def _absmax_input():
    """(2, 32, 9, 33) float32, |x| <= 4 except 1000.0 in channel 20 (an even row) and -6.5 in channel 3 (an odd
    row), both in the first batch item.  The bound 4 is attained where the cases below need it: in an even
    row of channel 2 and among the first 1004 elements."""
    x = seeded(21, 2, 32, 9, 33).clamp_(-4.0, 4.0)
    x[1, 2, 2, 3] = 4.0
    x[0, 0, 5, 5] = -4.0
    x[0, 20, 4, 7] = 1000.0
    x[0, 3, 5, 2] = -6.5
    return x.cuda()


ABSMAX_VIEWS = {
    "channel-slice": lambda x: x[:, :16],                       # numel() floats from data_ptr() reach channel 20
    "row-stride-2-of-a-slice": lambda x: x[:, :16, ::2],        # even rows only: -6.5 is not an element either
    "row-stride-2": lambda x: x[:, :, ::2],                     # 1000.0 (row 4) is an element, -6.5 is not
    "expanded": lambda x: x[:1, :16].expand(3, -1, -1, -1),     # numel() is three times the memory behind it
    "expanded-whole": lambda x: x[:1].expand(3, -1, -1, -1),
    "misaligned-dense": lambda x: x.flatten()[1:],              # 4 bytes past a 16-byte boundary
    "misaligned-tail": lambda x: x.flatten()[3:3 + 1001],
    "channels-last": lambda x: x.contiguous(memory_format=torch.channels_last),
    "permuted-dense": lambda x: x.permute(0, 2, 3, 1),          # dense, not contiguous: scanned in place
    "dense": lambda x: x,
}


@pytest.mark.parametrize("name", sorted(ABSMAX_VIEWS))
def test_absmax_of_views_is_the_maximum_of_their_elements(cv, name):
    """``absmax`` returns exactly ``t.abs().max()`` for strided, expanded and misaligned float32 views (reduced
    over a dense copy) and for dense tensors in any dimension order (scanned in place), and ``amax_of`` the
    same; the base tensor is left as it was."""
    x = _absmax_input()
    keep = x.clone()
    t = ABSMAX_VIEWS[name](x)
    want = t.abs().max().item()
    trap = {"channel-slice": 6.5, "row-stride-2-of-a-slice": 4.0, "expanded": 6.5, "row-stride-2": 1000.0,
            "expanded-whole": 1000.0, "misaligned-dense": 1000.0, "misaligned-tail": 4.0}
    assert name not in trap or want == trap[name]               # the memory next to the view holds more
    if name.startswith("misaligned"):
        assert t.data_ptr() % 16 != 0
    got = cv.absmax(t)
    assert got.shape == (1,) and got.dtype == torch.float32 and got.item() == want
    assert t._dsm_amax is got
    u = ABSMAX_VIEWS[name](x)                                    # a fresh view object: nothing attached yet
    assert cv.amax_of(u).item() == want and cv.amax_of(u) is u._dsm_amax
    with precision(cv, "f16x2"), cv.amax_scope(dev(cv)):        # and into an arena slot
        assert cv.absmax(ABSMAX_VIEWS[name](x)).item() == want
    assert torch.equal(x, keep)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.int32])
def test_absmax_refuses_other_dtypes_before_any_launch(cv, dtype):
    x = _absmax_input().to(dtype)
    with _Names(cv) as names:
        with pytest.raises(TypeError):
            cv.absmax(x)
        with pytest.raises(TypeError):
            cv.amax_of(x[:, :16])
    assert names == [] and getattr(x, "_dsm_amax", None) is None
    with pytest.raises(ValueError):
        cv.absmax(torch.empty(0, device="cuda"))


def test_a_sliced_input_does_not_overflow_the_convolution(cv):
    """What the wrong bound did downstream: a convolution over a channel slice whose memory neighbour holds a
    value 2^8 larger.  ``to_channels_last_3d`` copies the slice and carries no bound, so this was right before
    too -- pinned because ``carry_amax`` sits on that line."""
    a, w, _, _, _ = reference("conv3d")
    big = torch.cat([a, a * 256.0], 1).cuda()
    with precision(cv, "f16x2"), torch.no_grad(), cv.amax_scope(dev(cv)):
        y = run_layer(cv, "conv3d", big[:, :32], w.cuda())
    ref = F.conv3d(a.double(), w.double(), None, stride=1, padding=1)
    check("f16x2", "conv3d of a channel slice", y, ref)
    assert y._dsm_amax.item() == y.abs().max().item()
