"""GPU: the fused self-supervised loss with its per-step scalars in device memory
(dsm_selfsup_dyn_*, ``selfsup_pyramid_loss(params=)``) and the captured step built on it
(``graphs.GraphedSelfsupStep``).

Bounds.  The two forms of the op run the same kernels on the same numbers, so loss, aux and every
gather gradient are compared bit for bit; a scatter gradient is an fp32 atomic sum in an order
that differs from launch to launch, and is held to the bound tests/test_selfsup_gpu.py uses for
such a gradient (``_grad_close``).  Graphed against eager training: 2e-3 * max(1, |loss|), the
bound of tests/test_train_gpu.py for the same comparison; graphed against an eager evaluation of
the same weights: 1e-6 relative, the bound of ``test_validate_step_equals_training_loss``."""
import copy

import pytest
import torch

from tests.helpers import maxerr
from tests.test_selfsup_gpu import _grad_close, _selfsup_batch, _smooth

pytestmark = pytest.mark.gpu

B, H, W, LEVELS = 2, 37, 53, [0, 1, 2]           # ragged 16x16 tiles on both axes, six items
# name -> (objective, flag_mask, terms, epsilons per entry, the backward is a pure gather)
NAMES = {
    "depthmono": ("depthmono", False, ("ds", "lr"), 4, False),
    "depthmono-mask": ("depthmono", True, ("ds", "lr"), 4, False),
    "Cap_ds-mask": ("cap", True, ("ds",), 4, True),
    "Cap_ds_lr": ("cap", False, ("ds", "lr"), 4, False),
    "common-mask": ("common", True, ("ds", "lr"), 4, False),
    "SsSMnet-mask": ("sssmnet", True, ("ds", "lr"), 6, False),
}


def _inputs(seed, dlo=1.0, dhi=9.0):
    """As tests/test_selfsup_gpu.py::_case builds them (nedge 0)."""
    g = torch.Generator().manual_seed(seed)
    full = (_smooth(g, B, 6, H, W, 0.0, 1.0, 6) + 0.05 * torch.rand(B, 6, H, W, generator=g)).cuda()
    full1 = torch.flip(full, dims=[-1])
    dLs, dL1s = [], []
    for k in LEVELS:
        hk, wk = -(-H // 2 ** k), -(-W // 2 ** k)
        dLs.append((_smooth(g, B, 1, hk, wk, dlo, dhi, 4) / 2 ** k).cuda().requires_grad_())
        dL1s.append((_smooth(g, B, 1, hk, wk, dlo, dhi, 4) / 2 ** k).cuda().requires_grad_())
    return (full[:, :3], full[:, 3:6], (0, 0), dLs, full1[:, 3:6], full1[:, :3], (0, 0), dL1s, LEVELS)


def _kwargs(name):
    objective, _, terms, _, _ = NAMES[name]
    kw = {"objective": objective, "return_aux": True}
    if objective == "cap":
        kw["terms"] = terms
    if objective in ("cap", "sssmnet"):
        kw["ds_divisors"] = [2 ** k for k in LEVELS]
    return kw


def _scalars(seed, count, lo=1e-5, hi=1.1e-4):
    g = torch.Generator().manual_seed(seed)
    delts = [tuple((lo + (hi - lo) * torch.rand(count, generator=g)).tolist()) for _ in LEVELS]
    weights = (0.2 + torch.rand(len(LEVELS), generator=g)).tolist()
    return delts, weights


def _grads(ins):
    return [d.grad for d in ins[3]] + [d.grad for d in ins[7]]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_host_arguments_and_device_array_agree(hip_lib, name):
    from dsmnet_amd import costvolume as cv
    objective, mask, _, count, gather = NAMES[name]
    delts, weights = _scalars(3, count)
    factors = [2 ** k for k in LEVELS]
    ins = _inputs(12)
    loss, aux = cv.selfsup_pyramid_loss(*ins, weights, factors, mask, delts, **_kwargs(name))
    loss.backward()
    want = [g.clone() for g in _grads(ins)]
    for d in ins[3] + ins[7]:
        d.grad = None
    params = cv.selfsup_step_params(delts, weights, objective, mask).cuda()
    loss2, aux2 = cv.selfsup_pyramid_loss(*ins, None, factors, mask, None, params=params, **_kwargs(name))
    loss2.backward()
    got = _grads(ins)
    torch.cuda.synchronize()
    print("%s: loss %.8f / %.8f" % (name, float(loss.detach()), float(loss2.detach())))
    assert torch.isfinite(loss) and float(loss) != 0.0
    assert torch.equal(loss, loss2) and torch.equal(aux, aux2)
    if gather:
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    else:
        _grad_close(got, [w.double() for w in want], name)
    with pytest.raises(ValueError):                      # a mix of both forms
        cv.selfsup_pyramid_loss(*ins, weights, factors, mask, None, params=params, **_kwargs(name))
    with pytest.raises(ValueError):                      # misaligned
        off = torch.zeros(params.numel() + 1, device="cuda")[1:].view_as(params)
        cv.selfsup_pyramid_loss(*ins, None, factors, mask, None, params=off, **_kwargs(name))


def test_the_device_array_is_read_when_the_graph_runs(hip_lib):
    """Forward + backward of the op captured once; replayed with the array holding A, B, A again:
    every replay gives, bit for bit, the loss of an eager host-argument call with that set."""
    from dsmnet_amd import costvolume as cv
    name = "depthmono-mask"
    objective, mask, _, count, _ = NAMES[name]
    factors = [2 ** k for k in LEVELS]
    ins = _inputs(12)
    sets = [_scalars(s, count, 0.01, 0.2) for s in (21, 22)]       # exaggerated epsilons, other weights
    tables = [cv.selfsup_step_params(d, w, objective, mask) for d, w in sets]
    assert bool((tables[0] != tables[1])[:, [0, 1, 3]].all())       # every float the name reads differs
    eager = []
    for d, w in sets:
        eager.append(cv.selfsup_pyramid_loss(*ins, w, factors, mask, d).detach().clone())
    rel = abs(float(eager[0]) - float(eager[1])) / abs(float(eager[0]))
    print("loss A %.6f, loss B %.6f, rel %.3e" % (float(eager[0]), float(eager[1]), rel))
    assert rel > 1e-3                                    # a condition on the inputs (checked in float64 on the host too)
    params = tables[0].cuda()
    leaves = ins[3] + ins[7]

    def run():
        loss = cv.selfsup_pyramid_loss(*ins, None, factors, mask, None, params=params)
        return loss.detach(), torch.autograd.grad(loss, leaves)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grads = run()
    # C: A's weights with B's epsilons -- the epsilons alone move the loss by ~8e-4 relative (float64)
    sets.append((sets[1][0], sets[0][1]))
    tables.append(cv.selfsup_step_params(*sets[2], objective, mask))
    eager.append(cv.selfsup_pyramid_loss(*ins, sets[2][1], factors, mask, sets[2][0]).detach().clone())
    seen, gseen = [], []
    for k in (0, 1, 0, 2):
        params.copy_(tables[k])
        graph.replay()
        seen.append(loss.clone())
        gseen.append([g.clone() for g in grads])
    torch.cuda.synchronize()
    print("replays: %s" % [float(s) for s in seen])
    assert torch.equal(seen[0], eager[0]) and torch.equal(seen[1], eager[1]) and torch.equal(seen[2], seen[0])
    assert torch.equal(seen[3], eager[2]) and not torch.equal(seen[3], seen[0])
    # the backward read the array too: gradients follow the weights (A and B differ), A twice agrees
    assert not torch.allclose(gseen[0][0], gseen[1][0], rtol=1e-3, atol=0)
    _grad_close(gseen[2], [g.double() for g in gseen[0]], "replay A again")


# ---- GraphedSelfsupStep --------------------------------------------------------------------------
DISP_TOL = 1e-3           # px; the bound of tests/test_graph_state_gpu.py
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_graphs():
    yield
    _RUNS.clear()


def _eval(model, batch):
    model.eval()
    with torch.no_grad():
        out = [d.detach().clone() for d in model(batch[:, :3], batch[:, 3:6])[1]]
    model.train()
    return out


def _trajectory(name, Bn, Hs, Ws, nedge, flat, folds=False):
    """Six eager steps and six graphed steps over three batches from the same initial state, the seed set
    to 100 + k before step k on both sides.  ``folds``: eval forwards around the first three replays."""
    from dsmnet_amd import train
    from dsmnet_amd.graphs import GraphedSelfsupStep
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(0)
    m1 = model_create_by_name("dispnetcorr", 192).cuda()
    m2 = copy.deepcopy(m1)
    batches = [_selfsup_batch(Bn, Hs, Ws, s) for s in (5, 6, 7)]
    lf1, lf2 = (train.selfsup_losses(name, m1.count_levels, 10) for _ in range(2))
    lf1.Weight_Adjust_levels(3)
    lf2.Weight_Adjust_levels(3)
    o1 = train.make_optimizer(m1, lr=1e-4, capturable=True)
    eager = []
    for k, b in enumerate(batches + batches):
        torch.manual_seed(100 + k)
        eager.append(train.train_step_selfsup(m1, o1, lf1, b, nedge=nedge)[0])
    o2 = train.make_optimizer(m2, lr=1e-4, capturable=True)
    assert torch.is_tensor(o2.param_groups[0]["lr"]) and o2.param_groups[0]["lr"].is_cuda
    state = copy.deepcopy(m2.state_dict())
    step = GraphedSelfsupStep(m2, o2, lf2, batches[0], nedge=nedge, warmup=2, flat_gradients=flat)
    assert lf2.step_params is None                        # the loss object is left as it was
    m2.load_state_dict(state)                             # the warm-up and the capture ran real steps: rewind
    for st in o2.state.values():
        for v in st.values():
            if torch.is_tensor(v):
                v.zero_()
    r = dict(model=m2, optim=o2, lossfun=lf2, step=step, batches=batches, eager=eager, graphed=[])
    if folds:
        r["probe"] = _selfsup_batch(Bn, Hs, Ws, 9)
        r["e1"] = _eval(m2, r["probe"])                   # fills every fold cache of the eval path
    for k, b in enumerate(batches + batches):
        torch.manual_seed(100 + k)
        r["graphed"].append(float(step(b)[0]))
        if folds and k == 2:
            r["e2"] = _eval(m2, r["probe"])
            fresh = model_create_by_name("dispnetcorr", 192)
            fresh.load_state_dict(m2.state_dict())
            r["e_fresh"] = _eval(fresh.cuda(), r["probe"])
            del fresh
    print("%s flat=%s: eager %s\n  graphed %s" % (name, flat, ["%.5f" % v for v in eager],
                                                 ["%.5f" % v for v in r["graphed"]]))
    return r


def _single(hip_lib):
    if "single" not in _RUNS:
        _RUNS["single"] = _trajectory("depthmono-mask", 1, 128, 256, 0, False, folds=True)
    return _RUNS["single"]


def _follows(r):
    for a, b in zip(r["eager"], r["graphed"]):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (r["eager"], r["graphed"])
    assert r["graphed"][-1] < r["graphed"][0]


def test_graphed_selfsup_step_follows_the_eager_trajectory(hip_lib):
    r = _single(hip_lib)
    _follows(r)
    assert r["step"].flatgrads is None
    assert len(set(r["graphed"])) == len(r["graphed"])


def test_graphed_selfsup_step_in_its_multi_rank_form(hip_lib):
    r = _trajectory("depthmono-mask", 1, 128, 256, 0, True)
    _follows(r)
    fg = r["step"].flatgrads
    off = 0
    for p in (p for p in r["model"].parameters() if p.requires_grad):
        assert p.grad is not None and p.grad.data_ptr() == fg.flat.data_ptr() + 4 * off
        off += p.numel()
    assert off == fg.total == fg.flat.numel()             # no extra float


def test_graphed_selfsup_step_cap_ds_mask_preset(hip_lib):
    r = _trajectory("Cap_ds-mask", 2, 192, 384, 64, False)
    _follows(r)
    assert r["step"].nedge == 64 and tuple(r["step"].net_in.shape) == (2, 6, 64, 256)


def test_eval_after_graphed_selfsup_steps_equals_a_freshly_built_model(hip_lib):
    r = _single(hip_lib)
    moved, stale = max(maxerr(a, b) for a, b in zip(r["e_fresh"], r["e1"])), \
        max(maxerr(a, b) for a, b in zip(r["e2"], r["e_fresh"]))
    print("|e_fresh - e1| = %.3e px, |e2 - e_fresh| = %.3e px" % (moved, stale))
    assert all(torch.isfinite(d).all() for d in r["e2"] + r["e_fresh"])
    assert moved > 0.0                                    # the three steps changed the output
    assert stale <= DISP_TOL, (stale, moved)


def test_graphed_selfsup_step_does_not_synchronise_the_host(hip_lib):
    r = _single(hip_lib)
    step, batch = r["step"], r["batches"][1]
    step(batch)                                           # a warm call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, _ = step(batch)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)


def test_epsilons_and_weights_are_not_frozen_in_the_graph(hip_lib):
    """Runs last on the shared step: it sets the learning rate to zero and moves the weights."""
    from dsmnet_amd import train
    r = _single(hip_lib)
    step, model, lf, batch = r["step"], r["model"], r["lossfun"], r["batches"][0]
    lr = r["optim"].param_groups[0]["lr"]
    train.lr_adjust(r["optim"], 0, 1, 0.0, 0)             # through the tensor the captured Adam reads
    assert r["optim"].param_groups[0]["lr"] is lr and float(lr) == 0.0
    before = [p.detach().clone() for p in model.parameters()]
    lf_eager = train.selfsup_losses("depthmono-mask", model.count_levels, 10)

    def both(seed):
        lf_eager.weight_levels = list(lf.weight_levels)
        torch.manual_seed(seed)
        got = float(step(batch)[0])
        torch.manual_seed(seed)
        want = train.validate_step_selfsup(model, lf_eager, batch)[0]
        model.train()
        print("seed %d: graphed %.8f, eager %.8f" % (seed, got, want))
        assert abs(got - want) <= 1e-6 * abs(want), (got, want)
        return got
    a, b = both(7), both(8)
    assert a != b                                         # other epsilons, another loss
    assert all(torch.equal(p.detach(), q) for p, q in zip(model.parameters(), before))
    lf.Weight_Adjust_levels(7)                            # new weights, the same levels: no new capture
    c = both(7)
    assert abs(c - a) > 1e-3 * abs(a)
    lf.weight_levels[3] = 0                               # another set of levels is another graph
    with pytest.raises(ValueError, match="enter"):
        step(batch)


def test_constructor_checks(hip_lib):
    from dsmnet_amd import train
    from dsmnet_amd.graphs import GraphedSelfsupStep
    r = _single(hip_lib)
    model, batch = r["model"], r["batches"][0]
    lf = train.selfsup_losses("depthmono-mask", model.count_levels, 10)
    with pytest.raises(ValueError, match="capturable"):
        GraphedSelfsupStep(model, train.make_optimizer(model), lf, batch)
    with pytest.raises(ValueError, match="self-supervised"):
        GraphedSelfsupStep(model, r["optim"], train.losses("supervised", model.count_levels, 10), batch)
    with pytest.raises(ValueError):
        GraphedSelfsupStep(model, r["optim"], lf, batch[:, :5])
