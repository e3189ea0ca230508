"""Host state around ``GraphedTrainStep`` replays: the eval path's cached folds, and the flat gradient views.

A replay runs no Python.  The captured optimizer step (single-process form) and the BN kernels' raw-pointer
writes to the running statistics bump no ``_version``, which is what ``blocks3d._Folded``,
``blocks2d._Folded2d`` and the SPP fold are keyed on: an eval forward after N replays used to serve the packed
weights and BN affines made BEFORE them -- validation inside a graphed training loop looked frozen.  And in
the multi-rank form a ``model.zero_grad()`` (``set_to_none=True`` by default) unbinds ``p.grad`` from the
flat buffer the captured backward keeps writing to: the eager ``optim.step()`` saw no gradient at all.

PSMNet (D = 192), B = 1, 256x256 -- the least its SPP head admits, and the model ``GraphedTrainStep`` is
known to capture (tests/test_train_gpu.py, whose batch recipe, ``classif*`` down-scaling and loss are used)."""
import pytest
import torch

from tests.helpers import maxerr

pytestmark = pytest.mark.gpu

DISP_TOL = 1e-3           # px; the bound of tests/test_models_gpu.py
FORMS = {"single-process": False, "flat-gradients": True}
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_graphs():
    yield
    _RUNS.clear()


def _batch(B, H, W, shift, seed):
    """tests/test_train_gpu.py's: a random left view, the right one rolled by ``shift``, constant disparity."""
    g = torch.Generator().manual_seed(seed)
    left = torch.rand(B, 3, H, W, generator=g)
    right = torch.roll(left, -shift, dims=3)
    disp = torch.full((B, 1, H, W), float(shift))
    disp[:, :, :, :shift] = 0
    return torch.cat([left, right, disp], 1).cuda()


def _eval(model, batch):
    model.eval()
    with torch.no_grad():
        return [d.detach().clone() for d in model(batch[:, :3], batch[:, 3:6])[1]]


def _worst(a, b):
    return max(maxerr(x, y) for x, y in zip(a, b))


def run(form, hip_lib):
    """Build the step; eval forward e1 (fills every fold cache); three replays; eval forward e2; a freshly built
    model with the same state_dict on the same input, e_fresh.  Once per form, shared by the tests below."""
    if form in _RUNS:
        return _RUNS[form]
    from dsmnet_amd import train
    from dsmnet_amd.graphs import GraphedTrainStep
    from dsmnet_amd.models import model_create_by_name
    torch.manual_seed(0)
    model = model_create_by_name("psmnet", 192).cuda()
    for i in (1, 2, 3):
        with torch.no_grad():
            getattr(model, "classif%d" % i)[2].weight.mul_(1e-3)
    lossfun = train.losses("supervised", 1, 0)
    lossfun.Weight_Adjust_levels(0)
    batches = [_batch(1, 256, 256, 6, s) for s in (5, 6, 7)]
    probe = _batch(1, 256, 256, 6, 9)
    optim = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    step = GraphedTrainStep(model, optim, lossfun, batches[0], warmup=1, flat_gradients=FORMS[form])
    e1 = _eval(model, probe)
    model.train()
    zero = {}
    if FORMS[form]:
        # the three replays double as the zero_grad sequence: step, model.zero_grad() at torch's default, step
        params = [p for p in model.parameters() if p.requires_grad]
        fg = step.flatgrads
        losses = [float(step(batches[0])[0])]
        zero["after_first"] = [p.detach().clone() for p in params]
        model.zero_grad()
        zero["unbound"] = all(p.grad is None for p in params)
        losses.append(float(step(batches[1])[0]))
        zero["had_gt"] = float(fg.extra)
        zero["after_second"] = [p.detach().clone() for p in params]
        offsets, off = [], 0
        for p in params:
            offsets.append(p.grad is not None and p.grad.data_ptr() == fg.flat.data_ptr() + 4 * off)
            off += p.numel()
        zero["rebound"] = all(offsets) and off == fg.total
        zero["grad_max"] = fg.flat[:fg.total].abs().max().item()
        losses.append(float(step(batches[2])[0]))
    else:
        losses = [float(step(b)[0]) for b in batches]
    e2 = _eval(model, probe)
    fresh = model_create_by_name("psmnet", 192)
    fresh.load_state_dict(model.state_dict())
    e_fresh = _eval(fresh.cuda(), probe)
    del fresh
    _RUNS[form] = dict(model=model, optim=optim, step=step, batches=batches, probe=probe, losses=losses,
                       e1=e1, e2=e2, e_fresh=e_fresh, zero=zero)
    return _RUNS[form]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_eval_after_replays_equals_a_freshly_built_model(hip_lib, form):
    """eval, three graphed steps, eval: the second eval forward equals a fresh model's with the same
    ``state_dict`` within ``DISP_TOL`` (same kernels on the same weights: in fact far tighter, printed), and
    the three steps moved the output by more than ten times that -- else the comparison would say nothing.

    Without the invalidation in ``GraphedTrainStep.__call__`` the single-process form serves the folds e1
    made, so e2 is e1 and |e2 - e_fresh| is |e1 - e_fresh| ("state that outlives a
    launch"); in the flat-gradient form the eager optimizer step bumps every weight's version, and since
    every fold holds a weight that hides the stale running statistics.  All three differences are printed."""
    r = run(form, hip_lib)
    moved, stale, frozen = _worst(r["e_fresh"], r["e1"]), _worst(r["e2"], r["e_fresh"]), _worst(r["e2"], r["e1"])
    print("%s: losses %s; |e_fresh - e1| = %.3e px, |e2 - e_fresh| = %.3e px, |e2 - e1| = %.3e px"
          % (form, ["%.4f" % l for l in r["losses"]], moved, stale, frozen))
    assert all(torch.isfinite(d).all() for d in r["e2"] + r["e_fresh"])
    assert moved > 10 * DISP_TOL, moved                # a condition on the inputs: training moved the output
    assert stale <= DISP_TOL, (stale, frozen)


def test_flat_gradients_survive_zero_grad_between_graphed_steps(hip_lib):
    """step, ``model.zero_grad()`` at torch's default, step -- the first two of the three replays above, on the
    same model: the second step changes the parameters (before the views were re-attached Adam skipped every
    parameter: a change of exactly zero), and every ``p.grad`` is again a view of ``flatgrads.flat`` at its own
    offset, holding the gradients the captured backward wrote."""
    z = run("flat-gradients", hip_lib)["zero"]
    assert z["unbound"]                                # zero_grad() did set every gradient to None
    assert z["had_gt"] == 1.0                          # the batch had ground truth: the step was due
    second = sum((a - b).abs().sum().item() for a, b in zip(z["after_first"], z["after_second"]))
    changed = sum(1 for a, b in zip(z["after_first"], z["after_second"]) if not torch.equal(a, b))
    print("second step: sum |delta parameters| %.4e over %d of %d tensors; max |gradient| %.3e"
          % (second, changed, len(z["after_first"]), z["grad_max"]))
    assert all(torch.isfinite(t).all() for t in z["after_second"])
    assert second > 0.0 and changed > 0, (second, changed)
    assert z["rebound"] and z["grad_max"] > 0
