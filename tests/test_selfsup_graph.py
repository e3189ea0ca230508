"""CPU: the host side of the captured self-supervised step -- the C ABI of the device-array form of
the fused loss (dsm_selfsup_dyn_*: symbols and argument checks, no kernel is launched), the layout
of the array, the order of the host's random draws, the tensor learning rate, and the step on two
ranks over gloo."""
import ctypes
import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dsmnet_amd import sharding
from tests.test_sharding import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_signatures_and_library_agree(hip_lib):
    from dsmnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "dsmnet_hip.h")).read()
    declared = set(re.findall(r"\b(dsm_\w+)\s*\(", header))
    for name in ("dsm_selfsup_dyn_fwd", "dsm_selfsup_dyn_bwd"):
        assert name in declared
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == 9        # items, ext, n, flags, params + 4 pointers
        assert getattr(hip_lib, name) is not None         # exported by the built library
    assert hip_lib.dsm_abi_version() == 7


def _items(n=2):
    from dsmnet_amd import _lib
    items = (_lib.SelfsupItem * n)()
    for it in items:
        it.im = it.src = it.disp = it.disp_other = it.grad_disp = it.grad_other = 16
        it.B, it.h, it.w, it.H0, it.W0, it.scale_factor = 1, 20, 30, 20, 30, 1
    return items


def test_abi_argument_checks(hip_lib):
    """Every refusal comes back as a code before anything is launched (the pointers are dummies)."""
    from dsmnet_amd import _lib
    assert ctypes.sizeof(_lib.SelfsupItem) == 128
    items = _items()
    ws = ctypes.c_void_p(16)
    bad = ctypes.c_void_p(20)                              # 4-byte, not 16-byte aligned
    sss = _lib.DSM_SELFSUP_SSSMNET | _lib.DSM_SELFSUP_MASK
    for fn in (hip_lib.dsm_selfsup_dyn_fwd, hip_lib.dsm_selfsup_dyn_bwd):
        for flags in (0, _lib.DSM_SELFSUP_MASK, _lib.DSM_SELFSUP_CAP | _lib.DSM_SELFSUP_DS | _lib.DSM_SELFSUP_MASK,
                      _lib.DSM_SELFSUP_COMMON, sss):
            assert fn(items, None, 2, flags, None, ws, ws, ws, None) == -1     # no params
            assert fn(items, None, 2, flags, bad, ws, ws, ws, None) == -4      # misaligned params
            assert fn(items, None, 1, flags, ws, ws, ws, ws, None) == -1       # odd item count
            assert fn(items, None, 2, flags, ws, None, ws, ws, None) == -1     # no workspace
            assert fn(None, None, 2, flags, ws, ws, ws, ws, None) == -1        # no items
        assert fn(items, None, 2, sss, ws, ws, ws, ws, None) == -1             # SsSMnet without ext
        assert fn(items, None, 2, 64, ws, ws, ws, ws, None) == -1              # no such objective
        items[1].w = 31
        assert fn(items, None, 2, 0, ws, ws, ws, ws, None) == -1               # the views differ
        items[1].w = 30
    items[0].grad_disp = None
    assert hip_lib.dsm_selfsup_dyn_bwd(items, None, 2, 0, ws, ws, ws, ws, None) == -1   # no gradient buffer


# (name, flag_mask, two entries of distinct epsilons, the 2n x 4 table written out by hand)
E = [(0.01, 0.02, 0.03, 0.04, 0.05, 0.06), (0.11, 0.12, 0.13, 0.14, 0.15, 0.16)]
W = [0.25, 0.75]
TABLES = [
    ("depthmono", True, 4, [[0.01, 0.03, 0.0, 0.25], [0.02, 0.04, 0.0, 0.25],
                            [0.11, 0.13, 0.0, 0.75], [0.12, 0.14, 0.0, 0.75]]),
    ("cap", False, 4, [[0.01, 0.03, 0.0, 0.25], [0.02, 0.04, 0.0, 0.25],
                       [0.11, 0.13, 0.0, 0.75], [0.12, 0.14, 0.0, 0.75]]),
    ("common", False, 4, [[0.01, 0.03, 0.0, 0.25], [0.02, 0.04, 0.0, 0.25],
                          [0.11, 0.13, 0.0, 0.75], [0.12, 0.14, 0.0, 0.75]]),
    # SsSMnet: imL_wrap, imL1_wrap, imL_wrap1, imL1_wrap1 -- no disparity epsilon without -mask
    ("sssmnet", False, 4, [[0.01, 0.0, 0.03, 0.25], [0.02, 0.0, 0.04, 0.25],
                           [0.11, 0.0, 0.13, 0.75], [0.12, 0.0, 0.14, 0.75]]),
    # ... and dispL_wrap, dispL1_wrap after them with it
    ("sssmnet", True, 6, [[0.01, 0.05, 0.03, 0.25], [0.02, 0.06, 0.04, 0.25],
                          [0.11, 0.15, 0.13, 0.75], [0.12, 0.16, 0.14, 0.75]]),
]


@pytest.mark.parametrize("objective,mask,count,table", TABLES)
def test_step_params_layout(objective, mask, count, table):
    from dsmnet_amd import costvolume as cv
    delts = [e[:count] for e in E]
    got = cv.selfsup_step_params(delts, W, objective, mask)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, 4) and got.device.type == "cpu"
    want = torch.tensor(table, dtype=torch.float32)
    assert torch.equal(got, want), (got, want)
    out = torch.full((4, 4), -1.0)
    assert cv.selfsup_step_params(delts, W, objective, mask, out=out) is out and torch.equal(out, want)
    with pytest.raises(ValueError):
        cv.selfsup_step_params([e[:count - 1] for e in E], W, objective, mask)
    with pytest.raises(ValueError):
        cv.selfsup_step_params(delts, W[:1], objective, mask)
    # the items and the side array take their scalars through the same mapping
    spec = {"levels": [0, 0], "factors": [1, 1], "weights": W, "delts": delts, "lefttop": (0, 0), "lefttop1": (0, 0),
            "flag_mask": mask, "objective": objective, "terms": ("ds", "lr"), "ds_divisors": [1, 1], "params": None}
    im = torch.zeros(1, 3, 4, 6)
    d = [torch.zeros(1, 1, 4, 6)] * 4
    items = cv.SelfsupPyramidLossFunction._items(spec, (im, im, im, im), d)
    ext = cv.SelfsupPyramidLossFunction._ext(spec, d, torch.zeros(4 * 72))
    for i in range(4):
        row = [items[i].delt_im, items[i].delt_disp, ext[i].delt_im1 if objective == "sssmnet" else 0.0,
               items[i].weight]
        assert row == want[i].tolist(), (i, row)


def _lossfun(name, levels, maxepoch):
    from dsmnet_amd import train
    return train.selfsup_losses(name, levels, maxepoch)


def _pyramid_args(n):
    """CPU stand-ins with DispNetC's level shapes: the op is replaced, nothing reads the values."""
    h, w = 64, 128
    ds = [torch.zeros(1, 1, -(-h // 2 ** k), -(-w // 2 ** k)) for k in range(n)]
    im = torch.zeros(1, 3, h, w)
    return {"imR_src": im, "imL": im, "dispLs": ds, "scale_dispLs": list(range(n)), "LeftTop": [0, 0],
            "imR1_src": im, "imL1": im, "dispL1s": list(ds), "scale_dispL1s": list(range(n)), "LeftTop1": [0, 0]}


@pytest.mark.parametrize("name", ["depthmono-mask", "Cap_ds-mask", "common", "SsSMnet", "SsSMnet-mask"])
@pytest.mark.parametrize("adjusted", [True, False])
def test_draw_step_params_draws_what_the_loss_call_draws(monkeypatch, name, adjusted):
    from dsmnet_amd import costvolume as cv
    seen = {}

    def record(*args, **kwargs):
        seen["weights"], seen["delts"], seen["levels"] = args[9], args[12], args[8]
        seen["params"], seen["objective"] = kwargs.get("params"), kwargs.get("objective", "depthmono")
        return torch.zeros(())
    monkeypatch.setattr(cv, "selfsup_pyramid_loss", record)
    lf = _lossfun(name, 7, 10)
    if adjusted:
        lf.Weight_Adjust_levels(3)                         # every level has a weight
    args = _pyramid_args(7)
    assert lf.entered_levels(args["scale_dispLs"]) == (tuple(range(7)) if adjusted else (6,))
    torch.manual_seed(77)
    lf(args)
    after_call = torch.get_rng_state()
    count = 6 if name == "SsSMnet-mask" else 4
    assert len(seen["delts"]) == (7 if adjusted else 1) and all(len(d) == count for d in seen["delts"])
    want = cv.selfsup_step_params(seen["delts"], seen["weights"], seen["objective"], lf.flag_mask)
    torch.manual_seed(77)
    got = lf.draw_step_params(args["scale_dispLs"])
    assert torch.equal(torch.get_rng_state(), after_call)   # the same number of draws
    assert torch.equal(got, want)
    assert len(set(got[:, 0].tolist())) == got.shape[0]     # really random: all different
    # with the array set, the loss call draws nothing and hands the array on in place of both lists
    lf.step_params = got
    lf(args)
    assert torch.equal(torch.get_rng_state(), after_call)
    assert seen["params"] is got and seen["weights"] is None and seen["delts"] is None
    assert len(seen["levels"]) == got.shape[0] // 2


def test_supervised_loss_has_no_step_params():
    from dsmnet_amd import train
    lf = train.losses("supervised", 2, 4)
    assert lf.step_params is None
    with pytest.raises(ValueError):
        lf.draw_step_params([0, 1])


def test_lr_adjust_keeps_a_tensor_learning_rate():
    from dsmnet_amd import train
    model = torch.nn.Linear(3, 2)
    opt = train.make_optimizer(model, lr=1e-3, capturable=True)
    lr = opt.param_groups[0]["lr"]
    assert torch.is_tensor(lr) and lr.dim() == 0 and opt.param_groups[0]["capturable"]
    train.lr_adjust(opt, 10, 5, 1e-3, 9)                   # before epoch0: untouched
    assert opt.param_groups[0]["lr"] is lr and float(lr) == pytest.approx(1e-3)
    for epoch, halvings in ((10, 1), (14, 1), (15, 2), (27, 4)):
        train.lr_adjust(opt, 10, 5, 1e-3, epoch)
        assert opt.param_groups[0]["lr"] is lr             # the tensor a captured step reads
        assert float(lr) == pytest.approx(1e-3 * 0.5 ** halvings, rel=1e-6)
    plain = train.make_optimizer(model, lr=1e-3)
    assert isinstance(plain.param_groups[0]["lr"], float) and not plain.param_groups[0].get("capturable")
    train.lr_adjust(plain, 10, 5, 1e-3, 15)
    assert isinstance(plain.param_groups[0]["lr"], float) and plain.param_groups[0]["lr"] == 1e-3 * 0.25


class _ToyStereo(torch.nn.Module):
    def __init__(self):
        super(_ToyStereo, self).__init__()
        self.count_levels = 2
        self.conv = torch.nn.Conv2d(6, 1, 3, padding=1)

    def forward(self, imL, imR, mode="train"):
        d0 = self.conv(torch.cat([imL, imR], 1))
        return [0, 1], [d0, torch.nn.functional.avg_pool2d(d0, 2)]


class _ToyLoss(object):
    """A differentiable stand-in with the self-supervised argument dict."""
    flag_mask = False

    def __call__(self, a):
        loss = 0
        for d, d1 in zip(a["dispLs"], a["dispL1s"]):
            loss = loss + (d - a["imL"][:, :1, ::a["imL"].shape[2] // d.shape[2], ::a["imL"].shape[3] // d.shape[3]]).abs().mean()
            loss = loss + 0.5 * (d1 ** 2).mean()
        return loss


def _batch(seed):
    return torch.rand(2, 6, 8, 12, generator=torch.Generator().manual_seed(seed))


def _ranks_worker(rank, world, port, q):
    from dsmnet_amd import train
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sharding.init_from_env("gloo")
    torch.manual_seed(0)
    model = _ToyStereo()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    out = train.train_step_selfsup_ranks(model, opt, _ToyLoss(), _batch(100 + rank))   # world from the group
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, out, [p.detach().numpy().copy() for p in model.parameters()]))


def _own(model, batch):
    from dsmnet_amd import train
    loss, _ = train._selfsup_forward(model, _ToyLoss(), batch, 0, None)
    return loss


def test_train_step_selfsup_ranks_world_size_2_equals_averaged_gradients():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ranks_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {r: (out, params) for r, out, params in (q.get(timeout=120) for _ in procs)}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    torch.manual_seed(0)
    model = _ToyStereo()
    grads, own = [], []
    for r in range(2):
        model.zero_grad()
        loss = _own(model, _batch(100 + r))
        loss.backward()
        own.append(float(loss.detach()))
        grads.append([p.grad.clone() for p in model.parameters()])
    assert not torch.allclose(grads[0][0], grads[1][0])           # the ranks really differ
    want = [p.detach() - 0.1 * (g0 + g1) / 2 for p, g0, g1 in zip(model.parameters(), *grads)]
    for r in (0, 1):
        assert results[r][0] == (pytest.approx(own[r], rel=1e-6), -1.0, -1.0)   # the rank's own loss
        for got, w in zip(results[r][1], want):
            assert torch.allclose(torch.from_numpy(got), w, atol=1e-6)


def test_train_step_selfsup_ranks_on_one_rank_is_train_step_selfsup():
    from dsmnet_amd import train
    outs, params = [], []
    for step in (train.train_step_selfsup, train.train_step_selfsup_ranks):
        torch.manual_seed(0)
        model = _ToyStereo()
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        outs.append(step(model, opt, _ToyLoss(), _batch(5), world=1))
        params.append([p.detach().clone() for p in model.parameters()])
    assert outs[0] == outs[1]
    assert all(torch.equal(a, b) for a, b in zip(*params))
