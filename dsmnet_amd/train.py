"""Training steps with the reference's objectives and bookkeeping:
``losses`` (losses/loss.py:341-392,407-422,515-516 -- ``loss_supervised`` :326-338),
``lr_adjust`` (stereo.py:95-101), ``accuracy`` (stereo.py:103-113), ``AverageMeter``
(utils/utils.py:87-118) and the body of the reference's train / validate loops
(stereo_supervised.py:43-119, 121-190) as ``train_step`` / ``validate_step``.

The self-supervised ``depthmono-mask`` objective (loss.py:196-236, 393-405, 424-467; the
preset of DSMnet_train_kitti-raw.sh) runs as ONE fused HIP op over the whole pyramid
(``costvolume.selfsup_pyramid_loss``, csrc/selfsup.hip); ``train_step_selfsup`` /
``validate_step_selfsup`` are stereo_selfsupervised.py:48-118 / 148-200.  The ``Cap`` objectives
without a left-right term -- ``Cap``, ``Cap_ds``, ``Cap-mask`` and ``Cap_ds-mask``, the preset of
DSMnet_train_kitti.sh (loss.py:238-283 ``loss_Cap_ds_lr``) -- run through the same op with its
Cap rule: no "< 1024 valid pixels" fallback, the smoothness weight divided by 2**level of the
output's own level, terms chosen by the name; their backward is one gather launch and
bit-reproducible.  ``losses`` refuses ``common``, ``SsSMnet``, every Cap name with ``lr``
(``Cap_ds_lr``, ...) and plain ``depthmono`` (no ``-mask``): existing tests pin that gate.
``selfsup_losses``, its subclass, takes them all: ``common[-mask]`` (loss.py:154-194, depthmono's
rule with the depth-ratio smoothness C_ds3) is the op's ``objective="common"``, ``SsSMnet[-mask]``
(loss.py:285-324 through ``losses_pyramid2``, the warp of a warp) its ``objective="sssmnet"``; the
Cap names with ``lr`` and plain ``depthmono`` were always in the op.

A captured step (``graphs.GraphedSelfsupStep``) must not freeze what the reference changes from
step to step: ``losses.draw_step_params`` makes a loss call's random draws ahead of it, and with
``losses.step_params`` set the fused op reads epsilons and level weights from that device array
when its kernels run.  ``train_step_selfsup_ranks`` is ``train_step_selfsup`` for any world size.

The forward and backward of the model run on the HIP kernels (``costvolume`` autograd
functions).  The supervised objective over the whole pyramid of outputs, together with the D1 /
EPE of the first output, is ONE fused HIP op as well (``costvolume.supervised_pyramid_loss``,
csrc/suploss.hip: two launches forward, one backward, no host read in the capturable form) when
the maps are CUDA float32, the shapes are supported and the option ``fused_supervised_loss`` is
on (the default; DSM_FUSED_SUP_LOSS=0 turns it off); otherwise -- CPU tensors among them -- it is
the stock torch restatement below, unchanged.
"""
import weakref

import torch
import torch.nn.functional as F

from . import sharding


def _diff1_dx(img):
    return F.pad(img[:, :, :, 1:] - img[:, :, :, :-1], [0, 1, 0, 0])


def _diff1_dy(img):
    return F.pad(img[:, :, 1:] - img[:, :, :-1], [0, 0, 0, 1])


class losses(torch.nn.Module):
    """``losses(loss_name="supervised", count_levels, maxepoch_weight_adjust)``; call with the
    reference's argument dict ``{"disp_gt", "disps", "scale_disps", "flag_smooth"}``."""

    def __init__(self, loss_name="supervised", count_levels=1, maxepoch_weight_adjust=1):
        super(losses, self).__init__()
        name = loss_name.split("-")[0].lower()
        self.flag_mask = "mask" in loss_name
        if "supervised" in name:                     # setlossfun, loss.py:367-377
            self.lossfun = self.loss_supervised
            self.lossesfun = self.losses_pyramid0
        elif "depthmono" in name and self.flag_mask:
            # the preset of DSMnet_train_kitti-raw.sh; plain "depthmono" stays unbuilt (its
            # NotImplementedError is pinned by tests/test_train.py), the fused op takes both
            self.lossfun = self.loss_depthmono
            self.lossesfun = self.losses_pyramid1
        elif "cap" in name and "lr" not in name and "depthmono" not in name and "sssmnet" not in name:
            # loss.py:372-374, terms by the name (:270, :275).  The names with a left-right term stay
            # unbuilt at this level (Cap_ds_lr's NotImplementedError is pinned by
            # tests/test_selfsup.py); the fused op takes the term
            self.lossfun = self.loss_Cap_ds_lr
            self.lossesfun = self.losses_pyramid1
            self.cap_terms = ("ds",) if "ds" in name else ()
        else:
            raise NotImplementedError(
                "loss_name=%r is not built: supervised, depthmono-mask and Cap / Cap_ds / Cap-mask / "
                "Cap_ds-mask are; common (C_ds3), SsSMnet, depthmono without -mask and every Cap name "
                "with a left-right term (Cap_ds_lr, Cap_lr, ...) are not" % loss_name)
        self.maxepoch_weight_adjust = maxepoch_weight_adjust
        self.count_levels = count_levels
        self.weight_levels = [0] * count_levels
        self.weight_levels[-1] = 1
        # capturable = True: no host-side test for "no valid pixel" (a device synchronisation);
        # the loss is then a zero tensor instead of the reference's integer 0 -- what a hipGraph
        # capture of the whole step needs (graphs.GraphedTrainStep sets it)
        self.capturable = False
        self.last_metrics = None
        # a (2n, 4) device tensor (``costvolume.selfsup_step_params``' layout, e.g. a copy of
        # ``draw_step_params``' result): the self-supervised pyramid then draws nothing and hands the
        # fused op this array, which its kernels read when they run -- what lets a captured step
        # replay with every step's own epsilons and level weights (graphs.GraphedSelfsupStep)
        self.step_params = None

    def Weight_Adjust_levels(self, epoch):
        """Coarse-to-fine: the unit weight slides from the coarsest output (epoch 0) to the
        finest (``maxepoch_weight_adjust``); every other level keeps 0.01."""
        n, maxepoch = self.count_levels, self.maxepoch_weight_adjust
        self.weight_levels = [0.01] * n
        if n == 1 or epoch >= maxepoch:
            self.weight_levels[0] = 1
            return
        x = (1 - epoch / float(maxepoch)) * (n - 1)
        idx = int(x)
        w = x - idx
        self.weight_levels[idx] = 1 - w
        if idx < n - 1:
            self.weight_levels[idx + 1] = w

    def loss_supervised(self, disp_gt, disp, flag_smooth=False, factor=1.0):
        mask = disp_gt > 0
        if self.capturable:                     # same value, fixed shapes, no synchronisation
            m = mask.to(disp.dtype)
            n = m.sum().clamp_min(1.0)
            loss = (torch.abs(disp_gt - disp) * m).sum() / n
            if flag_smooth:
                dxdy = (torch.abs(_diff1_dx(disp)) + torch.abs(_diff1_dy(disp))) / factor
                loss = loss + 0.1 * (dxdy.clamp(0, 1) * m).sum() / n
            return loss
        if not bool(mask.any()):
            return 0
        loss = torch.abs(disp_gt - disp)[mask].mean()
        if flag_smooth:
            dxdy = (torch.abs(_diff1_dx(disp)) + torch.abs(_diff1_dy(disp))) / factor
            loss = loss + 0.1 * dxdy[mask].clamp(0, 1).mean()
        return loss

    def _fused_pyramid0(self, disp_gt, disps, scale_disps, flag_smooth):
        """The weighted outputs through ``costvolume.supervised_pyramid_loss``; ``NotImplemented``
        when the stock path has to run (CPU or non-fp32 maps, option off, unsupported shapes)."""
        if not (torch.is_tensor(disp_gt) and disp_gt.is_cuda and self.lossfun == self.loss_supervised):
            return NotImplemented
        from . import costvolume as cv
        if not cv.get_option("fused_supervised_loss"):
            return NotImplemented
        picked = [(i, level) for i, level in enumerate(scale_disps) if self.weight_levels[level] > 0]
        preds = [disps[i] for i, _ in picked]
        levels = [level for _, level in picked]
        if not preds or not cv.supervised_loss_supported(disp_gt, preds, levels):
            return NotImplemented
        # a level-0 output is used as it is (no crop): it has to be gt's size, as in the stock form
        if any(level == 0 and p.shape[-2:] != disp_gt.shape[-2:] for p, level in zip(preds, levels)):
            return NotImplemented
        loss, aux = cv.supervised_pyramid_loss(disp_gt, preds, levels,
                                               [self.weight_levels[level] for level in levels], flag_smooth)
        if picked[0] == (0, 0):
            # D1 / EPE of the first output ride along.  A weak reference: holding the output itself
            # would keep this step's whole autograd graph alive until the next call, across a
            # later hipGraph capture on the same model (graphs.GraphedTrainStep._quiesce)
            self.last_metrics = (weakref.ref(disps[0]), aux[4], aux[3])
        if not self.capturable and float(aux[0]) == 0:      # the step's one host read
            return 0
        return loss

    def losses_pyramid0(self, disp_gt, disps, scale_disps, flag_smooth=False):
        self.last_metrics = None                # (weak ref to the first output, D1, EPE) of the latest fused call
        fused = self._fused_pyramid0(disp_gt, disps, scale_disps, flag_smooth)
        if fused is not NotImplemented:
            return fused
        _, _, h, w = disp_gt.shape
        loss = 0
        for pred, level in zip(disps, scale_disps):
            weight = self.weight_levels[level]
            if weight <= 0:
                continue
            if pred.dim() == 3:          # PSMNet returns (B,H,W); the reference's diff1_dx asserts 4-D
                pred = pred.unsqueeze(1)
            if level > 0:
                pred = F.interpolate(pred, scale_factor=2 ** level, mode="bilinear",
                                     align_corners=False)[:, :, :h, :w]
            loss = loss + self.lossfun(disp_gt, pred, flag_smooth, factor=1) * weight
        return loss

    def loss_depthmono(self, imL, imR_src, LeftTop, dispL, imL1, imR1_src, LeftTop1, dispL1,
                       level=0, scale_factor=1, weight=1.0, delts=None):
        """loss.py:196-236 for ONE pyramid entry, both views (the reference calls it once per view
        with the warps precomputed): weight * (C(left view) + C(flipped view)) through the fused
        op.  ``imL``/``imL1`` are the level-0 crops; ``level`` picks imL[:, :, ::2**level, ::2**level]."""
        from . import costvolume as cv
        if delts is None:
            delts = tuple(_draw_delt() for _ in range(4))
        return cv.selfsup_pyramid_loss(imL, imR_src, LeftTop, [dispL], imL1, imR1_src, LeftTop1,
                                       [dispL1], [level], [weight], [scale_factor], self.flag_mask,
                                       [delts])

    def loss_Cap_ds_lr(self, imL, imR_src, LeftTop, dispL, imL1, imR1_src, LeftTop1, dispL1,
                       level=0, scale_factor=1, weight=1.0, delts=None, factor=1):
        """loss.py:238-283 for ONE pyramid entry, both views, as ``loss_depthmono`` above; ``factor``
        divides the smoothness weight (the reference passes 2**level of the output's level)."""
        from . import costvolume as cv
        if delts is None:
            delts = tuple(_draw_delt() for _ in range(4))
        return cv.selfsup_pyramid_loss(imL, imR_src, LeftTop, [dispL], imL1, imR1_src, LeftTop1,
                                       [dispL1], [level], [weight], [scale_factor], self.flag_mask,
                                       [delts], objective="cap", terms=self.cap_terms, ds_divisors=[factor])

    def _draw_rule(self):
        """(objective of the fused op, epsilons per weighted level, the rule that leaves a level out)
        of this loss: losses_pyramid1 skips ``weight <= 0`` (loss.py:436) and draws four,
        losses_pyramid2 skips ``weight == 0`` (:482) and draws four, six with ``-mask``."""
        if self.lossesfun == getattr(self, "losses_pyramid2", None):
            return "sssmnet", 6 if self.flag_mask else 4, lambda weight: weight == 0
        if self.lossesfun != self.losses_pyramid1:
            raise ValueError("not a self-supervised loss")
        return self._objective_kwargs(None).get("objective", "depthmono"), 4, lambda weight: weight <= 0

    def entered_levels(self, scale_dispLs):
        """Indices into ``scale_dispLs`` of the outputs the pyramid loss enters with the current
        ``weight_levels``: a host decision, and the shape of a captured step."""
        _, _, skip = self._draw_rule()
        return tuple(i for i, level in enumerate(scale_dispLs) if not skip(self.weight_levels[level]))

    def draw_step_params(self, scale_dispLs, out=None):
        """The epsilons of every entered level, drawn from the CPU generator in the reference's order
        and count -- the very calls an ordinary loss call makes -- with the current ``weight_levels``,
        as ``costvolume.selfsup_step_params``' (2n, 4) float32 CPU tensor (``out``: filled when
        given).  Under one seed, this followed by a loss call with ``step_params`` set uses the floats
        an ordinary loss call would have drawn."""
        from . import costvolume as cv
        objective, n_delts, _ = self._draw_rule()
        entered = self.entered_levels(scale_dispLs)
        if not entered:
            raise ValueError("draw_step_params: no level of %r has a weight" % (list(scale_dispLs),))
        weights = [self.weight_levels[scale_dispLs[i]] for i in entered]
        delts = [tuple(_draw_delt() for _ in range(n_delts)) for _ in entered]
        return cv.selfsup_step_params(delts, weights, objective, self.flag_mask, out=out)

    def _pyramid_entries(self, dispLs, dispL1s, scale_dispLs, n_delts=4, skip=lambda weight: weight <= 0):
        """The weighted entries of losses_pyramid1 / losses_pyramid2 (loss.py:426-446, 471-491) as the
        lists the fused op takes: levels above maxlevel = min(2, max level) are upsampled (stock
        autograd) to the maxlevel grid and compared with that image level; the ``n_delts`` random
        epsilons of every weighted level are drawn in the reference's order from torch's CPU
        generator.  ``divisors``: 2**level of the output's OWN level (loss.py:456, 503)."""
        dispLs = [d.unsqueeze(1) if d.dim() == 3 else d for d in dispLs]      # PSMNet: (B,H,W)
        dispL1s = [d.unsqueeze(1) if d.dim() == 3 else d for d in dispL1s]
        maxlevel = min(2, max(scale_dispLs))
        h = w = None
        if maxlevel in scale_dispLs:
            _, _, h, w = dispLs[maxlevel].shape
        ds, ds1, levels, weights, factors, delts, divisors = [], [], [], [], [], [], []
        for i, level in enumerate(scale_dispLs):
            weight = self.weight_levels[level]
            if skip(weight):
                continue
            if level > maxlevel:
                s = 2 ** (level - maxlevel)
                dL = F.interpolate(dispLs[i], scale_factor=s, mode="bilinear", align_corners=False)[:, :, :h, :w]
                dL1 = F.interpolate(dispL1s[i], scale_factor=s, mode="bilinear", align_corners=False)[:, :, :h, :w]
                factors.append(2 ** maxlevel)
            else:
                dL, dL1 = dispLs[i], dispL1s[i]
                factors.append(2 ** level)
            ds.append(dL)
            ds1.append(dL1)
            levels.append(min(level, maxlevel))
            weights.append(weight)
            divisors.append(2 ** level)
            if self.step_params is None:         # else ``draw_step_params`` drew them already
                delts.append(tuple(_draw_delt() for _ in range(n_delts)))
        if self.step_params is not None:        # weights and epsilons are in the device array
            weights = delts = None
        return ds, ds1, levels, weights, factors, delts, divisors

    def _step_kwargs(self):
        """The keyword that hands the fused op the device array (none without one: the call is the
        one it always was)."""
        return {} if self.step_params is None else {"params": self.step_params}

    def _objective_kwargs(self, divisors):
        """The keywords that name the objective to the fused op (none: depthmono)."""
        if self.lossfun == self.loss_Cap_ds_lr:
            return {"objective": "cap", "terms": self.cap_terms, "ds_divisors": divisors}
        return {}

    def losses_pyramid1(self, imR_src, imL, dispLs, scale_dispLs, LeftTop, imR1_src, imL1, dispL1s,
                        scale_dispL1s=None, LeftTop1=(0, 0)):
        """loss.py:424-467: the four random epsilons of every weighted level are drawn in the
        reference's order -- imL_wrap, imL1_wrap, dispL_wrap, dispL1_wrap -- (all four, also where
        the objective does not use a warp: the reference draws inside imwrap_BCHW, which it calls
        four times regardless); then ONE fused launch sequence for the whole pyramid.  The Cap
        objectives also get 2**level of the output's OWN level (loss.py:456), not the clamped one,
        as the divisor of their smoothness weight."""
        from . import costvolume as cv
        ds, ds1, levels, weights, factors, delts, divisors = self._pyramid_entries(dispLs, dispL1s, scale_dispLs)
        if not ds:
            return 0
        return cv.selfsup_pyramid_loss(imL, imR_src, LeftTop, ds, imL1, imR1_src, LeftTop1, ds1,
                                       levels, weights, factors, self.flag_mask, delts,
                                       **self._step_kwargs(), **self._objective_kwargs(divisors))

    def forward(self, args):
        return self.lossesfun(**args)


class selfsup_losses(losses):
    """Every self-supervised name of the reference's ``losses`` (loss.py:345-348) on the fused op,
    dispatched in ``setlossfun``'s order (:362-377): ``depthmono[-mask]``, ``SsSMnet[-mask]``, every
    ``Cap`` name -- those with a left-right term too -- and ``common[-mask]``.  ``losses`` itself
    keeps refusing the names it always refused (existing tests pin its gate; opening it is a
    one-line change for whoever may edit them); for the names it builds, this class makes the same
    calls and gives the same bits.  ``supervised`` belongs to ``losses``."""

    def __init__(self, loss_name="depthmono-mask", count_levels=1, maxepoch_weight_adjust=1):
        name = loss_name.split("-")[0].lower()
        if not (name in ("supervised", "depthmono", "sssmnet", "cap_ds_lr", "common") or "cap" in name):
            raise ValueError("loss_name=%r is none of the reference's (loss.py:347-348)" % loss_name)
        if "supervised" in name:                     # setlossfun's first branch
            raise ValueError("loss_name=%r is not self-supervised: use train.losses" % loss_name)
        # the parent's constructor for the level weights and the bookkeeping, under a name that passes
        # its gate; what the name selects is set below
        super(selfsup_losses, self).__init__("depthmono-mask", count_levels, maxepoch_weight_adjust)
        self.flag_mask = "mask" in loss_name
        if "depthmono" in name:                      # loss.py:366-377, in that order
            self.lossfun, self.lossesfun = self.loss_depthmono, self.losses_pyramid1
        elif "sssmnet" in name:
            self.lossfun, self.lossesfun = self.loss_SsSMnet, self.losses_pyramid2
        elif "cap" in name:
            self.lossfun, self.lossesfun = self.loss_Cap_ds_lr, self.losses_pyramid1
            self.cap_terms = tuple(t for t in ("ds", "lr") if t in name)          # loss.py:270, 275
        else:                                        # "common": the only name left after the check above
            self.lossfun, self.lossesfun = self.loss_common, self.losses_pyramid1

    def _objective_kwargs(self, divisors):
        if self.lossfun == self.loss_common:
            return {"objective": "common"}
        return super(selfsup_losses, self)._objective_kwargs(divisors)

    def loss_common(self, imL, imR_src, LeftTop, dispL, imL1, imR1_src, LeftTop1, dispL1,
                    level=0, scale_factor=1, weight=1.0, delts=None):
        """loss.py:154-194 for ONE pyramid entry, both views, as ``loss_depthmono``."""
        from . import costvolume as cv
        if delts is None:
            delts = tuple(_draw_delt() for _ in range(4))
        return cv.selfsup_pyramid_loss(imL, imR_src, LeftTop, [dispL], imL1, imR1_src, LeftTop1,
                                       [dispL1], [level], [weight], [scale_factor], self.flag_mask,
                                       [delts], objective="common")

    def loss_SsSMnet(self, imL, imR_src, LeftTop, dispL, imL1, imR1_src, LeftTop1, dispL1,
                     level=0, scale_factor=1, weight=1.0, delts=None, factor=1):
        """loss.py:285-324 for ONE pyramid entry, both views, as ``loss_Cap_ds_lr``: ``factor``
        divides the smoothness weight.  Four epsilons, six with ``-mask``."""
        from . import costvolume as cv
        if delts is None:
            delts = tuple(_draw_delt() for _ in range(6 if self.flag_mask else 4))
        return cv.selfsup_pyramid_loss(imL, imR_src, LeftTop, [dispL], imL1, imR1_src, LeftTop1,
                                       [dispL1], [level], [weight], [scale_factor], self.flag_mask,
                                       [delts], objective="sssmnet", ds_divisors=[factor])

    def losses_pyramid2(self, imR_src, imL, dispLs, scale_dispLs, LeftTop, imR1_src, imL1, dispL1s,
                        scale_dispL1s=None, LeftTop1=(0, 0)):
        """loss.py:469-512: as ``losses_pyramid1`` with the epsilons of the reference's warps in ITS
        order -- imL_wrap, imL1_wrap, imL_wrap1, imL1_wrap1 and, with ``-mask`` only, dispL_wrap,
        dispL1_wrap -- and with its skip rule (a level is left out when its weight is 0, :482)."""
        from . import costvolume as cv
        ds, ds1, levels, weights, factors, delts, divisors = self._pyramid_entries(
            dispLs, dispL1s, scale_dispLs, 6 if self.flag_mask else 4, lambda weight: weight == 0)
        if not ds:
            return 0
        return cv.selfsup_pyramid_loss(imL, imR_src, LeftTop, ds, imL1, imR1_src, LeftTop1, ds1,
                                       levels, weights, factors, self.flag_mask, delts,
                                       objective="sssmnet", ds_divisors=divisors, **self._step_kwargs())


def _draw_delt():
    """utils/imwrap.py:70: 1e-4 * (torch.rand(1)[0] + 0.1), in fp32, from the CPU generator (a host
    draw: no device synchronisation)."""
    return float(1e-4 * (torch.rand(1)[0] + 0.1))


def lr_adjust(optimizer, epoch0, stride, lr0, epoch):
    """Halve the learning rate every ``stride`` epochs from ``epoch0`` on (first halving at
    ``epoch0`` itself); untouched before."""
    if epoch < epoch0:
        return
    n = ((epoch - epoch0) // stride) + 1
    lr = lr0 * (0.5 ** n)
    for group in optimizer.param_groups:
        if torch.is_tensor(group["lr"]):        # a captured optimizer step reads this very tensor
            group["lr"].fill_(lr)
        else:
            group["lr"] = lr


def accuracy(dispL, dispL_gt):
    """(D1 %, EPE) over gt > 0.  Good pixel: error <= 3 px OR <= 5 % (the reference's OR)."""
    if dispL.dim() == 3:
        dispL = dispL.unsqueeze(1)
    mask = dispL_gt > 0
    diff = (dispL_gt - dispL).abs()[mask]
    epe = diff.mean()
    good = (diff <= 3) | ((diff / dispL_gt[mask]) <= 0.05)
    d1 = 100 - 100.0 * good.sum() / mask.sum()
    return d1, epe


class AverageMeter(object):
    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def make_optimizer(model, lr=1e-4, betas=(0.9, 0.999), capturable=False):
    """stereo.py:37-40 with main.py's defaults (:31-33).  ``capturable``: the form a captured step
    needs (graphs.GraphedTrainStep / GraphedSelfsupStep) -- fused Adam whose learning rate is a
    0-dim tensor on the parameters' device, which ``lr_adjust`` fills in place."""
    if not capturable:
        return torch.optim.Adam(model.parameters(), lr=lr, betas=betas)
    params = list(model.parameters())
    lr = torch.tensor(float(lr), dtype=torch.float32, device=params[0].device)
    return torch.optim.Adam(params, lr=lr, betas=betas, capturable=True, fused=True)


def _metrics(lossfun, disp0, disp_gt):
    """(D1, EPE) of the first output: what the fused loss of this very call computed along the way,
    else ``accuracy`` (two more passes over the maps)."""
    last = getattr(lossfun, "last_metrics", None)
    if last is not None and last[0]() is disp0:
        return last[1], last[2]
    return accuracy(disp0.detach(), disp_gt)


def _split(batch):
    if batch.shape[1] < 7:
        raise ValueError("a supervised batch is (B, >=7, H, W): imL | imR | dispL")
    return batch[:, :3], batch[:, 3:6], batch[:, 6:7]


def _world(world):
    import torch.distributed as dist
    if world is not None:
        return world
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def train_step(model, optim, lossfun, batch, world=None):
    """One iteration of stereo_supervised.py:53-97: forward in train mode, pyramid loss with
    ``flag_smooth=True``, backward, (multi-GPU: one flat gradient all-reduce), Adam step.
    ``batch`` = (B,7,H,W) imL | imR | dispL, as the reference's loader yields it.
    Returns (loss, D1, EPE) as floats.

    Single process: a batch without any ground-truth pixel gives the reference's integer-0 loss
    and the step is skipped, as there (losses/loss.py:330-331).  Several ranks: EVERY rank runs
    backward and the all-reduce every step (the loss is the tensor form, zero -- with zero
    gradients -- on a rank without ground truth), so the collective calls always match; the
    number of ranks that had ground truth rides in the same bucket and the optimizer step is
    skipped on all ranks together when it is zero."""
    from . import costvolume as cv
    with cv.amax_scope(batch.device):            # fp16 convolution modes: one arena of maxima per step
        return _train_step(model, optim, lossfun, batch, world)


def _train_step(model, optim, lossfun, batch, world):
    model.train()
    world = _world(world)
    imL, imR, dispL = _split(batch)
    scale_dispLs, dispLs = model(imL, imR)
    args = {"disp_gt": dispL, "disps": dispLs, "scale_disps": scale_dispLs, "flag_smooth": True}
    optim.zero_grad()
    if world > 1:
        was = lossfun.capturable
        lossfun.capturable = True               # tensor loss on every rank, no host-side branch
        try:
            loss = lossfun(args)
        finally:
            lossfun.capturable = was
        loss.backward()
        has_gt = (dispL > 0).any().to(torch.float32).reshape(1)
        _, n_gt = sharding.allreduce_gradients(model.parameters(), world=world, extra=has_gt)
        if float(n_gt) > 0:
            optim.step()
    else:
        loss = lossfun(args)
        if torch.is_tensor(loss):              # the integer 0 when no pixel has ground truth
            loss.backward()
            optim.step()
    d1, epe = _metrics(lossfun, dispLs[0], dispL)
    return float(loss.detach() if torch.is_tensor(loss) else loss), float(d1), float(epe)


def validate_step(model, lossfun, batch):
    """One iteration of stereo_supervised.py:129-162 (eval mode, no gradients)."""
    model.eval()
    imL, imR, dispL = _split(batch)
    with torch.no_grad():
        scale_dispLs, dispLs = model(imL, imR)
        loss = lossfun({"disp_gt": dispL, "disps": dispLs, "scale_disps": scale_dispLs,
                        "flag_smooth": True})
        d1, epe = _metrics(lossfun, dispLs[0], dispL)
    return float(loss), float(d1), float(epe)


def _selfsup_args(batch, nedge, augment):
    """stereo_selfsupervised.py:63-90: the flipped pair is the second view; the network sees the
    (augmented) nedge-cropped images, the loss warps the un-cropped right images from LeftTop."""
    bn, c, h, w = batch.shape
    if c < 6 or h <= 2 * nedge or w <= 2 * nedge:
        raise ValueError("a self-supervised batch is (B, >=6, H, W) with H, W > 2 * nedge = %d" % (2 * nedge))
    batch1 = torch.flip(batch, dims=[-1])
    batch_aug = batch[:, :6, nedge:h - nedge, nedge:w - nedge].clone()
    if augment is not None:
        batch_aug = augment(batch_aug)
    batch1_aug = torch.flip(batch_aug, dims=[-1])
    pre = (batch_aug[:, :3], batch_aug[:, 3:6], batch1_aug[:, 3:6], batch1_aug[:, :3])
    args = {"imR_src": batch[:, 3:6], "imL": batch[:, :3, nedge:h - nedge, nedge:w - nedge],
            "LeftTop": [nedge, nedge], "imR1_src": batch1[:, :3],
            "imL1": batch1[:, 3:6, nedge:h - nedge, nedge:w - nedge], "LeftTop1": [nedge, nedge]}
    return pre, args


def _selfsup_forward(model, lossfun, batch, nedge, augment):
    (imL_pre, imR_pre, imL1_pre, imR1_pre), args = _selfsup_args(batch, nedge, augment)
    scale_dispLs, dispLs = model(imL_pre, imR_pre)
    scale_dispL1s, dispL1s = model(imL1_pre, imR1_pre)
    args.update({"dispLs": dispLs, "scale_dispLs": scale_dispLs, "dispL1s": dispL1s,
                 "scale_dispL1s": scale_dispL1s})
    return lossfun(args), dispLs


def _selfsup_accuracy(batch, dispLs, nedge):
    if batch.shape[1] < 7:
        return -1.0, -1.0
    h, w = batch.shape[2:]
    d1, epe = accuracy(dispLs[0].detach(), batch[:, 6:7, nedge:h - nedge, nedge:w - nedge])
    return float(d1), float(epe)


def train_step_selfsup(model, optim, lossfun, batch, augment=None, world=None, nedge=None):
    """One iteration of stereo_selfsupervised.py:57-118: ``batch`` (B,>=6,H,W) imL | imR [| dispL]
    on the device; the flipped pair (torch.flip, on the device) gives the second view; nedge = 64
    with ``-mask``, else 0; two forwards and one backward inside ONE ``amax_scope``; Adam step.
    ``augment``: applied to the cropped (B,6,h,w) copy in place of myTransforms.Stereo_color_batch
    (default: identity); the reference's choice is ``transforms.Stereo_color()`` (one fused launch).
    ``nedge``: overrides the crop (None: the reference's rule).
    Returns (loss, D1, EPE) as floats; D1 = EPE = -1 without ground truth (< 7 channels)."""
    from . import costvolume as cv
    if _world(world) > 1:
        raise NotImplementedError("train_step_selfsup runs on a single rank")
    if nedge is None:
        nedge = 64 if lossfun.flag_mask else 0
    with cv.amax_scope(batch.device):          # forward, forward, backward: one arena
        model.train()
        loss, dispLs = _selfsup_forward(model, lossfun, batch, nedge, augment)
        optim.zero_grad()
        if torch.is_tensor(loss):
            loss.backward()
            optim.step()
    d1, epe = _selfsup_accuracy(batch, dispLs, nedge)
    return float(loss.detach() if torch.is_tensor(loss) else loss), d1, epe


def train_step_selfsup_ranks(model, optim, lossfun, batch, augment=None, world=None, nedge=None):
    """``train_step_selfsup`` on any number of ranks.  One rank: exactly its calls.  Several: every
    rank runs forward, forward, backward on its own batch -- with its own augmentation and epsilons,
    drawn from its own generator --, then ONE flat gradient all-reduce
    (``sharding.allreduce_gradients``: the mean over ranks) and the optimizer step.  Every rank must
    call it every step.  Returns the rank's own (loss, D1, EPE)."""
    from . import costvolume as cv
    world = _world(world)
    if world == 1:
        return train_step_selfsup(model, optim, lossfun, batch, augment=augment, world=1, nedge=nedge)
    if nedge is None:
        nedge = 64 if lossfun.flag_mask else 0
    with cv.amax_scope(batch.device):
        model.train()
        loss, dispLs = _selfsup_forward(model, lossfun, batch, nedge, augment)
        optim.zero_grad()
        if torch.is_tensor(loss):              # no weighted level: zero gradients, the collective all the same
            loss.backward()
        sharding.allreduce_gradients(model.parameters(), world=world)
        optim.step()
    d1, epe = _selfsup_accuracy(batch, dispLs, nedge)
    return float(loss.detach() if torch.is_tensor(loss) else loss), d1, epe


def validate_step_selfsup(model, lossfun, batch, augment=None):
    """One iteration of stereo_selfsupervised.py:148-200: eval mode, nedge = 0, no gradients.
    ``augment``: as in ``train_step_selfsup``; the reference's choice is ``transforms.Stereo_normalize()``."""
    from . import costvolume as cv
    model.eval()
    with torch.no_grad(), cv.amax_scope(batch.device):
        loss, dispLs = _selfsup_forward(model, lossfun, batch, 0, augment)
    d1, epe = _selfsup_accuracy(batch, dispLs, 0)
    return float(loss), d1, epe


def evaluate_step(model, batch, augment=None, per_image=False):
    """Every evaluation number of one batch in two launches after the forward, without a host read:
    ``costvolume.stereo_metrics`` on the model's first output (csrc/metrics.hip; utils/evaluate.py,
    stereo.py:103-113).  ``batch`` (B,>=6,H,W) imL | imR [| dispL] on the device.  With >= 7 channels
    ``batch[:, 6:7]`` is the ground truth; without, the ground-truth metrics are NaN and the
    photometric ones are what judges a self-supervised run.  The images of the photometric error are
    the batch's own (un-augmented, so non-negative: see ``dsmnet_amd.evaluate``), warped with the sign
    the losses use (``imwrap_BCHW(imR, dispL)``, loss.py:449).  ``augment``: applied to the copy the
    network sees, as in ``validate_step_selfsup`` (the reference's choice: ``transforms.Stereo_normalize()``).
    Eval mode, no gradients, one ``amax_scope``.  Returns ``stereo_metrics_finish``'s dict of float64
    device tensors, over the whole batch or, with ``per_image``, one value per image."""
    from . import costvolume as cv
    if batch.dim() != 4 or batch.shape[1] < 6:
        raise ValueError("an evaluation batch is (B, >=6, H, W): imL | imR [| dispL]")
    model.eval()
    seen = batch[:, :6]
    if augment is not None:
        seen = augment(seen.clone())
    with torch.no_grad(), cv.amax_scope(batch.device):
        _, dispLs = model(seen[:, :3], seen[:, 3:6])
        gt = batch[:, 6:7] if batch.shape[1] >= 7 else None
        sums = cv.stereo_metrics(dispLs[0], gt, batch[:, :3], batch[:, 3:6])
        return cv.stereo_metrics_finish(sums, per_image=per_image)
