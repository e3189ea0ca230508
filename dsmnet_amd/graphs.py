"""hipGraph replay of a whole eval-mode forward.

A PSMNet forward is ~110 launches of 10-700 us; replaying them from one captured graph takes the
Python/ctypes launch path (3-5 ms of host time per forward) off the critical path, which matters
when eight ranks share one host.  Everything on the eval path is capture-safe: the library
launches on torch's current stream, never allocates or synchronises, and all scratch and
output tensors come from torch's caching allocator (graph-private pool during capture).
"""
import torch


class GraphedForward(object):
    """``g = GraphedForward(model, left, right)``; ``scales, disps = g(left2, right2)``.

    Inputs of the captured shapes are copied into static buffers and the graph is replayed;
    the returned tensors are the graph's static outputs (overwritten by the next call --
    ``clone()`` what must outlive it).  Eval mode / no-grad only."""

    def __init__(self, model, *example_inputs, warmup=3):
        if model.training:
            raise ValueError("GraphedForward captures an eval-mode forward: call model.eval() first")
        if not all(t.is_cuda for t in example_inputs):
            raise RuntimeError("GraphedForward needs CUDA (HIP) tensors: there is no CPU fallback")
        self.model = model
        self.static_in = [t.clone() for t in example_inputs]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(warmup):           # weight packing, BN folding, kernel attributes
                model(*self.static_in)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.static_out = model(*self.static_in)

    def replay(self):
        self.graph.replay()
        return self.static_out

    def __call__(self, *inputs):
        if len(inputs) != len(self.static_in):
            raise ValueError("expected %d inputs" % len(self.static_in))
        for dst, src in zip(self.static_in, inputs):
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError("GraphedForward was captured for %s %s, got %s %s"
                                 % (tuple(dst.shape), dst.dtype, tuple(src.shape), src.dtype))
            dst.copy_(src)
        return self.replay()


class GraphedTrainStep(object):
    """One supervised training step -- train-mode forward, pyramid loss, backward, optimizer step
    (``train.train_step`` without its host-side metrics) -- captured once and replayed.

    A PSMNet step is ~3,000 kernel launches, most of them stock torch / MIOpen kernels of ~5 us for
    the train-mode 2-D towers; on an idle host the replay takes about as long as eager launches, and
    what the graph buys is independence from the host when several ranks share it.
    ``step = GraphedTrainStep(model, optim, lossfun, batch)``;
    ``loss, disps = step(next_batch)`` (static tensors).
    The optimizer must be built with ``capturable=True``; build it with ``fused=True`` as well: the
    capturable foreach Adam issues ~4 tiny kernels per parameter tensor (518 divisions and 145
    counter increments per PSMNet step, 3 ms of a 27 ms step at 256x512 -- DESIGN.md section 9).

    Several ranks (``torch.distributed`` initialised, or ``world=N``): the forward and the backward
    are the captured graph -- the ~3,000 launches that would otherwise go through eight Python
    interpreters sharing one host -- with every gradient a view of one flat buffer
    (``sharding.FlatGradients``); after the replay come, eagerly, ONE all-reduce of that buffer
    over RCCL (+ one division) and the fused optimizer step: three or four launches per step outside
    the graph.  (Capturing the collective itself would save those at the price of tying the graph
    to the communicator's state; with 20.9 MB per step and a step of >= 100 ms it buys nothing.)
    A rank whose batch has no ground-truth pixel contributes zero gradients and takes part in the
    collective all the same; the number of ranks that had ground truth rides in the same buffer
    and the optimizer step is skipped on every rank together when it is zero (as
    ``train.train_step`` does).  ``model.zero_grad()`` / ``optim.zero_grad()`` between steps are
    harmless in this form: the views are re-attached before the eager optimizer step.

    Every call drops the cached packed weights and BN folds of the eval path
    (``blocks3d.invalidate_folded_caches``): a replay changes weights and running statistics without
    running the Python that would have bumped their version counters.

    An eager backward through the same model before the capture leaves gradient tensors and
    autograd buffers that were allocated OUTSIDE the capture's private pool, on the default
    stream; re-used inside the capture (``.grad`` accumulation, a freed block handed back by the
    caching allocator with a pending cross-stream event) they invalidate it, and the HIP runtime
    aborted in ``capture_end`` instead of raising.  The constructor therefore drops every
    gradient, collects garbage (dead autograd graphs release their buffers) and synchronises
    the device before the side-stream warm-up and again before the capture, so that the capture
    starts from allocations of its own (tests/test_models_gpu.py:
    ``test_graphed_train_step_after_an_eager_step_on_the_same_model``)."""

    n_extra = 1          # floats after the gradients in the flat buffer: "this rank had ground truth"

    def __init__(self, model, optim, lossfun, example_batch, warmup=3, world=None, flat_gradients=None):
        """``flat_gradients``: force (True) the multi-rank form -- forward + backward captured, flat
        gradient exchange and optimizer step outside -- also in a single process (tests); default:
        exactly when there are several ranks."""
        self._bind(model, optim, lossfun, world, flat_gradients)
        if not example_batch.is_cuda or example_batch.shape[1] < 7:
            raise ValueError("GraphedTrainStep needs a CUDA (HIP) batch (B, >=7, H, W): imL | imR | dispL")
        lossfun.capturable = True
        model.train()
        self.batch = example_batch[:, :7].clone()
        self._capture(warmup)

    def _bind(self, model, optim, lossfun, world, flat_gradients):
        import torch.distributed as dist
        if world is None:
            world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.world = int(world)
        self.split = bool(flat_gradients) if flat_gradients is not None else self.world > 1
        if not all(g.get("capturable", False) for g in optim.param_groups):
            raise ValueError("%s: build the optimizer with capturable=True" % type(self).__name__)
        self.model, self.optim, self.lossfun = model, optim, lossfun

    def _prepare(self):
        """Whatever ``_step`` needs that is not known before a first forward (on the warm-up stream)."""

    def _capture(self, warmup):
        """Quiesce, warm up on a side stream, quiesce again, capture ``_step`` (see the class docstring)."""
        self.flatgrads = None
        self._quiesce()
        if self.split:
            from . import sharding
            self.flatgrads = sharding.FlatGradients(self.model.parameters(), n_extra=self.n_extra)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._prepare()
            for _ in range(warmup):
                self._step()
        torch.cuda.current_stream().wait_stream(side)
        self._quiesce()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss, self.disps = self._step()

    def _quiesce(self):
        """No gradient, no dead autograd graph, no kernel in flight: the state a capture (or the
        warm-up on the side stream) must start from."""
        import gc
        if self.flatgrads is None:
            self.optim.zero_grad(set_to_none=True)
            for p in self.model.parameters():
                p.grad = None
        else:
            self.flatgrads.attach()
        gc.collect()
        torch.cuda.synchronize()

    def _step(self):
        from . import costvolume as cv
        with cv.amax_scope(self.batch.device):      # fp16 convolution modes: one arena of maxima per step
            return self._step_body()

    def _step_body(self):
        b = self.batch
        if self.flatgrads is not None:
            # several ranks: only forward + backward are captured; gradients accumulate into the
            # views of the flat buffer, whose last float counts "this rank had ground truth"
            self.flatgrads.zero()
            scales, disps = self.model(b[:, :3], b[:, 3:6])
            loss = self.lossfun({"disp_gt": b[:, 6:7], "disps": disps, "scale_disps": scales,
                                 "flag_smooth": True})
            loss.backward()
            self.flatgrads.extra.copy_((b[:, 6:7] > 0).any().to(self.flatgrads.flat.dtype).reshape(1))
            return loss.detach(), [d.detach() for d in disps]
        self.optim.zero_grad(set_to_none=True)
        scales, disps = self.model(b[:, :3], b[:, 3:6])
        loss = self.lossfun({"disp_gt": b[:, 6:7], "disps": disps, "scale_disps": scales,
                             "flag_smooth": True})
        loss.backward()
        self.optim.step()
        return loss.detach(), [d.detach() for d in disps]

    def _exchange_and_update(self):
        """The part of a multi-rank step that stays outside the graph."""
        self.flatgrads.reattach()                # a zero_grad() since the last step unbound the views
        n_gt = self.flatgrads.allreduce(self.world)
        if float(n_gt) > 0:                      # (a host read: one scalar per step)
            self.optim.step()

    def __call__(self, batch):
        if batch.shape[0] != self.batch.shape[0] or batch.shape[2:] != self.batch.shape[2:]:
            raise ValueError("GraphedTrainStep was captured for %s, got %s"
                             % (tuple(self.batch.shape), tuple(batch.shape)))
        from . import blocks3d
        self.batch.copy_(batch[:, :7])
        self.graph.replay()
        # the replay ran no Python: the captured optimizer step and the BN kernels' raw-pointer writes
        # bumped no version counter, so every fold made from these tensors is stale (DESIGN.md
        # section 9, "state that outlives a launch")
        blocks3d.invalidate_folded_caches()
        if self.flatgrads is not None:
            self._exchange_and_update()
        return self.loss, self.disps


class GraphedSelfsupStep(GraphedTrainStep):
    """One self-supervised training step (``train.train_step_selfsup`` without its host-side metrics)
    captured once and replayed: the two flips, both train-mode forwards inside one ``amax_scope``, the
    fused pyramid loss, the backward and, in the single-process form, the optimizer step.
    ``step = GraphedSelfsupStep(model, optim, lossfun, batch, augment=None, nedge=None)``;
    ``loss, dispLs = step(next_batch)`` (static tensors; ``costvolume.stereo_metrics`` on them gives
    D1 / EPE).  ``batch``: (B, >=6, H, W) imL | imR on the device, channels 0..5 are used.

    What changes from step to step does not live in the graph.  The reference draws the epsilons of
    its warps afresh for every step and moves the level weights every epoch; the fused loss reads
    both from a device array when its kernels RUN (``costvolume.selfsup_pyramid_loss(params=)``,
    dsm_selfsup_dyn_*).  A call therefore, in this order: copies the batch into its static buffer,
    crops it and applies ``augment`` eagerly to the cropped copy (its host draws come first, as in
    the eager step); draws the step's epsilons from the CPU generator in the reference's order
    (``lossfun.draw_step_params``, with the current ``weight_levels``) into pinned memory and sends
    them with a non-blocking copy -- the host never waits for the device, and a pinned buffer is
    used again only once its copy's event has completed (else a new one is made); replays.  So
    ``lossfun.Weight_Adjust_levels(epoch)`` between calls needs no new capture -- unless it changes
    WHICH levels have a weight, which is the graph's shape: the call then raises ``ValueError``.
    Build the step after the weights have been adjusted once (the constructor's default weights
    enter the finest level only).

    Several ranks, or ``flat_gradients=True``: forwards and backward are captured, into
    ``sharding.FlatGradients`` views; ``reattach()``, one all-reduce and the optimizer step follow
    eagerly.  Every rank draws its own augmentation and epsilons.  The rest -- capturable optimizer,
    ``invalidate_folded_caches`` after every replay, the quiesce / warm-up / capture sequence -- is
    ``GraphedTrainStep``'s."""

    n_extra = 0          # no "had ground truth" count: every rank always has a loss

    def __init__(self, model, optim, lossfun, example_batch, augment=None, nedge=None, warmup=3, world=None,
                 flat_gradients=None):
        self._bind(model, optim, lossfun, world, flat_gradients)
        if not hasattr(lossfun, "draw_step_params") or lossfun.lossesfun == lossfun.losses_pyramid0:
            raise ValueError("GraphedSelfsupStep needs a self-supervised loss (train.selfsup_losses)")
        if not example_batch.is_cuda or example_batch.dim() != 4 or example_batch.shape[1] < 6:
            raise ValueError("GraphedSelfsupStep needs a CUDA (HIP) batch (B, >=6, H, W): imL | imR")
        self.nedge = nedge = (64 if lossfun.flag_mask else 0) if nedge is None else int(nedge)
        h, w = example_batch.shape[2:]
        if h <= 2 * nedge or w <= 2 * nedge:
            raise ValueError("GraphedSelfsupStep: H, W must exceed 2 * nedge = %d" % (2 * nedge))
        self.augment = augment
        model.train()
        self.batch = example_batch[:, :6].clone()
        self.net_in = self._crop(self.batch).clone()          # what the network sees (augmented)
        self.scales = self.entered = self.params = None
        self._pinned = []                                     # [(pinned (2n,4) tensor, event of its last copy)]
        self._capture(warmup)

    def _crop(self, t):
        n = self.nedge
        return t[:, :, n:t.shape[2] - n, n:t.shape[3] - n]

    def _prepare(self):
        """The model's output levels are known only from a forward; with them, the levels the loss
        enters (the captured shape) and the static device array, filled once for the warm-up."""
        with torch.no_grad():
            scales, _ = self.model(self.net_in[:, :3], self.net_in[:, 3:6])
        self.scales = tuple(int(k) for k in scales)
        self.entered = self.lossfun.entered_levels(self.scales)
        first = self.lossfun.draw_step_params(self.scales)
        self.params = first.to(self.batch.device)

    def _send_step_params(self):
        """This step's epsilons and weights, host to device without a host wait."""
        slot = next((s for s in self._pinned if s[1].query()), None)
        if slot is None:                          # every buffer may still be read by a copy in flight
            slot = (torch.empty(tuple(self.params.shape), dtype=torch.float32, pin_memory=True), torch.cuda.Event())
            self._pinned.append(slot)
        self.lossfun.draw_step_params(self.scales, out=slot[0])
        self.params.copy_(slot[0], non_blocking=True)
        slot[1].record()

    def _step_body(self):
        b, x = self.batch, self.net_in
        b1, x1 = torch.flip(b, dims=[-1]), torch.flip(x, dims=[-1])
        if self.flatgrads is not None:
            self.flatgrads.zero()
        else:
            self.optim.zero_grad(set_to_none=True)
        scales, disps = self.model(x[:, :3], x[:, 3:6])
        scales1, disps1 = self.model(x1[:, 3:6], x1[:, :3])
        n = self.nedge
        args = {"imR_src": b[:, 3:6], "imL": self._crop(b[:, :3]), "LeftTop": [n, n],
                "imR1_src": b1[:, :3], "imL1": self._crop(b1[:, 3:6]), "LeftTop1": [n, n],
                "dispLs": disps, "scale_dispLs": scales, "dispL1s": disps1, "scale_dispL1s": scales1}
        was = self.lossfun.step_params
        self.lossfun.step_params = self.params
        try:
            loss = self.lossfun(args)
        finally:
            self.lossfun.step_params = was
        loss.backward()
        if self.flatgrads is None:
            self.optim.step()
        return loss.detach(), [d.detach() for d in disps]

    def _exchange_and_update(self):
        self.flatgrads.reattach()
        self.flatgrads.allreduce(self.world)
        self.optim.step()

    def __call__(self, batch):
        if batch.shape[0] != self.batch.shape[0] or batch.shape[1] < 6 or batch.shape[2:] != self.batch.shape[2:]:
            raise ValueError("GraphedSelfsupStep was captured for %s, got %s"
                             % (tuple(self.batch.shape), tuple(batch.shape)))
        entered = self.lossfun.entered_levels(self.scales)
        if entered != self.entered:
            raise ValueError("GraphedSelfsupStep was captured with the outputs %s entering the loss; the weights "
                             "now enter %s: build a new step" % (list(self.entered), list(entered)))
        from . import blocks3d
        self.batch.copy_(batch[:, :6])
        crop = self._crop(self.batch)
        self.net_in.copy_(crop if self.augment is None else self.augment(crop.clone()))
        self._send_step_params()
        self.graph.replay()
        blocks3d.invalidate_folded_caches()      # as in GraphedTrainStep: the replay bumped no version counter
        if self.flatgrads is not None:
            self._exchange_and_update()
        return self.loss, self.disps
