"""``DeviceLoader``: from a ``Dataset_stereo`` to device batches without forming fp32 frames.

Per batch: the samples are decoded by a thread pool (``Dataset_stereo.raw_item``), every plane is
packed as decoded -- 8-bit RGB, 8/16-bit or float32 disparity -- into one pinned staging buffer,
one non-blocking copy takes it to the device, and ``Compose.call_raw`` turns the bytes into the
(B, C, h, w) batch: one ``dsm_stereo_spatial_raw`` launch per 32 images (crop to the common size,
float conversion, concatenation, flip, shift, crop, scale, ToTensor), then the colour launches.

Random numbers, per image in index order: the flip's ``np.random.rand()`` (drawn only when the
dataset is ``Train`` and C is even), then ``Spatial_stereo.draw``'s numbers -- the order of the
reference's loop with ``num_workers=0``; the colour draws follow through ``Compose.plan``.
``shuffle=True`` draws one ``torch.randperm(len)`` per epoch on the CPU generator.

Iterate a loader on one stream.  Not capturable into a hipGraph: offsets and sizes change from
batch to batch.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import transforms as T

MAX_THREADS = 16


def pack_layout(items, formats):
    """Where every plane of a batch goes in the staging buffer.  ``items``: ``raw_item`` results;
    ``formats``: each sample's ``disp_format``.  Returns ``(sources, total_bytes)``, ``sources`` in
    the field order of ``dsm_frame_source`` with flip 0.  RGB planes go anywhere; a uint16 plane
    starts at an even offset, a float32 plane at a multiple of 4."""
    sources, at = [], 0
    for (planes, (y0, x0), _, _), fmt in zip(items, formats):
        offs = []
        for p in planes:
            at = -(-at // p.dtype.itemsize) * p.dtype.itemsize
            offs.append(at)
            at += p.nbytes
        offs += [-1] * (4 - len(offs))
        Hs, Ws = planes[0].shape[:2]
        sources.append((offs[0], offs[1], offs[2], offs[3], Hs, Ws, y0, x0, 0, fmt))
    return sources, at


class DeviceLoader(object):
    """An iterable of ``(batch, filenames)``; ``batch`` is the new (B, C, h, w) fp32 device tensor
    that ``transform`` (one of the four recipes: a ``transforms.Compose`` led by ``Spatial_stereo``
    and / or ``ToTensor_numpy``) makes of ``batch_size`` samples of ``dataset``, bit-identical to
    ``transform`` applied to the samples' fp32 frames.  ``threads`` decode (at most 16)."""

    def __init__(self, dataset, transform, batch_size, shuffle=False, drop_last=False, device=None, threads=4):
        if not isinstance(transform, T.Compose) or (transform.spatial is None and transform.to_tensor is None):
            raise TypeError("DeviceLoader: transform must be a transforms.Compose led by Spatial_stereo and / or "
                            "ToTensor_numpy (Stereo_train, Stereo_Spatial, Stereo_ToTensor, Stereo_eval), got %r"
                            % (transform,))
        if int(batch_size) < 1:
            raise ValueError("DeviceLoader: batch_size must be positive, got %r" % (batch_size,))
        self.dataset, self.transform, self.batch_size = dataset, transform, int(batch_size)
        self.shuffle, self.drop_last, self.device = bool(shuffle), bool(drop_last), device
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self._stage = [None, None]          # pinned staging buffers, used alternately
        self._copied = [None, None]         # event after the last copy out of each
        self._turn = 0
        self._dev = None

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        n = len(self.dataset)
        order = torch.randperm(n).tolist() if self.shuffle else list(range(n))
        with ThreadPoolExecutor(max_workers=self.threads) as pool:
            for i in range(0, n, self.batch_size):
                idxs = order[i:i + self.batch_size]
                if len(idxs) < self.batch_size and self.drop_last:
                    return
                yield self._batch(pool, idxs)

    def _batch(self, pool, idxs):
        ds = self.dataset
        items = list(pool.map(ds.raw_item, idxs))
        sizes = set(it[2] for it in items)
        if len(sizes) != 1:
            raise ValueError("DeviceLoader: the samples of a batch differ in size (%s) and the dataset has no "
                             "size_min to crop them to" % sorted(sizes))
        C = ds.channels
        formats = [ds.disp_format(it[0][2]) if C >= 7 else 0 for it in items]
        sources, total = pack_layout(items, formats)
        device = torch.device("cuda", torch.cuda.current_device()) if self.device is None else torch.device(self.device)
        k, self._turn = self._turn, self._turn ^ 1
        # State that outlives a launch: the copy out of staging buffer k two batches ago may still be
        # in flight.  Its event is waited on (this host thread only, no device-wide synchronise)
        # before the host writes the buffer again or lets go of it.
        if self._copied[k] is not None:
            self._copied[k].synchronize()
        if self._stage[k] is None or self._stage[k].numel() < total:
            self._stage[k] = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=True)
        stage = self._stage[k].numpy()
        for (planes, _, _, _), s in zip(items, sources):
            for p, off in zip(planes, s[:4]):
                stage[off:off + p.nbytes] = p.reshape(-1).view(np.uint8)
        with torch.cuda.device(device):
            # State that outlives a launch: the device buffer is read by the previous batch's launch.
            # The copy below, and a replacement's allocation, are ordered behind it by the stream.
            if self._dev is None or self._dev.numel() < total or self._dev.device != device:
                self._dev = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
            raw = self._dev[:total]
            raw.copy_(self._stage[k][:total], non_blocking=True)
            # the guard of staging buffer k: recorded right after its copy
            self._copied[k] = torch.cuda.Event()
            self._copied[k].record()
            flip = (lambda: int(np.random.rand() > 0.5)) if ds.Train and C % 2 == 0 else None
            batch = self.transform.call_raw(raw, sources, next(iter(sizes)), C, draw_flip=flip)
        return batch, [it[3] for it in items]
