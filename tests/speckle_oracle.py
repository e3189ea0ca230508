"""numpy restatement of the speckle filter (csrc/speckle.hip, ``costvolume.filter_speckles``; the semantics
are those of include/dsmnet_hip.h) and the seeded maps its tests run on.  numpy only.

    node    isfinite(disp) and (valid is None or valid)
    edge    4-neighbours of one image, both nodes, |disp[p] - disp[q]| <= max_diff, subtracted and compared
            in float32 (numpy's float32 subtraction is correctly rounded, as the device's is)
    size    the nodes of the pixel's connected component, 0 for a pixel that is no node
    keep    node and size > max_size;  out = disp where keep, else new_val

The components come from hooking every root to the smaller root across an edge and then jumping pointers
until every label is a root, repeated to the fixed point: a handful of passes also on a path that is as
long as the image has pixels (a plain min-label propagation would need one pass per pixel of it).

Every generator returns a ``Case`` whose ``disp`` is (B,H,W) float32; ``info`` states the property the map
was built to have.  All of them are deterministic: the same arguments give the same arrays."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", ("disp", "valid", "max_diff", "info"))
FAR = np.float32(64.0)                                  # farther than any max_diff the tests use


def edges(disp, valid, max_diff):
    """(p, q) linear indices over (B,H,W) of every edge, and the node map."""
    disp = np.asarray(disp, np.float32)
    B, H, W = disp.shape
    node = np.isfinite(disp)
    if valid is not None:
        node &= np.asarray(valid).astype(bool)
    d = np.where(node, disp, np.float32(0))             # the value of a non-node is never used
    md = np.float32(max_diff)
    idx = np.arange(B * H * W, dtype=np.int64).reshape(B, H, W)
    with np.errstate(over="ignore"):                    # two finite values may differ by more than float32 holds
        right = node[:, :, 1:] & node[:, :, :-1] & (np.abs(d[:, :, 1:] - d[:, :, :-1]) <= md)
        down = node[:, 1:] & node[:, :-1] & (np.abs(d[:, 1:] - d[:, :-1]) <= md)
    p = np.concatenate([idx[:, :, 1:][right], idx[:, 1:][down]])
    q = np.concatenate([idx[:, :, :-1][right], idx[:, :-1][down]])
    return p, q, node


def labels(p, q, n):
    """The smallest index of each index's component under the edges (p, q)."""
    lab = np.arange(n, dtype=np.int64)
    while True:
        lp, lq = lab[p], lab[q]                          # roots: every label is one after the jumps below
        open_ = lp != lq
        if not open_.any():
            return lab
        lp, lq = lp[open_], lq[open_]
        m = np.minimum(lp, lq)
        np.minimum.at(lab, lp, m)
        np.minimum.at(lab, lq, m)
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt


def filter_speckles(disp, max_size, max_diff, valid=None, new_val=0.0):
    """-> (out float32, keep bool, size int32), each of disp's shape ((B,H,W) or (B,1,H,W))."""
    disp = np.asarray(disp, np.float32)
    shape = disp.shape
    d3 = disp.reshape((shape[0],) + shape[-2:])
    v3 = None if valid is None else np.asarray(valid).reshape(d3.shape)
    p, q, node = edges(d3, v3, max_diff)
    lab = labels(p, q, d3.size).reshape(d3.shape)
    cnt = np.bincount(lab[node], minlength=d3.size)
    size = np.where(node, cnt[lab], 0).astype(np.int32)
    keep = node & (size > max_size)
    out = np.where(keep, d3, np.float32(new_val)).astype(np.float32)
    return out.reshape(shape), keep.reshape(shape), size.reshape(shape)


# ---------------------------------------------------------------------------------------------------
# maps
# ---------------------------------------------------------------------------------------------------
def _band(H, W, row, n):
    """The first n pixels, row-major, of the full-width band that starts at `row`: a connected set."""
    m = np.zeros(H * W, bool)
    m[row * W: row * W + n] = True
    return m.reshape(H, W)


@functools.lru_cache(maxsize=None)
def blobs(H, W, planted=0, seed=0):
    """Piecewise-constant random regions (levels 4 apart, a texture of 0 / 0.25 / 0.5 on top, so that
    max_diff 0, 0.5 and 1 give different regions) with, where they fit, two planted constant regions of
    exactly ``planted`` and ``planted + 1`` pixels, each farther than FAR from everything else:
    info["planted"] = [(value, pixels), ...]."""
    rng = np.random.default_rng(1000 + seed)
    ys = np.sort(rng.integers(0, H, size=max(1, H // 5)))
    xs = np.sort(rng.integers(0, W, size=max(1, W // 9)))
    level = rng.integers(0, 6, size=(len(ys) + 1, len(xs) + 1))
    disp = level[np.searchsorted(ys, np.arange(H), side="right")][:, np.searchsorted(xs, np.arange(W), side="right")]
    disp = (4.0 * disp + 0.25 * rng.integers(0, 3, size=(H, W))).astype(np.float32)
    done = []
    row = min(H - 1, 14)                                  # the bands start just above a tile border
    for k, n in enumerate((planted, planted + 1)):
        rows = -(-n // W)
        if planted < 1 or row + rows > H:
            break
        value = np.float32(1000.0 * (k + 1))
        disp[_band(H, W, row, n)] = value
        done.append((float(value), n))
        row += rows
    return Case(disp[None], None, None, {"planted": done})


@functools.lru_cache(maxsize=None)
def serpentine(H, W):
    """A one-pixel-wide path over every even row end to end, joined through one pixel of the odd rows at
    alternating ends; the rest of the odd rows is FAR away.  info["size"]: the pixels of the path."""
    path = np.zeros((H, W), bool)
    path[0::2] = True
    for y in range(1, H, 2):
        path[y, W - 1 if (y // 2) % 2 == 0 else 0] = True
    disp = np.where(path, np.float32(10), np.float32(10) + FAR).astype(np.float32)
    return Case(disp[None], None, None, {"path": path, "size": int(path.sum())})


@functools.lru_cache(maxsize=None)
def spiral(H, W):
    """A one-pixel-wide spiral path from the top-left corner to the centre, walls one pixel wide and FAR
    away.  info["size"]: the pixels of the path."""
    path = np.zeros((H, W), bool)
    inside = lambda y, x: 0 <= y < H and 0 <= x < W
    y = x = k = 0
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    path[0, 0] = True
    while True:
        for turn in range(2):
            dy, dx = dirs[(k + turn) % 4]
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not path[ny, nx] and not (inside(ay, ax) and path[ay, ax]):
                k, y, x = (k + turn) % 4, ny, nx
                path[y, x] = True
                break
        else:
            break
    disp = np.where(path, np.float32(20), np.float32(20) + FAR).astype(np.float32)
    return Case(disp[None], None, None, {"path": path, "size": int(path.sum())})


def checker(H, W):
    """Every pixel FAR from its four neighbours: all singletons."""
    yy, xx = np.mgrid[0:H, 0:W]
    return Case((((yy + xx) % 2) * FAR + 1).astype(np.float32)[None], None, None, {"size": 1})


def uniform(H, W):
    return Case(np.full((1, H, W), 7.5, np.float32), None, None, {"size": H * W})


def ramp(H, W, step=0.5, joined=True):
    """disp[y, x] = x * step with step a multiple of 0.25 and W <= 1030: every value and difference is exact.
    ``joined``: max_diff == step, one region.  Otherwise step == nextafter(max_diff, inf) (max_diff is the
    float32 just below step): W regions, one per column."""
    assert W <= 1030 and step > 0 and (step * 4) == int(step * 4)
    step = np.float32(step)
    disp = np.broadcast_to(np.arange(W, dtype=np.float32) * step, (1, H, W)).copy()
    md = step if joined else np.nextafter(step, np.float32(0))
    assert joined or np.nextafter(md, np.float32(np.inf)) == step
    return Case(disp, None, float(md), {"size": H * W if joined else H})


def cross(H, W, cy, cx):
    """A plus sign of (up to) five pixels centred at (cy, cx) -- the caller puts it where tiles meet -- on a
    uniform background FAR away.  info["size"]: its pixels inside the image."""
    disp = np.full((H, W), 5 + FAR, np.float32)
    n = 0
    for dy, dx in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
        if 0 <= cy + dy < H and 0 <= cx + dx < W:
            disp[cy + dy, cx + dx] = 5
            n += 1
    return Case(disp[None], None, None, {"size": n, "at": (cy, cx)})


def horseshoe(H, W, y0, xb, down=False):
    """A U of nine pixels: two arms of three pixels in columns xb-3 .. xb-1 of rows y0 and y0 + 2, and the
    bend in column xb, rows y0 .. y0 + 2.  With xb the first column of a tile, the arms lie in one tile
    and meet only through its right neighbour.  ``down``: the same transposed (xb a column, y0 the first
    row of the tile below: arms in rows y0-3 .. y0-1 of columns xb and xb + 2).  Background FAR away."""
    disp = np.full((W, H) if down else (H, W), 9 + FAR, np.float32)
    a, b = (xb, y0) if down else (y0, xb)                # in the untransposed frame: row a, column b
    assert a >= 0 and a + 3 <= disp.shape[0] and b >= 3 and b < disp.shape[1]
    disp[a, b - 3:b] = 9
    disp[a + 2, b - 3:b] = 9
    disp[a:a + 3, b] = 9
    disp = disp.T.copy() if down else disp
    return Case(disp[None], None, None, {"size": 9})


@functools.lru_cache(maxsize=None)
def holes(H, W, planted=0, seed=0):
    """``blobs`` with NaN, +Inf and -Inf pixels and a random ``valid`` mask.  info["poisoned"] / info["plain"]:
    the same map with the values under valid == False set to NaN / to an in-range number: the results must
    be equal."""
    base = blobs(H, W, planted, seed).disp.copy()
    rng = np.random.default_rng(2000 + seed)
    u = rng.random(base.shape)
    base[u < 0.04] = np.nan
    base[(u >= 0.04) & (u < 0.07)] = np.inf
    base[(u >= 0.07) & (u < 0.10)] = -np.inf
    valid = rng.random(base.shape) < 0.8
    poisoned = np.where(valid, base, np.float32(np.nan)).astype(np.float32)
    plain = np.where(valid, base, np.float32(4.25)).astype(np.float32)
    return Case(poisoned, valid, None, {"poisoned": poisoned, "plain": plain})


@functools.lru_cache(maxsize=None)
def pair(H, W, seed=0):
    """B = 2, two different images; the last row of image 0 and the first row of image 1 carry one value."""
    a, b = blobs(H, W, 0, seed + 1).disp[0].copy(), blobs(H, W, 0, seed + 2).disp[0][::-1, ::-1].copy()
    a[H - 1] = 3.0
    b[0] = 3.0
    return Case(np.stack([a, b]), None, None, {"row_value": 3.0})
