"""numpy / Python restatement (test infrastructure only) of the vessel centreline of csrc/centreline.hip, slow and obvious:

  q(d, zq)                                        (d^2 zq + 128) >> 8
  clearance(vol, lo, hi, R, zq)                   uint16 [N, H, W]: 0 on background, otherwise min(R^2, the smallest dx^2 + dy^2 +
                                                  q(|dz|) to a background voxel inside the volume) -- three passes of shifted minima
  clearance_direct(vol, lo, hi, R, zq)            the same from the definition, a loop over every background voxel (small volumes)
  field(clear, pen, steps, start, R)              uint32 [N, H, W]: the least fixed point of dist[v] = min over neighbours u of
                                                  min(dist[u] + step(u -> v), SAT) with dist[start] = 0 -- 26 shifted minima, repeated
                                                  on the neighbourhood of what changed until nothing changes
  trace(clear, pen, steps, dist, ends, R, max_points) -> (paths int32 [E, max_points], counts int32 [E], stats int32 [8])
  helix_tube()                                    the helical vessel of tests/test_reformat.py: (vol, axis points, start, end)"""
import math

import numpy as np

UNREACHED = 0xFFFFFFFF
SAT = 0xFFFFFFFE

OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]


def kind(dz, dy, dx):
    """Which of the five step lengths a move uses: in-plane face, in-plane edge, z alone, z + one in-plane, z + two in-plane."""
    k = (dy != 0) + (dx != 0)
    return k - 1 if dz == 0 else 2 + k


def q(d, zq):
    return (int(d) * int(d) * int(zq) + 128) >> 8


def _shift(a, d, axis, fill):
    """b[i] = a[i + d] along `axis`, `fill` where i + d leaves the array."""
    out = np.full_like(a, fill)
    n = a.shape[axis]
    if abs(d) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(max(d, 0), n + min(d, 0))
    dst[axis] = slice(max(-d, 0), n - max(d, 0))
    out[tuple(dst)] = a[tuple(src)]
    return out


def clearance(vol, lo, hi, R, zq=256):
    vol = np.asarray(vol)
    assert vol.dtype == np.int16 and vol.ndim == 3 and 1 <= R <= 32 and 16 <= zq <= 65535
    fg = (vol >= lo) & (vol <= hi)
    bg = (~fg).astype(np.int64)
    g = np.where(fg, R, 0).astype(np.int64)      # the distance along the row, at most R; outside the volume is not background
    for d in range(1, R):
        for s in (-d, d):
            g = np.where(fg & (_shift(bg, s, 2, 0) == 1), np.minimum(g, d), g)
    f = g * g
    for d in range(1, R):
        for s in (-d, d):
            t = _shift(g, s, 1, R)
            f = np.minimum(f, t * t + d * d)
    f = np.where(fg, np.minimum(f, R * R), 0)
    c = f.copy()
    for d in range(1, vol.shape[0]):
        if q(d, zq) >= R * R:
            break
        for s in (-d, d):
            c = np.minimum(c, _shift(f, s, 0, R * R) + q(d, zq))
    return np.where(fg, c, 0).astype(np.uint16)


def clearance_direct(vol, lo, hi, R, zq=256):
    vol = np.asarray(vol)
    fg = (vol >= lo) & (vol <= hi)
    out = np.zeros(vol.shape, dtype=np.uint16)
    back = np.argwhere(~fg)
    for z, y, x in np.argwhere(fg):
        best = R * R
        for bz, by, bx in back:
            best = min(best, (bx - x) ** 2 + (by - y) ** 2 + q(abs(bz - z), zq))
        out[z, y, x] = best
    return out


def _cost(clear, pen, R):
    """pen[clear] per voxel as the kernels read it: clamped into 1 .. 4095, 0 on background."""
    clear = np.asarray(clear).astype(np.int64)
    p = np.clip(np.asarray(pen).astype(np.int64), 1, 4095)
    assert p.shape == (R * R + 1,)
    return np.where(clear > 0, p[np.minimum(clear, R * R)], 0)


def field(clear, pen, steps, start, R):
    clear = np.asarray(clear)
    n, h, w = clear.shape
    cost = _cost(clear, pen, R).reshape(-1)
    dist = np.full(n * h * w, UNREACHED, dtype=np.uint64)
    stats = np.zeros(8, dtype=np.int32)
    if not (0 <= start < dist.size) or cost[start] == 0:
        stats[0] = 1
        return dist.astype(np.uint32).reshape(n, h, w), stats
    dist[start] = 0
    front = np.array([start], dtype=np.int64)
    while front.size:
        z, y, x = front // (h * w), (front // w) % h, front % w
        changed = []
        for dz, dy, dx in OFFSETS:      # the move u -> v = u + offset, for every u that changed
            vz, vy, vx = z + dz, y + dy, x + dx
            ok = (vz >= 0) & (vz < n) & (vy >= 0) & (vy < h) & (vx >= 0) & (vx < w)
            v = ((vz * h + vy) * w + vx)[ok]
            u = front[ok]
            keep = cost[v] > 0
            v, u = v[keep], u[keep]
            cand = np.minimum(dist[u] + np.uint64(steps[kind(dz, dy, dx)]) * cost[v].astype(np.uint64), np.uint64(SAT))
            low = cand < dist[v]
            if low.any():
                np.minimum.at(dist, v[low], cand[low])
                changed.append(v[low])
        front = np.unique(np.concatenate(changed)) if changed else np.zeros(0, dtype=np.int64)
    stats[3] = int((dist == SAT).any())
    return dist.astype(np.uint32).reshape(n, h, w), stats


def trace(clear, pen, steps, dist, ends, R, max_points):
    clear = np.asarray(clear)
    n, h, w = clear.shape
    cost = _cost(clear, pen, R).reshape(-1)
    d = np.asarray(dist).reshape(-1).astype(np.int64)
    paths = np.full((len(ends), max_points), -1, dtype=np.int32)
    counts = np.zeros(len(ends), dtype=np.int32)
    stats = np.zeros(8, dtype=np.int32)
    for e, v in enumerate(int(t) for t in ends):
        if not (0 <= v < d.size) or cost[v] == 0 or d[v] == UNREACHED:
            stats[1] += 1
            continue
        k = 0
        while True:
            if k >= max_points:
                counts[e] = -1
                stats[2] += 1
                break
            paths[e, k] = v
            k += 1
            if d[v] == 0:
                counts[e] = k
                break
            z, y, x = v // (h * w), (v // w) % h, v % w
            best = None
            for dz, dy, dx in OFFSETS:      # u = v + offset; the move u -> v has the kind of the offset
                uz, uy, ux = z + dz, y + dy, x + dx
                if not (0 <= uz < n and 0 <= uy < h and 0 <= ux < w):
                    continue
                u = (uz * h + uy) * w + ux
                if cost[u] == 0 or d[u] == UNREACHED or d[u] >= d[v]:
                    continue
                if min(d[u] + steps[kind(dz, dy, dx)] * cost[v], SAT) == d[v] and (best is None or u < best):
                    best = u
            if best is None:
                counts[e] = -2
                stats[4] += 1
                stats[6] = 1
                break
            v = int(best)
    return paths, counts, stats


def blobs(shape, seed, count=None, rmax=5.0):
    """int16 `shape`: the union of random balls (1500) on a background of 0, with the corners of the volume kept background."""
    rng = np.random.RandomState(seed)
    n, h, w = shape
    z, y, x = np.indices(shape)
    vol = np.zeros(shape, dtype=np.int16)
    count = max(3, (n * h * w) // 600) if count is None else count
    for _ in range(count):
        c = rng.random_sample(3) * np.array(shape)
        r = 1.0 + rng.random_sample() * (rmax - 1.0)
        vol[(z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r] = 1500
    vol[0, 0, 0] = 0
    return vol


def helix_tube():
    """The 40 x 48 x 44 helical tube of radius 2.5 of tests/test_reformat.py -> (vol int16, the axis points float64 [400, 3] in
    (z, y, x), the voxel nearest the first axis point, the voxel nearest the last)."""
    n, h, w = 40, 48, 44
    turn = np.linspace(0.0, 3.0 * math.pi, 400)
    helix = np.stack([3.0 + 33.0 * turn / turn[-1], 24.0 + 12.0 * np.sin(turn), 22.0 + 12.0 * np.cos(turn)], axis=1)
    z, y, x = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
    grid = np.stack([z, y, x], axis=-1).reshape(-1, 1, 3).astype(np.float32)
    near = np.concatenate([((grid[s:s + 8192] - helix[None].astype(np.float32)) ** 2).sum(axis=2).min(axis=1)
                           for s in range(0, len(grid), 8192)])
    vol = np.where(near.reshape(n, h, w) <= 2.5 ** 2, 1000, 0).astype(np.int16)
    ends = [tuple(int(round(v)) for v in helix[i]) for i in (0, -1)]
    return vol, helix, ends[0], ends[1]


def axis_distance(points, axis):
    """For every point (z, y, x) the distance to the nearest of the axis points."""
    p = np.asarray(points, dtype=np.float64)[:, None, :]
    return np.sqrt(((p - np.asarray(axis, dtype=np.float64)[None]) ** 2).sum(axis=2).min(axis=1))
