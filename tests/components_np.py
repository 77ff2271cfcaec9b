"""numpy / Python restatement (test infrastructure only) of the connected components of csrc/components.hip, slow and obvious:

  offsets(connectivity)                         the forward neighbour offsets (dz, dy, dx): 3 / 9 / 13 for 6 / 18 / 26
  label(vol, lo, hi, connectivity)              int32 [N, H, W]: -1 on background (vol < lo or vol > hi), otherwise the smallest
                                                linear index of the voxel's component -- an explicit union-find over every pair of
                                                adjacent foreground voxels, the larger root always hung under the smaller
  sizes(labels)                                 int32 [N, H, W]: the voxel count at every root, 0 elsewhere
  select(labels, min_voxels, seeds, largest, ntop) -> (keep uint8 [N, H, W], top int32 [ntop, 2], stats int32 [8])
  apply(vol, labels, keep, background, fill)    int16 [N, H, W]
  level(values, wc, ww, hu)                     project_np.level"""
import numpy as np

from project_np import level  # noqa: F401


LO, HI = 100, 3000      # the threshold band of the test volumes below


def random_field(shape, density, seed):
    """int16 `shape`: a voxel is foreground (a value in LO .. HI, both ends planted) with probability `density`; the background
    lies below LO and above HI, so both ends of the band are tested."""
    rng = np.random.RandomState(seed)
    fg = rng.random_sample(shape) < density
    inside = rng.choice(np.array([LO, LO + 1, 1500, HI - 1, HI], dtype=np.int16), size=shape)
    outside = rng.choice(np.array([-32768, -1024, 0, LO - 1, HI + 1, 32767], dtype=np.int16), size=shape)
    return np.where(fg, inside, outside).astype(np.int16)


def snake(shape, cut=None):
    """One component under every connectivity, with the longest parent chains: on even slices every even row is filled and one
    link voxel on each odd row, at alternating ends, joins the rows to one serpentine; one link voxel on each odd slice, at
    alternating ends too, joins the slices.  cut = (z, y, x): that voxel removed."""
    n, h, w = shape
    vol = np.zeros(shape, dtype=np.int16)
    last = (h - 1) - (h - 1) % 2      # the last even row
    for z in range(n):
        if z % 2 == 0:
            vol[z, 0::2, :] = 1500
            for y in range(1, last, 2):
                vol[z, y, w - 1 if (y // 2) % 2 == 0 else 0] = 1500
        else:
            y, x = (0, 0) if (z // 2) % 2 == 0 else (last, w - 1)
            vol[z, y, x] = 1500
    if cut is not None:
        vol[cut] = 0
    return vol


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return np.where((z + y + x) % 2 == 0, 1500, 0).astype(np.int16)


def offsets(connectivity):
    limit = {6: 1, 18: 2, 26: 3}[connectivity]
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) < (0, 0, 0) and abs(dz) + abs(dy) + abs(dx) <= limit:
                    out.append((dz, dy, dx))
    return out


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def label(vol, lo, hi=32767, connectivity=26):
    vol = np.asarray(vol)
    assert vol.dtype == np.int16 and vol.ndim == 3
    n, h, w = vol.shape
    fg = (vol >= lo) & (vol <= hi)
    index = np.arange(n * h * w, dtype=np.int64).reshape(n, h, w)
    parent = list(range(n * h * w))
    for dz, dy, dx in offsets(connectivity):
        # the voxels (z, y, x) whose neighbour (z + dz, y + dy, x + dx) lies in the volume, and those neighbours
        me = (slice(-dz if dz < 0 else 0, n - dz if dz > 0 else n), slice(-dy if dy < 0 else 0, h - dy if dy > 0 else h),
              slice(-dx if dx < 0 else 0, w - dx if dx > 0 else w))
        nb = (slice(0 if dz <= 0 else dz, n + dz if dz < 0 else n), slice(0 if dy <= 0 else dy, h + dy if dy < 0 else h),
              slice(0 if dx <= 0 else dx, w + dx if dx < 0 else w))
        both = fg[me] & fg[nb]
        for a, b in zip(index[me][both].tolist(), index[nb][both].tolist()):
            ra, rb = _find(parent, a), _find(parent, b)
            if ra < rb:
                parent[rb] = ra
            elif rb < ra:
                parent[ra] = rb
    out = np.full(n * h * w, -1, dtype=np.int32)
    for i in np.flatnonzero(fg.reshape(-1)).tolist():
        out[i] = _find(parent, i)
    return out.reshape(n, h, w)


def sizes(labels):
    flat = np.asarray(labels).reshape(-1)
    return np.bincount(flat[flat >= 0], minlength=flat.size).astype(np.int32).reshape(np.shape(labels))


def select(labels, min_voxels=1, seeds=None, largest=0, ntop=8):
    flat = np.asarray(labels).reshape(-1)
    size = sizes(flat)
    roots = np.flatnonzero(size > 0)
    stats = np.zeros(8, dtype=np.int32)
    stats[0] = int((flat >= 0).sum())
    stats[1] = roots.size
    seeded = None
    if seeds is not None and len(seeds) > 0:
        seeded = set()
        for s in seeds:
            s = int(s)
            if 0 <= s < flat.size and flat[s] >= 0:
                seeded.add(int(flat[s]))
            else:
                stats[5] += 1
    cand = [int(r) for r in roots if size[r] >= min_voxels and (seeded is None or int(r) in seeded)]
    cand.sort(key=lambda r: (-int(size[r]), r))
    stats[2] = len(cand)
    kept = cand[:largest] if largest > 0 else cand
    stats[3] = len(kept)
    stats[4] = sum(int(size[r]) for r in kept)
    keep = np.zeros(flat.size, dtype=np.uint8)
    keep[kept] = 1
    top = np.tile(np.array([-1, 0], dtype=np.int32), (ntop, 1))
    for p, r in enumerate(kept[:ntop]):
        top[p] = (r, size[r])
    return keep.reshape(np.shape(labels)), top, stats


def apply(vol, labels, keep, background=False, fill=0):
    vol, flat = np.asarray(vol), np.asarray(labels).reshape(-1)
    fg = flat >= 0
    kept = np.zeros(flat.size, dtype=bool)
    kept[fg] = np.asarray(keep).reshape(-1)[flat[fg]] == 1
    stay = kept | (~fg if background else np.zeros(flat.size, dtype=bool))
    return np.where(stay.reshape(vol.shape), vol, np.int16(fill)).astype(np.int16)
