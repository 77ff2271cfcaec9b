"""CPU: the definition of the vessel centreline (tests/centreline_np.py, the restatement csrc/centreline.hip is compared with on the
GPU) against scipy -- the clearance against the Euclidean distance transform, the cost field against Dijkstra on the directed
graph -- the properties of a traced path, the tie-break, a helical vessel end to end through the host geometry, and the refusals
that need no GPU."""
import functools
import os

import numpy as np
import pytest

import centreline_np as clnp
import reformat_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGS = {"ctg_centreline_clearance": "piiiiiiippp", "ctg_centreline_seed": "piiilpppipp", "ctg_centreline_relax": "piiipiiiiiipppiiipp",
        "ctg_centreline_saturated": "plpp", "ctg_centreline_trace": "piiipiiiiiippiipppp"}
LO, HI = 100, 3000


def test_header_and_binding_carry_the_entries():
    from cta_gan_amd import _lib, ops
    from test_abi import parse_header
    header = parse_header()
    for name, sig in SIGS.items():
        assert header.get(name) == sig and _lib.SIGNATURES.get(name) == sig, name
    text = open(os.path.join(ROOT, "include", "ctagan_hip.h")).read()
    comment = text.split("int ctg_centreline_clearance(")[0][-6500:]
    assert "added under ABI 15: purely additive" in comment and "infer.py" in comment
    assert _lib.ABI_VERSION == 15 and "#define CTG_ABI_VERSION 15" in text
    src = open(os.path.join(ROOT, "cta_gan_amd", "csrc", "centreline.hip")).read()
    assert src.count('extern "C"') == len(SIGS) and all('extern "C" int ' + name + "(" in src for name in SIGS)
    tz, ty, tx = ops.CENTRELINE_TILE
    assert "#define CL_TZ %d\n" % tz in src and "#define CL_TY %d\n" % ty in src and "#define CL_TX %d\n" % tx in src


# ---------------------------------------------------------------------------------------------- 1. clearance
@pytest.mark.parametrize("shape", [(9, 33, 131), (13, 17, 70)])
def test_clearance_is_the_capped_squared_distance_transform(shape):
    from scipy.ndimage import distance_transform_edt
    vol = clnp.blobs(shape, seed=shape[2])
    fg = (vol >= LO) & (vol <= HI)
    assert 0.05 < fg.mean() < 0.95 and fg[:, :, 0].any()      # background inside, and vessels cut by a face of the volume
    edt2 = np.rint(distance_transform_edt(fg) ** 2).astype(np.int64)
    for r in (1, 3, 6):
        got = clnp.clearance(vol, LO, HI, r)
        assert got.dtype == np.uint16 and np.array_equal(got, np.minimum(edt2, r * r))
    assert clnp.clearance(vol, LO, HI, 3).max() == 9 and edt2.max() > 9      # the cap is reached


def test_clearance_with_thick_slices_equals_the_definition():
    vol = clnp.blobs((7, 12, 14), seed=5, count=6, rmax=4.0)
    for r, zq in ((4, 1600), (6, 1600), (3, 256), (5, 64)):
        assert np.array_equal(clnp.clearance(vol, LO, HI, r, zq), clnp.clearance_direct(vol, LO, HI, r, zq)), (r, zq)
    full = np.full((3, 4, 5), 1500, dtype=np.int16)      # no background at all: outside the volume is not background
    assert (clnp.clearance(full, LO, HI, 5) == 25).all()
    assert (clnp.clearance(np.zeros((3, 4, 5), dtype=np.int16), LO, HI, 5) == 0).all()
    assert clnp.q(1, 256) == 1 and clnp.q(3, 1600) == 56 and clnp.q(2, 16) == 0


# ---------------------------------------------------------------------------------------------- 2. the cost field
@functools.lru_cache(maxsize=None)
def blob_case():
    from cta_gan_amd.infer import centreline_penalty, centreline_steps
    vol = clnp.blobs((13, 40, 70), seed=11)
    r = 4
    clear = clnp.clearance(vol, LO, HI, r)
    pen, steps = centreline_penalty(r), centreline_steps(1.0)
    from scipy.ndimage import label
    lab, count = label(clear > 0, structure=np.ones((3, 3, 3)))
    big = int(np.argmax(np.bincount(lab.reshape(-1))[1:])) + 1
    members = np.flatnonzero(lab.reshape(-1) == big)
    start = int(members[0])
    dist, stats = clnp.field(clear, pen, steps, start, r)
    return vol, clear, pen, steps, r, lab, big, members, start, dist, stats


def test_field_is_dijkstra_on_the_directed_graph():
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    vol, clear, pen, steps, r, lab, big, members, start, dist, stats = blob_case()
    n, h, w = clear.shape
    assert members.size > 2000 and int(lab.max()) > 1 and stats.tolist() == [0] * 8
    cost = clnp._cost(clear, pen, r)
    z, y, x = np.indices(clear.shape)
    rows, cols, vals = [], [], []
    for dz, dy, dx in clnp.OFFSETS:
        vz, vy, vx = z + dz, y + dy, x + dx
        ok = (vz >= 0) & (vz < n) & (vy >= 0) & (vy < h) & (vx >= 0) & (vx < w) & (cost > 0)
        u = ((z * h + y) * w + x)[ok]
        v = ((vz * h + vy) * w + vx)[ok]
        keep = cost.reshape(-1)[v] > 0
        rows.append(u[keep])
        cols.append(v[keep])
        vals.append(steps[clnp.kind(dz, dy, dx)] * cost.reshape(-1)[v[keep]])
    graph = csr_matrix((np.concatenate(vals).astype(np.float64), (np.concatenate(rows), np.concatenate(cols))), shape=(clear.size,) * 2)
    want = dijkstra(graph, directed=True, indices=start)      # costs below 2^31: exact in float64
    flat = dist.reshape(-1)
    reached = np.isfinite(want)
    assert np.array_equal(reached, lab.reshape(-1) == big) and (flat[~reached] == clnp.UNREACHED).all()
    assert want[reached].max() < 2 ** 31 and np.array_equal(flat[reached].astype(np.float64), want[reached])
    # a start on background or outside the volume reaches nothing and is counted
    for bad in (int(np.flatnonzero(clear.reshape(-1) == 0)[0]), -1, clear.size):
        d, s = clnp.field(clear, pen, steps, bad, r)
        assert (d == clnp.UNREACHED).all() and s.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- 3. the trace
def test_a_traced_path_is_connected_descends_and_ends_at_the_start():
    vol, clear, pen, steps, r, lab, big, members, start, dist, stats = blob_case()
    n, h, w = clear.shape
    other = int(np.flatnonzero((lab.reshape(-1) != big) & (lab.reshape(-1) > 0))[0])
    ends = [int(members[-1]), int(members[members.size // 2]), other, int(np.flatnonzero(clear.reshape(-1) == 0)[0]), -5, clear.size, start]
    paths, counts, st = clnp.trace(clear, pen, steps, dist, ends, r, 400)
    assert counts[2:6].tolist() == [0, 0, 0, 0] and counts[6] == 1 and (counts[:2] > 10).all() and st.tolist() == [0, 4, 0, 0, 0, 0, 0, 0]
    assert (paths[2:6] == -1).all() and paths[6, 0] == start
    flat = dist.reshape(-1).astype(np.int64)
    for e in (0, 1):
        p = paths[e, :counts[e]].astype(np.int64)
        assert p[0] == ends[e] and p[-1] == start and (paths[e, counts[e]:] == -1).all()
        zyx = np.stack([p // (h * w), (p // w) % h, p % w], axis=1)
        assert (np.abs(np.diff(zyx, axis=0)).max(axis=1) == 1).all()      # 26-adjacent
        assert (np.diff(flat[p]) < 0).all() and flat[p[-1]] == 0
    short = int(counts[0]) - 1
    paths2, counts2, st2 = clnp.trace(clear, pen, steps, dist, ends[:1], r, short)
    assert counts2.tolist() == [-1] and st2[2] == 1 and np.array_equal(paths2[0], paths[0, :short])


def test_ties_go_to_the_smallest_linear_index():
    # 1 x 2 x 3, every voxel foreground, no background anywhere: clear = R^2 = 1, a flat penalty.  From 0 = (0, 0) to 5 = (1, 2):
    # 0 -> 1 -> 5 (10 + 14) and 0 -> 4 -> 5 (14 + 10) cost the same; the walk back from 5 takes 1, the smaller index
    full = np.full((1, 2, 3), 1500, dtype=np.int16)
    clear = clnp.clearance(full, LO, HI, 1)
    pen = np.array([1, 1], dtype=np.uint16)
    dist, _ = clnp.field(clear, pen, (10, 14, 10, 14, 17), 0, 1)
    assert dist.reshape(-1).tolist() == [0, 10, 20, 10, 14, 24]
    paths, counts, _ = clnp.trace(clear, pen, (10, 14, 10, 14, 17), dist, [5], 1, 4)
    assert counts.tolist() == [3] and paths[0].tolist() == [5, 1, 0, -1]
    # 3 x 3 x 3 with every move of length 10: (2, 2, 0) = 24 is two moves from 0, through (1, 1, 0) = 12 or (1, 1, 1) = 13
    full = np.full((3, 3, 3), 1500, dtype=np.int16)
    clear = clnp.clearance(full, LO, HI, 1)
    dist, _ = clnp.field(clear, pen, (10,) * 5, 0, 1)
    paths, counts, _ = clnp.trace(clear, pen, (10,) * 5, dist, [24, 26], 1, 3)
    assert counts.tolist() == [3, 3] and paths.tolist() == [[24, 12, 0], [26, 13, 0]]


def test_a_field_that_does_not_explain_itself_sets_the_flag():
    full = np.full((1, 1, 4), 1500, dtype=np.int16)
    clear = clnp.clearance(full, LO, HI, 1)
    pen = np.array([1, 1], dtype=np.uint16)
    foreign = np.array([0, 10, 25, 35], dtype=np.uint32).reshape(1, 1, 4)      # 25 is not 10 + 10
    paths, counts, stats = clnp.trace(clear, pen, (10, 14, 10, 14, 17), foreign, [3], 1, 8)
    assert counts.tolist() == [-2] and stats[4] == 1 and stats[6] == 1 and paths[0].tolist() == [3, 2] + [-1] * 6


# ---------------------------------------------------------------------------------------------- 4. a vessel
@functools.lru_cache(maxsize=None)
def helix_case():
    from cta_gan_amd.infer import centreline_penalty, centreline_steps
    vol, axis, start, end = clnp.helix_tube()
    n, h, w = vol.shape
    r = 8
    clear = clnp.clearance(vol, 500, 32767, r)
    steps = centreline_steps(1.0)
    s, e = ((p[0] * h + p[1]) * w + p[2] for p in (start, end))
    out = {}
    for name, pen in (("shaped", centreline_penalty(r)), ("flat", np.ones(r * r + 1, dtype=np.uint16))):
        dist, stats = clnp.field(clear, pen, steps, s, r)
        paths, counts, st = clnp.trace(clear, pen, steps, dist, [e], r, 4 * (n + h + w))
        assert stats.tolist() == [0] * 8 and st.tolist() == [0] * 8 and counts[0] > 80
        p = paths[0, :counts[0]][::-1].astype(np.int64)
        out[name] = np.stack([p // (h * w), (p // w) % h, p % w], axis=1)
    return vol, axis, out


def test_the_traced_path_stays_in_the_middle_of_a_helical_vessel():
    from cta_gan_amd.infer import curved_lines, smooth_centreline
    vol, axis, voxels = helix_case()
    n, h, w = vol.shape
    for window in (1, 5):
        off = clnp.axis_distance(smooth_centreline(voxels["shaped"], window), axis)
        assert off.max() <= 1.25, (window, off.max(), off.mean())      # half the radius: traced and smoothed alike
    flat = clnp.axis_distance(voxels["flat"], axis)
    assert flat.max() > 1.25, flat.max()      # a path that only counts length cuts the corners
    pts = smooth_centreline(voxels["shaped"], 5)
    lines, steps = curved_lines(n, h, w, pts, cols=21)
    got, cnt = reformat_np.reformat(vol, lines, 21, 1, "max", "trilinear")
    assert lines.shape[1] > 100 and (cnt[0, :, 10] == 1).all() and (got[0, :, 10] == 1000).all()      # the core, on every row
    assert (got[0, :, 0] == 0).all() and (got[0, :, 20] == 0).all()


def test_smoothing_and_tables():
    from cta_gan_amd.infer import centreline_penalty, centreline_steps, smooth_centreline
    assert centreline_steps(1.0) == (10, 14, 10, 14, 17) and centreline_steps(2.0) == (10, 14, 20, 22, 24)
    pen = centreline_penalty(8)
    assert pen.dtype == np.uint16 and pen.shape == (65,) and pen[0] == 64 and pen[64] == 1 and (np.diff(pen[1:].astype(int)) <= 0).all()
    assert centreline_penalty(2, far=3, near=4095).tolist() == [4095, 1026, 354, 76, 3]
    p = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [2, 1, 0], [2, 2, 0]], dtype=np.int64)
    assert np.array_equal(smooth_centreline(p, 1), p.astype(np.float64))
    s = smooth_centreline(p, 3)
    assert s.dtype == np.float64 and np.allclose(s[0], [1 / 3, 0, 0]) and np.allclose(s[2], [4 / 3, 2 / 3, 0]) and np.allclose(s[4], [2, 5 / 3, 0])


def test_predict_options():
    import predict
    base = ["--weights", "w", "--input", "i", "--output", "o"]
    o = predict.parse_args(base)
    assert o.cl is None and not o.cpr_traced
    o = predict.parse_args(base + ["--cl-start", "3,24,34", "--cl-end", "36,24,10", "--cl-end", "5,6,7", "--cl-threshold", "500",
                                   "--cl-radius", "6", "--cl-output", "pts.npy", "--aspect", "2.5"])
    assert o.cl == {"threshold": (500, 32767), "start": (3, 24, 34), "ends": [(36, 24, 10), (5, 6, 7)], "radius": 6, "aspect": 2.5}
    assert not o.cpr_traced
    o = predict.parse_args(base + ["--cl-start", "3,24,34", "--cl-end", "36,24,10", "--cl-threshold=-5,300", "--cpr-dir", "c", "--cpr-width",
                                   "21", "--cpr-angles", "2", "--reformat-sampling", "nearest"])
    assert o.cpr_traced and o.cl["threshold"] == (-5, 300) and o.cl["radius"] == 8
    assert o.cl["cpr"] == {"angles": [0.0, 90.0], "cols": 21, "depth": 1, "sampling": "nearest", "mode": "max"}
    tables, _ = predict.reformat_tables(o)
    assert tables is None      # the centreline view makes the curved reformat itself
    o = predict.parse_args(base + ["--cl-start", "3,24,34", "--cl-end", "36,24,10", "--cl-threshold", "500", "--cpr-dir", "c",
                                   "--cpr-centreline", "p.npy"])
    assert not o.cpr_traced and "cpr" not in o.cl      # a centreline file given: the reformat runs along that one
    for bad in (["--cl-start", "1,2,3"], ["--cl-end", "1,2,3"], ["--cl-threshold", "5"], ["--cl-output", "p.npy"],
                ["--cl-start", "1,2,3", "--cl-end", "1,2,4"], ["--cl-start", "1,2", "--cl-end", "1,2,4", "--cl-threshold", "5"],
                ["--cl-start", "1,2,3", "--cl-end", "1,2,-4", "--cl-threshold", "5"], ["--cl-start", "a,2,3", "--cl-end", "1,2,4", "--cl-threshold", "5"],
                ["--cl-start", "1,2,3", "--cl-end", "1,2,4", "--cl-threshold", "5,4"],
                ["--cl-start", "1,2,3", "--cl-end", "1,2,4", "--cl-threshold", "5", "--cl-radius", "33"],
                ["--cl-start", "1,2,3", "--cl-end", "1,2,4", "--cl-threshold", "5", "--aspect", "20"], ["--cpr-dir", "c"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
    for flag in ("--cl-start Z,Y,X", "--cl-end Z,Y,X", "--cl-threshold LO[,HI]", "--cl-radius R", "--cl-output pts.npy"):
        assert flag in predict.__doc__ and flag in open(os.path.join(ROOT, "README.md")).read(), flag


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_that_need_no_gpu():
    from cta_gan_amd import ops
    from cta_gan_amd.infer import (SeriesTranslator, VolumeCentreline, centreline_penalty, centreline_steps, smooth_centreline)
    assert ops.CENTRELINE_TILE == (8, 16, 32) and ops.CENTRELINE_MAX_ENDS == 64 and len(ops.CENTRELINE_STATS) == 8
    base = dict(threshold=100, start=(0, 0, 0), ends=[(3, 4, 5)])
    for kw in (dict(threshold=None), dict(threshold=(5, 4)), dict(threshold=1.5), dict(threshold=40000), dict(start=(0, 0)),
               dict(start=(4, 0, 0)), dict(start=(0.5, 0, 0)), dict(ends=[]), dict(ends=[(0, 0, 6)]), dict(ends=[(-1, 0, 0)]),
               dict(ends=[(0, 0, 0)] * 65), dict(radius=0), dict(radius=33), dict(radius=2.5), dict(aspect=0.0), dict(aspect=0.2),
               dict(aspect=16.0), dict(aspect=float("nan")), dict(penalty=np.ones(5, dtype=np.uint16)),
               dict(penalty=np.zeros(65, dtype=np.uint16)), dict(penalty=np.full(65, 5000)), dict(max_points=0), dict(max_points=True),
               dict(smooth=4), dict(smooth=0), dict(cpr=3), dict(cpr={"rows": 3}), dict(cpr={"mode": "sum"}), dict(cpr={"sampling": "cubic"}),
               dict(cpr={"pitch": 0.0}), dict(cpr={"angles": ()}), dict(rounds_per_call=0), dict(max_rounds=0), dict(max_rounds=2 ** 20 + 1)):
        with pytest.raises(ValueError):
            VolumeCentreline(4, 5, 6, **{**base, **kw})
    for shape in ((0, 5, 6), (4097, 5, 6), (4096, 4096, 128)):
        with pytest.raises(ValueError):
            VolumeCentreline(*shape, **{**base, "ends": [(0, 0, 1)]})
    view = VolumeCentreline(4, 5, 6, (100, 200), (0, 0, 1), [(3, 4, 5), (0, 0, 0)], radius=3, aspect=2.5, max_points=7, hu=True)
    assert (view.lo, view.hi, view.start, view.ends_host.tolist(), view.zq, view.fill) == (100, 200, 1, [119, 0], 1600, -1024)
    assert view.steps == centreline_steps(2.5) and np.array_equal(view.pen_host, centreline_penalty(3))
    assert view.nbytes == 10 * 120 + 2 * 10 + 4 * 2 + 8 * 1 + 4 * 4096 + 4 * 2 * 8 + 32
    assert VolumeCentreline(40, 48, 44, **base).max_points == 4 * (40 + 48 + 44)
    with pytest.raises(RuntimeError, match="exactly once"):
        view.result()      # before any slice has arrived
    for bad in (dict(radius=0), dict(radius=33), dict(radius=3, far=0), dict(radius=3, near=4096), dict(radius=3, far=1.5)):
        with pytest.raises(ValueError):
            centreline_penalty(**bad)
    for bad in (0.0, -1.0, 0.2, 26.0, float("inf")):
        with pytest.raises(ValueError):
            centreline_steps(bad)
    for bad in (dict(points=np.zeros((3, 2))), dict(points=np.zeros((0, 3))), dict(points=np.zeros((3, 3)), window=2),
                dict(points=np.zeros((3, 3)), window=0), dict(points=np.zeros((3, 3)), window=1.0)):
        with pytest.raises(ValueError):
            smooth_centreline(**bad)
    for kw in (dict(centreline={"threshold": 1, "start": (0, 0, 0)}),                      # no ends
               dict(centreline={**base, "angle": 3}),                                       # an unknown option
               dict(centreline=3)):
        with pytest.raises((ValueError, TypeError)):
            SeriesTranslator(None, **kw)
