"""GPU: the vessel centreline of the resident volume (csrc/centreline.hip through ops.centreline_clearance / centreline_field /
centreline_trace, cta_gan_amd/infer.py: VolumeCentreline, centreline_volume, SeriesTranslator(centreline=...)) against the numpy
restatement tests/centreline_np.py.  Exact integer arithmetic and a field that is a least fixed point: every comparison is
np.array_equal, never a tolerance, and stats[6] (the internal-error flag) reads 0 everywhere."""
import functools

import numpy as np
import pytest
import torch

import centreline_np as clnp
import components_np as cnp
import project_np
import reformat_np

LO, HI = cnp.LO, cnp.HI
STEPS = (10, 14, 10, 14, 17)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib, ops
    _lib.load()
    return ops


def cpu(t):
    return t.cpu().numpy()


def dev16(a):
    """A uint16 numpy array as a uint16 device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def shapes():
    from cta_gan_amd import ops
    tz, ty, tx = ops.CENTRELINE_TILE
    return [(1, 1, 1), (tz - 1, ty - 1, 37), (2 * tz + 1, 2 * ty + 1, 2 * tx + 3), (1, 3 * ty, 3 * tx), (3 * tz, 1, 5)]


def odd_shape():
    return shapes()[2]


def index(shape, z, y, x):
    return (z * shape[1] + y) * shape[2] + x


@functools.lru_cache(maxsize=None)
def blob_volume(shape):
    vol = clnp.blobs(shape, seed=shape[2] + shape[0], rmax=4.0)
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def blob_clearance(shape, r, zq):
    c = clnp.clearance(blob_volume(shape), LO, HI, r, zq)
    c.setflags(write=False)
    return c


# ---------------------------------------------------------------------------------------------- 1. clearance
@pytest.mark.parametrize("index_", range(5))
def test_clearance_equals_the_restatement(ops, index_):
    from test_components_gpu import shifted
    shape = shapes()[index_]
    vol = blob_volume(shape)
    dev = torch.from_numpy(np.array(vol)).cuda()
    for r in (1, 3, 32):
        for zq in (256, 1600):
            want = blob_clearance(shape, r, zq)
            for x in (dev, shifted(dev)):
                got = ops.centreline_clearance(x, LO, HI, r, zq)
                assert got.dtype == torch.uint16 and tuple(got.shape) == shape
                assert np.array_equal(cpu(got), want), (shape, r, zq, x is not dev)
    if shape == odd_shape():      # the test cannot pass on a volume without vessels
        assert 0.05 < (vol >= LO).mean() < 0.95 and blob_clearance(shape, 32, 256).max() > 9


def test_clearance_of_empty_and_full_volumes_and_reused_arrays(ops):
    shape = odd_shape()
    v = shape[0] * shape[1] * shape[2]
    scratch = torch.empty(v, dtype=torch.uint16, device="cuda")
    clear = torch.empty(shape, dtype=torch.uint16, device="cuda")
    for value, r, want in ((0, 5, 0), (1500, 5, 25), (1500, 32, 1024), (HI + 1, 3, 0)):
        dev = torch.full(shape, value, dtype=torch.int16, device="cuda")
        got = ops.centreline_clearance(dev, LO, HI, r, 1600, scratch=scratch, clear=clear)
        assert got is clear and (cpu(got) == want).all(), (value, r)
    with pytest.raises(RuntimeError):
        ops.centreline_clearance(dev, LO, HI, 3, scratch=clear, clear=clear)
    with pytest.raises(RuntimeError):
        ops.centreline_clearance(dev.cpu(), LO, HI, 3)
    with pytest.raises(RuntimeError):
        ops.centreline_clearance(dev, LO, HI, 33)
    with pytest.raises(RuntimeError):
        ops.centreline_clearance(dev, LO, HI, 3, zq=15)


# ---------------------------------------------------------------------------------------------- 2. the cost field
@functools.lru_cache(maxsize=None)
def blob_field(r=4):
    """(clear, pen, start, dist, stats, component labels) of the odd blob volume by the restatement: computed once and shared."""
    from cta_gan_amd.infer import centreline_penalty
    shape = odd_shape()
    clear = blob_clearance(shape, r, 256)
    lab = cnp.label(np.where(clear > 0, 1500, 0).astype(np.int16), LO, HI, 26).reshape(-1)
    roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
    big = int(roots[np.argmax(sizes)])
    members = np.flatnonzero(lab == big)
    start = int(members[members.size // 3])
    pen = centreline_penalty(r)
    dist, stats = clnp.field(clear, pen, STEPS, start, r)
    for a in (dist, stats):
        a.setflags(write=False)
    return clear, pen, start, dist, stats, lab, big


@functools.lru_cache(maxsize=None)
def snake_field(heavy):
    """The snake of the odd shape under R = 1 (clear = 1 on the snake): (clear, pen, steps, dist, stats) by the restatement, from
    voxel 0; heavy: steps 255 and pen 4095, under which the sums saturate."""
    vol = cnp.snake(odd_shape())
    clear = clnp.clearance(vol, LO, HI, 1)
    pen = np.array([4095, 4095] if heavy else [7, 3], dtype=np.uint16)
    steps = (255,) * 5 if heavy else STEPS
    dist, stats = clnp.field(clear, pen, steps, 0, 1)
    for a in (clear, dist, stats):
        a.setflags(write=False)
    return clear, pen, steps, dist, stats


def test_field_on_blobs_leaves_other_components_unreached(ops):
    clear, pen, start, dist, stats, lab, big = blob_field()
    assert int((lab == big).sum()) > 1000 and int(((lab >= 0) & (lab != big)).sum()) > 100
    assert (dist.reshape(-1)[(lab >= 0) & (lab != big)] == clnp.UNREACHED).all() and stats.tolist() == [0] * 8
    d_clear, d_pen = dev16(clear), dev16(pen)
    runs = []
    for per in (1, 16):
        got, st = ops.centreline_field(d_clear, d_pen, STEPS, start, 4, rounds_per_call=per)
        assert got.dtype == torch.uint32 and np.array_equal(cpu(got), dist) and cpu(st).tolist() == [0] * 8, per
        runs.append(ops.centreline_field.rounds)
    assert runs[0] <= runs[1] < runs[0] + 16 and runs[1] % 16 == 0
    reuse = torch.zeros(clear.shape, dtype=torch.uint32, device="cuda")
    got, st = ops.centreline_field(d_clear, d_pen, STEPS, start, 4, dist=reuse)
    assert got is reuse and np.array_equal(cpu(got), dist)
    # a start on background, and outside the volume: nothing is reached, the start is counted
    for bad in (int(np.flatnonzero(clear.reshape(-1) == 0)[0]), -1, clear.size):
        got, st = ops.centreline_field(d_clear, d_pen, STEPS, bad, 4)
        assert (cpu(got) == clnp.UNREACHED).all() and cpu(st).tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


def test_field_along_the_snake_crosses_tile_faces_hundreds_of_times(ops):
    clear, pen, steps, dist, stats = snake_field(False)
    assert int((clear > 0).sum()) > 5000 and int((dist != clnp.UNREACHED).sum()) == int((clear > 0).sum()) and stats.tolist() == [0] * 8
    d_clear, d_pen = dev16(clear), dev16(pen)
    got, st = ops.centreline_field(d_clear, d_pen, steps, 0, 1, rounds_per_call=16, max_rounds=32768)
    assert np.array_equal(cpu(got), dist) and cpu(st).tolist() == [0] * 8
    assert ops.centreline_field.rounds > 100
    got1, st1 = ops.centreline_field(d_clear, d_pen, steps, 0, 1, rounds_per_call=64, max_rounds=32768)
    assert np.array_equal(cpu(got1), dist)
    with pytest.raises(RuntimeError, match="max_rounds"):
        ops.centreline_field(d_clear, d_pen, steps, 0, 1, rounds_per_call=1, max_rounds=2)
    torch.cuda.synchronize()


def test_field_saturates_as_the_restatement_does(ops):
    clear, pen, steps, dist, stats = snake_field(True)
    assert int((dist == clnp.SAT).sum()) > 100 and int((dist < clnp.SAT).sum()) > 100 and stats.tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    got, st = ops.centreline_field(dev16(clear), dev16(pen), steps, 0, 1, max_rounds=32768)
    assert np.array_equal(cpu(got), dist) and cpu(st).tolist() == stats.tolist()


# ---------------------------------------------------------------------------------------------- 3. the trace
def test_trace_equals_the_restatement(ops):
    clear, pen, start, dist, stats, lab, big = blob_field()
    members = np.flatnonzero(lab == big)
    other = int(np.flatnonzero((lab >= 0) & (lab != big))[0])
    ends = [int(members[0]), int(members[-1]), int(members[members.size // 2]), other, int(np.flatnonzero(clear.reshape(-1) == 0)[0]),
            -3, clear.size, start]
    d_clear, d_pen, d_dist = dev16(clear), dev16(pen), torch.from_numpy(np.array(dist).view(np.int32)).cuda().view(torch.uint32)
    d_ends = torch.tensor(ends, dtype=torch.int32, device="cuda")
    longest = int(clnp.trace(clear, pen, STEPS, dist, ends, 4, 4096)[1].max())
    assert longest > 20
    for max_points in (longest + 9, longest, longest - 1, 1):
        paths, counts, st = clnp.trace(clear, pen, STEPS, dist, ends, 4, max_points)
        d_stats = torch.zeros(8, dtype=torch.int32, device="cuda")
        got, cnt = ops.centreline_trace(d_clear, d_pen, STEPS, d_dist, d_ends, 4, max_points, stats=d_stats)
        assert np.array_equal(cpu(cnt), counts) and np.array_equal(cpu(got), paths), max_points
        assert cpu(d_stats).tolist() == st.tolist() and st[6] == 0
        assert counts[3:7].tolist() == [0, 0, 0, 0] and counts[7] == 1      # another component, background, outside, the start
    assert (counts[:3] == -1).all() and st[2] == 3      # max_points = 1 is too small for every true path
    got, cnt = ops.centreline_trace(d_clear, d_pen, STEPS, d_dist, d_ends[:1], 4, 64)      # a fresh stats
    assert int(cnt[0]) == clnp.trace(clear, pen, STEPS, dist, ends[:1], 4, 64)[1][0]


def test_ties_under_a_flat_penalty(ops):
    shape = (5, 9, 11)
    full = np.full(shape, 1500, dtype=np.int16)
    clear = cpu(ops.centreline_clearance(torch.from_numpy(full).cuda(), LO, HI, 1))
    assert (clear == 1).all()
    pen = np.array([1, 1], dtype=np.uint16)
    for steps in (STEPS, (10,) * 5):
        dist, _ = clnp.field(clear, pen, steps, 0, 1)
        ends = [clear.size - 1, index(shape, 4, 8, 0), index(shape, 0, 8, 10), index(shape, 2, 4, 10)]
        paths, counts, _ = clnp.trace(clear, pen, steps, dist, ends, 1, 32)
        d_dist, st = ops.centreline_field(dev16(clear), dev16(pen), steps, 0, 1)
        got, cnt = ops.centreline_trace(dev16(clear), dev16(pen), steps, d_dist, torch.tensor(ends, dtype=torch.int32, device="cuda"), 1, 32,
                                        stats=st)
        assert np.array_equal(cpu(d_dist), dist) and np.array_equal(cpu(cnt), counts) and np.array_equal(cpu(got), paths)
        assert cpu(st).tolist() == [0] * 8 and (counts > 4).all()


# ---------------------------------------------------------------------------------------------- 4. ABI refusals
def test_abi_refusals_launch_nothing(ops):
    from cta_gan_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, h, w = 3, 5, 7
    v = n * h * w
    vol = torch.from_numpy(cnp.random_field((n, h, w), 0.6, 1)).cuda()
    u16 = lambda count, value: torch.full((count,), value, dtype=torch.int16, device="cuda")
    i32 = lambda count, value: torch.full((count,), value, dtype=torch.int32, device="cuda")
    scratch, clear, pen, dist, active, marks = u16(v + 1, 777), u16(v + 1, 777), u16(10, 1), i32(v + 1, 777), i32(4, 777), i32(9, 777)
    stats, ends, paths, counts = i32(9, 777), i32(3, 0), i32(3 * 8, 777), i32(3, 777)
    P = {k: t.data_ptr() for k, t in dict(vol=vol, scratch=scratch, clear=clear, pen=pen, dist=dist, active=active, marks=marks,
                                         stats=stats, ends=ends, paths=paths, counts=counts).items()}

    def clr(vol=P["vol"], N=n, H=h, W=w, lo=LO, hi=HI, R=3, zq=256, scratch=P["scratch"], clear=P["clear"]):
        return lib.ctg_centreline_clearance(vol, N, H, W, lo, hi, R, zq, scratch, clear, st)

    def seed(clear=P["clear"], N=n, H=h, W=w, start=0, dist=P["dist"], active=P["active"], marks=P["marks"], mr=8, stats=P["stats"]):
        return lib.ctg_centreline_seed(clear, N, H, W, start, dist, active, marks, mr, stats, st)

    def relax(clear=P["clear"], N=n, H=h, W=w, pen=P["pen"], R=3, s=(10, 14, 10, 14, 17), dist=P["dist"], active=P["active"],
              marks=P["marks"], mr=8, first=0, rounds=2, stats=P["stats"]):
        return lib.ctg_centreline_relax(clear, N, H, W, pen, R, *s, dist, active, marks, mr, first, rounds, stats, st)

    def trace(clear=P["clear"], N=n, H=h, W=w, pen=P["pen"], R=3, s=(10, 14, 10, 14, 17), dist=P["dist"], ends=P["ends"], E=3, mp=8,
              paths=P["paths"], counts=P["counts"], stats=P["stats"]):
        return lib.ctg_centreline_trace(clear, N, H, W, pen, R, *s, dist, ends, E, mp, paths, counts, stats, st)

    def sat(dist=P["dist"], V=v, stats=P["stats"]):
        return lib.ctg_centreline_saturated(dist, V, stats, st)

    bad = [clr(vol=None), clr(scratch=None), clr(clear=None), clr(scratch=P["clear"]), clr(N=0), clr(H=4097), clr(W=0),
           clr(N=4096, H=4096, W=128), clr(lo=5, hi=4), clr(lo=-32769), clr(hi=32768), clr(R=0), clr(R=33), clr(zq=15), clr(zq=65536),
           clr(vol=P["vol"] + 1), clr(scratch=P["scratch"] + 1), clr(clear=P["clear"] + 1),
           seed(clear=None), seed(dist=None), seed(active=None), seed(marks=None), seed(stats=None), seed(N=0), seed(W=4097), seed(mr=0),
           seed(mr=2 ** 20 + 1), seed(clear=P["clear"] + 1), seed(dist=P["dist"] + 2), seed(active=P["active"] + 2),
           seed(marks=P["marks"] + 1), seed(stats=P["stats"] + 2),
           relax(clear=None), relax(pen=None), relax(dist=None), relax(active=None), relax(marks=None), relax(stats=None), relax(H=0),
           relax(R=0), relax(R=33), relax(s=(0, 14, 10, 14, 17)), relax(s=(10, 14, 10, 14, 256)), relax(s=(10, 14, -1, 14, 17)),
           relax(mr=0), relax(first=-1), relax(rounds=-1), relax(first=7, rounds=2), relax(first=2 ** 30, rounds=2 ** 30),
           relax(pen=P["pen"] + 1), relax(dist=P["dist"] + 2), relax(marks=P["marks"] + 2),
           trace(clear=None), trace(pen=None), trace(dist=None), trace(ends=None), trace(paths=None), trace(counts=None),
           trace(stats=None), trace(N=4097), trace(R=33), trace(s=(10, 14, 10, 0, 17)), trace(E=0), trace(E=65), trace(mp=0),
           trace(mp=2 ** 24 + 1), trace(ends=P["ends"] + 2), trace(paths=P["paths"] + 1), trace(counts=P["counts"] + 2),
           sat(dist=None), sat(stats=None), sat(V=0), sat(V=2 ** 31), sat(dist=P["dist"] + 2)]
    assert bad == [1] * len(bad), bad      # CTG_EINVAL
    torch.cuda.synchronize()
    for t, sentinel in ((scratch, 777), (clear, 777), (dist, 777), (active, 777), (marks, 777), (stats, 777), (paths, 777), (counts, 777)):
        assert int((t != sentinel).sum()) == 0      # nothing was launched
    # the same calls with everything in order succeed, and write only what is theirs
    assert clr() == 0 and seed() == 0 and relax(rounds=8) == 0 and sat() == 0 and trace() == 0
    torch.cuda.synchronize()
    want = clnp.clearance(cpu(vol), LO, HI, 3)
    assert np.array_equal(cpu(clear[:v]).view(np.uint16).reshape(n, h, w), want) and int(clear[v]) == 777 and int(scratch[v]) == 777
    assert int(dist[v]) == 777 and int(stats[8]) == 777 and int(marks[8]) == 777 and int(stats[6]) == 0


# ---------------------------------------------------------------------------------------------- 5. through the layers
def test_volume_centreline_chunks_in_any_order(ops):
    from cta_gan_amd.infer import VolumeCentreline, centreline_penalty, smooth_centreline
    clear, pen, start, dist, stats, lab, big = blob_field()
    shape = odd_shape()
    n, h, w = shape
    vol = np.array(blob_volume(shape))
    members = np.flatnonzero(lab == big)
    ends = [int(members[0]), int(members[-1])]
    zyx = lambda i: (i // (h * w), (i // w) % h, i % w)
    view = VolumeCentreline(n, h, w, (LO, HI), zyx(start), [zyx(e) for e in ends], radius=4, max_points=300, smooth=3, clearance=True)
    dev = torch.from_numpy(vol).cuda()
    order = np.random.RandomState(3).permutation(n)
    for z in order[:-1]:
        view.update(dev[z:z + 1], int(z))
    with pytest.raises(RuntimeError, match="exactly once"):
        view.result()
    view.update(dev[order[-1]:order[-1] + 1], int(order[-1]))
    paths, counts, st = clnp.trace(clear, pen, STEPS, dist, ends, 4, 300)
    for _ in range(2):
        out = view.result()
        assert np.array_equal(cpu(out["clearance"]), clear) and np.array_equal(cpu(out["paths"]), paths)
        assert np.array_equal(cpu(out["counts"]), counts) and cpu(out["stats"]).tolist() == [0] * 8 and "cpr" not in out
        for e in range(2):
            p = paths[e, :counts[e]][::-1].astype(np.int64)
            want = smooth_centreline(np.stack(zyx(p), axis=1), 3)
            assert out["points"][e].dtype == torch.float64 and np.array_equal(cpu(out["points"][e]), want)
    # a start on background, an end in another component, a path that does not fit
    bg = zyx(int(np.flatnonzero(clear.reshape(-1) == 0)[0]))
    other = zyx(int(np.flatnonzero((lab >= 0) & (lab != big))[0]))
    for kw, exc in ((dict(start=bg), ValueError), (dict(ends=[zyx(ends[0]), other]), ValueError), (dict(max_points=3), ValueError)):
        args = {"start": zyx(start), "ends": [zyx(ends[0])], "radius": 4, **kw}
        bad = VolumeCentreline(n, h, w, (LO, HI), **args)
        bad.update(dev, 0)
        with pytest.raises(exc):
            bad.result()


def test_the_helix_end_to_end_with_its_curved_reformat(ops):
    from cta_gan_amd.infer import centreline_penalty, centreline_steps, centreline_volume, curved_lines, smooth_centreline
    vol, axis, start, end = clnp.helix_tube()
    n, h, w = vol.shape
    cpr = dict(angles=(0.0, 90.0), cols=21, sampling="trilinear")
    out = centreline_volume(vol, 500, start, [end], batch=16, cpr=cpr, wc=500.0, ww=1000.0)
    assert isinstance(out["paths"], np.ndarray) and out["clearance"] is None and out["stats"].tolist() == [0] * 8
    clear = clnp.clearance(vol, 500, 32767, 8)
    pen, steps = centreline_penalty(8), centreline_steps(1.0)
    dist, _ = clnp.field(clear, pen, steps, (start[0] * h + start[1]) * w + start[2], 8)
    paths, counts, _ = clnp.trace(clear, pen, steps, dist, [(end[0] * h + end[1]) * w + end[2]], 8, 4 * (n + h + w))
    assert np.array_equal(out["paths"], paths) and np.array_equal(out["counts"], counts) and counts[0] > 80
    p = paths[0, :counts[0]][::-1].astype(np.int64)
    pts = smooth_centreline(np.stack([p // (h * w), (p // w) % h, p % w], axis=1), 5)
    assert len(out["points"]) == 1 and np.array_equal(out["points"][0], pts)
    assert clnp.axis_distance(out["points"][0], axis).max() <= 1.25      # half the radius of the tube
    lines, t = curved_lines(n, h, w, pts, angles=(0.0, 90.0), cols=21)
    want, _ = reformat_np.reformat(vol, lines, 21, t, "max", "trilinear")
    assert len(out["cpr"]) == 1 and np.array_equal(out["cpr"][0]["values"], want)
    assert np.array_equal(out["cpr"][0]["level"], project_np.level(want, 500.0, 1000.0, False))
    assert (want[:, :, 10] == 1000).all() and (want[0, :, 0] == 0).all()      # the core of the vessel on every row of both planes
    # a device volume stays on the device
    dev = centreline_volume(torch.from_numpy(vol).cuda(), 500, start, [end], level=False, cpr=dict(cols=21))
    assert dev["paths"].is_cuda and dev["points"][0].is_cuda and dev["cpr"][0]["level"] is None
    assert np.array_equal(cpu(dev["cpr"][0]["values"]), want[:1])


def make_generator(seed=0):
    from cta_gan_amd import synth
    from cta_gan_amd.Model.HdGan import Generator
    return synth.fill_module(Generator(1, 1), seed=seed).cuda()


def test_series_translator_centreline(ops):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator, centreline_penalty, centreline_steps, smooth_centreline
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        g = make_generator()
        vol = np.random.RandomState(7).randint(-1100, 3200, size=(7, 64, 64)).astype(np.int16)
        base_kw = dict(batch=2, project="max", slab=3)
        base = SeriesTranslator(g, **base_kw)(vol)
        off = SeriesTranslator(g, centreline=None, **base_kw)(vol)
        assert sorted(off) == sorted(base) and "centreline" not in off and np.array_equal(off["pix"], base["pix"])
        pix = base["pix"]
        n, h, w = pix.shape
        lo, r, aspect = int(np.percentile(pix, 50)), 3, 2.0
        clear = clnp.clearance(pix, lo, 32767, r, 1024)
        lab = cnp.label(np.where(clear > 0, 1500, 0).astype(np.int16), LO, HI, 26).reshape(-1)
        roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
        members = np.flatnonzero(lab == roots[np.argmax(sizes)])
        assert members.size > 100
        zyx = lambda i: (int(i // (h * w)), int((i // w) % h), int(i % w))
        start, ends = int(members[0]), [int(members[-1]), int(members[members.size // 2])]
        pen, steps = centreline_penalty(r), centreline_steps(aspect)
        dist, _ = clnp.field(clear, pen, steps, start, r)
        paths, counts, _ = clnp.trace(clear, pen, steps, dist, ends, r, 4 * (n + h + w))
        assert (counts > 1).all()
        tr = SeriesTranslator(g, centreline=dict(threshold=lo, start=zyx(start), ends=[zyx(e) for e in ends], radius=r, aspect=aspect,
                                                 clearance=True, cpr=dict(cols=9)), **base_kw)
        for _ in range(2):      # (a second call on the same object)
            o = tr(vol)
            assert np.array_equal(o["pix"], base["pix"])
            for a in base["projections"]:
                assert np.array_equal(o["projections"][a]["values"], base["projections"][a]["values"])
            cl = o["centreline"]
            assert np.array_equal(cl["clearance"], clear) and np.array_equal(cl["paths"], paths) and np.array_equal(cl["counts"], counts)
            assert cl["stats"].tolist() == [0] * 8 and len(cl["points"]) == 2 and len(cl["cpr"]) == 2
            for e in range(2):
                p = paths[e, :counts[e]][::-1].astype(np.int64)
                assert np.array_equal(cl["points"][e], smooth_centreline(np.stack([p // (h * w), (p // w) % h, p % w], axis=1), 5))
                assert cl["cpr"][e]["values"].shape[2] == 9 and cl["cpr"][e]["level"].shape == cl["cpr"][e]["values"].shape
    finally:
        nets.set_default_compute_dtype(torch.float32)
