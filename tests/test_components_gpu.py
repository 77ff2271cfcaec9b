"""GPU: connected components of the resident volume (csrc/components.hip through ops.components_label / components_select /
components_apply, cta_gan_amd/infer.py: VolumeComponents, components_volume, SeriesTranslator(components=...), predict.py
--cc-output) against the numpy restatement tests/components_np.py.  Exact integer arithmetic and labels defined as the smallest
linear index of a component: every comparison is np.array_equal, never a tolerance, and stats[6] (the internal-error flag) reads 0
everywhere."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import components_np as cnp
import project_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = cnp.LO, cnp.HI
CONNS = (6, 18, 26)
DENSITY = {6: 0.31, 18: 0.14, 26: 0.10}      # where the components are many and tortuous

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


def shifted(dev):
    """The same planes as a view behind one more plane: with odd H W the base pointer itself is only 2-byte aligned."""
    v = torch.cat([dev[:1], dev])[1:]
    hw = dev.shape[1] * dev.shape[2]
    assert v.is_contiguous() and v.data_ptr() == v._base.data_ptr() + 2 * hw
    return v


def tile():
    from cta_gan_amd import ops
    return ops.COMPONENTS_TILE


def shapes():
    tz, ty, tx = tile()
    return [(1, 1, 1), (tz - 1, ty - 1, 37), (2 * tz + 1, 2 * ty + 1, 2 * tx + 3), (1, 3 * ty, 3 * tx), (3 * tz, 1, 5)]


def odd_shape():
    return shapes()[2]


@functools.lru_cache(maxsize=None)
def field(shape, density, seed=0):
    return cnp.random_field(shape, density, seed + int(density * 100) + shape[2])


@functools.lru_cache(maxsize=None)
def labelled(kind, shape, arg, conn):
    """(vol, labels, sizes) of a test volume by the restatement: computed once and shared."""
    vol = field(shape, arg) if kind == "field" else (cnp.snake(shape, arg) if kind == "snake" else cnp.checkerboard(shape))
    lab = cnp.label(vol, LO, HI, conn)
    for a in (vol, lab):
        a.setflags(write=False)
    return vol, lab, cnp.sizes(lab)


def run(ops, dev, conn, lo=LO, hi=HI, **select):
    """One pass through the three ops on a device volume -> numpy (labels, sizes, keep, top, stats)."""
    labels, stats = ops.components_label(dev, lo, hi, conn)
    sizes, keep, top = ops.components_select(labels, stats, **select)
    return cpu(labels), cpu(sizes), cpu(keep), cpu(top), cpu(stats)


def check_labelling(ops, kind, shape, arg, conn):
    vol, lab, size = labelled(kind, shape, arg, conn)
    dev = torch.from_numpy(np.array(vol)).cuda()
    for x in (dev, shifted(dev)):
        labels, sizes, keep, top, stats = run(ops, x, conn)
        assert labels.dtype == np.int32 and labels.shape == vol.shape
        assert np.array_equal(labels, lab), (kind, shape, arg, conn, x is not dev)
        assert np.array_equal(sizes, size), (kind, shape, arg, conn)
        nroots = int((size > 0).sum())
        assert stats.tolist() == [int((lab >= 0).sum()), nroots, nroots, nroots, int((lab >= 0).sum()), 0, 0, 0]
        assert np.array_equal(keep, (size > 0).astype(np.uint8))
    return lab, size


# ---------------------------------------------------------------------------------------------- 1. random fields
@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("index", range(5))
def test_random_fields_equal_the_restatement(ops, index, conn):
    shape = shapes()[index]
    lab, size = check_labelling(ops, "field", shape, DENSITY[conn], conn)
    if shape == odd_shape():      # the test cannot pass on a volume of a few blobs
        assert int((size > 0).sum()) > 300 and int(size.max()) > 40


@pytest.mark.parametrize("density", [0.0, 0.5, 1.0])
def test_empty_giant_and_full_volumes(ops, density):
    for conn in CONNS:
        lab, size = check_labelling(ops, "field", odd_shape(), density, conn)
        if density == 1.0:
            assert int(size.reshape(-1)[0]) == lab.size and int((size > 0).sum()) == 1
        if density == 0.0:
            assert int((lab >= 0).sum()) == 0


# ---------------------------------------------------------------------------------------------- 2. the snake
@pytest.mark.parametrize("shape_index", [2, 1])
def test_snake_is_one_component_and_a_cut_gives_two(ops, shape_index):
    shape = shapes()[shape_index]
    cut = (2 * (shape[0] // 4), 2 * (shape[1] // 4), shape[2] // 2)      # the middle of a filled row
    for conn in CONNS:
        lab, size = check_labelling(ops, "snake", shape, None, conn)
        assert int((size > 0).sum()) == 1 and lab.max() == 0
        lab, size = check_labelling(ops, "snake", shape, cut, conn)
        assert int((size > 0).sum()) == 2


# ---------------------------------------------------------------------------------------------- 3. adjacency across tile borders
def test_two_voxels_across_faces_edges_and_corners_of_tiles(ops):
    """Two single voxels b and a = b + offset for all 26 offsets, b at anchors chosen so that the contact crosses a tile face, a
    tile edge and the tile corner in x, y and z (and lies inside one tile): c = 6 / 18 / 26 join exactly face / face + edge / all."""
    tz, ty, tx = tile()
    shape = (2 * tz, 2 * ty, 2 * tx)
    anchors = [(tz, ty, tx), (tz - 1, ty - 1, tx - 1), (tz, 5, 5), (2, ty, 5), (2, 5, tx), (tz, ty, 5), (tz, 5, tx), (2, ty, tx),
               (tz - 1, 5, 5), (2, ty - 1, 5), (2, 5, tx - 1), (2, 5, 5)]
    offs = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
    h, w = shape[1], shape[2]
    dev = torch.zeros(shape, dtype=torch.int16, device="cuda")
    for conn in CONNS:
        limit = {6: 1, 18: 2, 26: 3}[conn]
        got = []
        for b in anchors:
            for o in offs:
                a = tuple(p + d for p, d in zip(b, o))
                dev.zero_()
                dev[b] = 1500
                dev[a] = 1500
                labels, stats = ops.components_label(dev, LO, HI, conn)
                got.append(torch.stack([labels[a], labels[b], stats[0], stats[6]]))
        got = cpu(torch.stack(got)).reshape(len(anchors), len(offs), 4)
        for i, b in enumerate(anchors):
            for j, o in enumerate(offs):
                a = tuple(p + d for p, d in zip(b, o))
                ia, ib = (a[0] * h + a[1]) * w + a[2], (b[0] * h + b[1]) * w + b[2]
                joined = sum(abs(d) for d in o) <= limit
                want = [min(ia, ib)] * 2 if joined else [ia, ib]
                assert got[i, j].tolist() == want + [2, 0], (conn, b, o)


def test_checkerboard(ops):
    shape = (4, 6, 10)
    for conn, count in ((6, 120), (18, 1), (26, 1)):
        lab, size = check_labelling(ops, "board", shape, None, conn)
        assert int((size > 0).sum()) == count
    # half of a larger volume as components of one voxel: more roots per chunk than the size kernel's LDS table holds
    lab, size = check_labelling(ops, "board", odd_shape(), None, 6)
    assert int((size > 0).sum()) == (lab.size + 1) // 2 and int(size.max()) == 1


# ---------------------------------------------------------------------------------------------- 4. selection
def check_selection(ops, dev, lab, conn, **select):
    labels, sizes, keep, top, stats = run(ops, dev, conn, **select)
    k, t, s = cnp.select(lab, **select)
    assert np.array_equal(labels, lab)
    assert np.array_equal(keep, k), select
    assert top.shape == t.shape and np.array_equal(top, t), (select, top.tolist(), t.tolist())
    assert stats.tolist() == s.tolist(), (select, stats.tolist(), s.tolist())
    return k, t, s


def test_selection_by_size_rank_and_seed(ops):
    conn, shape = 6, odd_shape()
    vol, lab, size = labelled("field", shape, DENSITY[conn], conn)
    dev = torch.from_numpy(np.array(vol)).cuda()
    counts = np.sort(size[size > 0])[::-1]
    third = int(counts[2])
    assert counts.size > 300 and third > 3
    for m in (third - 1, third, third + 1):      # min_voxels at, one below and one above an existing size
        k, t, s = check_selection(ops, dev, lab, conn, min_voxels=m)
        assert s[2] == int((counts >= m).sum())
    for largest in (1, 3, 64):
        k, t, s = check_selection(ops, dev, lab, conn, largest=largest, ntop=64)
        assert s[3] == largest and (t[largest:] == (-1, 0)).all() and (t[:largest, 0] >= 0).all()
    # more than the number of candidates: everything that passes min_voxels, the rows beyond are (-1, 0)
    k, t, s = check_selection(ops, dev, lab, conn, min_voxels=third, largest=64, ntop=64)
    assert 3 <= s[2] == s[3] < 64 and (t[s[3]:] == (-1, 0)).all()
    check_selection(ops, dev, lab, conn, min_voxels=int(counts[0]) + 1, largest=5, ntop=8)      # nothing passes
    check_selection(ops, dev, lab, conn, ntop=0)
    check_selection(ops, dev, lab, conn, largest=2, ntop=8)      # top has more rows than are kept
    # seeds: on two components, twice on one, on background, combined with largest and min_voxels
    flat = lab.reshape(-1)
    roots = np.flatnonzero(size.reshape(-1) > 0)
    big = int(np.flatnonzero(size.reshape(-1) == counts[0])[0])
    big_members = np.flatnonzero(flat == big)
    small = int(roots[np.argmin(size.reshape(-1)[roots])])
    bg = np.flatnonzero(flat < 0)
    seeds = np.array([big_members[-1], big_members[len(big_members) // 2], small, bg[0], bg[-1]], dtype=np.int32)
    for extra in ({}, {"largest": 1}, {"min_voxels": 2}, {"largest": 64, "ntop": 3}):
        k, t, s = check_seeded(ops, dev, lab, conn, seeds, **extra)
        assert s[5] == 2
    k, t, s = check_seeded(ops, dev, lab, conn, seeds[:2])
    assert s[2] == 1 and s[4] == counts[0] and t[0].tolist() == [big, int(counts[0])]
    k, t, s = check_seeded(ops, dev, lab, conn, seeds[3:])      # only background seeds: nothing is kept
    assert s[2] == 0 and s[5] == 2 and int(k.sum()) == 0


def check_seeded(ops, dev, lab, conn, seeds, **select):
    labels, sizes, keep, top, stats = run(ops, dev, conn, seeds=torch.from_numpy(np.asarray(seeds, dtype=np.int32)).cuda(), **select)
    k, t, s = cnp.select(lab, seeds=list(seeds), **select)
    assert np.array_equal(keep, k) and np.array_equal(top, t) and stats.tolist() == s.tolist(), (select, stats.tolist(), s.tolist())
    return k, t, s


def test_equal_sizes_the_smaller_root_wins(ops):
    tz, ty, tx = tile()
    vol = np.zeros((tz + 1, ty + 1, tx + 3), dtype=np.int16)
    # five twins of 4 voxels along x, two of them across the tile face in x
    for z, y, x in [(0, 0, 3), (0, 5, tx - 2), (2, 3, 7), (tz, ty, tx - 1), (1, ty - 1, 20)]:
        vol[z, y, x:x + 4] = 1500
    vol[3, 9, 9:14] = 1500                 # one bigger, and two smaller
    vol[1, 8, 1:3] = 1500
    vol[tz, 2, 2] = 1500
    lab = cnp.label(vol, LO, HI, 26)
    assert np.sort(cnp.sizes(lab)[cnp.sizes(lab) > 0]).tolist() == [1, 2, 4, 4, 4, 4, 4, 5]
    dev = torch.from_numpy(vol).cuda()
    for largest in (1, 2, 3, 4, 5, 6):
        k, t, s = check_selection(ops, dev, lab, 26, largest=largest, ntop=8)
        fours = t[1:largest, 0]
        assert t[0, 1] == 5 and (np.diff(fours) > 0).all() and (t[1:min(largest, 6), 1] == 4).all()
    check_selection(ops, dev, lab, 26, min_voxels=4, ntop=8)


# ---------------------------------------------------------------------------------------------- 5. apply
def test_apply_modes_levels_and_sentinels(ops):
    from cta_gan_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    conn, shape = 26, odd_shape()
    vol, lab, size = labelled("field", shape, DENSITY[conn], conn)
    v = vol.size
    keep, _, _ = cnp.select(lab, min_voxels=5)
    assert 0 < int(keep.sum()) < int((size > 0).sum())
    d_lab, d_keep = torch.from_numpy(np.array(lab)).cuda(), torch.from_numpy(keep).cuda()
    pad = 19
    for off in (0, 1, 3, 8):      # the volume behind `off` extra voxels: every alignment class of the 16-byte body
        buf = torch.zeros(v + off + pad, dtype=torch.int16, device="cuda")
        buf[off:off + v] = torch.from_numpy(np.array(vol)).cuda().reshape(-1)
        for background, fill, hu, (wc, ww) in ((0, 0, 0, (50.0, 400.0)), (1, 0, 1, (150.0, 300.0)), (0, -1024, 1, (50.0, 400.0)),
                                               (1, -1024, 0, (300.0, 1500.0))):
            want = cnp.apply(vol, lab, keep, bool(background), fill)
            want_level = project_np.level(want, wc, ww, bool(hu))
            for want_out, want_lvl in ((True, True), (True, False), (False, True)):
                out = torch.full((v + 2 * pad + off,), 12345, dtype=torch.int16, device="cuda")
                lvl = torch.full((v + 2 * pad + off,), 123, dtype=torch.uint8, device="cuda")
                r = lib.ctg_components_apply(buf.data_ptr() + 2 * off, d_lab.data_ptr(), d_keep.data_ptr(), v, background, fill, wc, ww, hu,
                                             out.data_ptr() + 2 * (pad + off) if want_out else None,
                                             lvl.data_ptr() + pad + off if want_lvl else None, st)
                assert r == 0
                o, l = cpu(out), cpu(lvl)
                body = slice(pad + off, pad + off + v)
                if want_out:
                    assert np.array_equal(o[body].reshape(shape), want), (off, background, fill)
                if want_lvl:
                    assert np.array_equal(l[body].reshape(shape), want_level), (off, background, fill, hu)
                assert (o[:pad + off] == 12345).all() and (o[pad + off + v:] == 12345).all()
                assert (l[:pad + off] == 123).all() and (l[pad + off + v:] == 123).all()
                if not want_out:
                    assert (o == 12345).all()
                if not want_lvl:
                    assert (l == 123).all()
    values, level = ops.components_apply(torch.from_numpy(np.array(vol)).cuda(), d_lab, d_keep, background=True, fill=-7, hu=True)
    want = cnp.apply(vol, lab, keep, True, -7)
    assert np.array_equal(cpu(values), want) and np.array_equal(cpu(level), project_np.level(want, 50.0, 400.0, True))
    with pytest.raises(RuntimeError):
        ops.components_apply(torch.from_numpy(np.array(vol)).cuda(), d_lab, d_keep, want_values=False, want_level=False)


# ---------------------------------------------------------------------------------------------- 6. determinism
def test_two_runs_give_identical_bits(ops):
    shape = odd_shape()
    for kind, arg, conn in (("snake", None, 26), ("field", DENSITY[6], 6)):
        vol, lab, size = labelled(kind, shape, arg, conn)
        dev = torch.from_numpy(np.array(vol)).cuda()
        runs = []
        for _ in range(2):
            labels, stats = ops.components_label(dev, LO, HI, conn)
            sizes, keep, top = ops.components_select(labels, stats, min_voxels=2, largest=7, ntop=9)
            values, level = ops.components_apply(dev, labels, keep)
            runs.append([cpu(t) for t in (labels, stats, sizes, keep, top, values, level)])
        for a, b in zip(*runs):
            assert np.array_equal(a, b)
        assert runs[0][1][6] == 0


# ---------------------------------------------------------------------------------------------- 7. ABI refusals
def test_abi_refusals_launch_nothing(ops):
    from cta_gan_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, h, w = 3, 5, 7
    v = n * h * w
    vol = torch.from_numpy(cnp.random_field((n, h, w), 0.3, 1)).cuda()
    labels = torch.full((v + 1,), 777, dtype=torch.int32, device="cuda")
    stats = torch.full((9,), 777, dtype=torch.int32, device="cuda")
    sizes = torch.full((v + 1,), 777, dtype=torch.int32, device="cuda")
    keep = torch.full((v,), 77, dtype=torch.uint8, device="cuda")
    top = torch.full((9, 2), 777, dtype=torch.int32, device="cuda")
    seeds = torch.zeros(3, dtype=torch.int32, device="cuda")
    out = torch.full((v + 1,), 12345, dtype=torch.int16, device="cuda")
    lvl = torch.full((v,), 123, dtype=torch.uint8, device="cuda")
    P = {k: t.data_ptr() for k, t in dict(vol=vol, labels=labels, stats=stats, sizes=sizes, keep=keep, top=top, seeds=seeds, out=out,
                                         lvl=lvl).items()}

    def label(vol=P["vol"], N=n, H=h, W=w, lo=LO, hi=HI, conn=26, labels=P["labels"], stats=P["stats"]):
        return lib.ctg_components_label(vol, N, H, W, lo, hi, conn, labels, stats, st)

    def select(labels=P["labels"], V=v, m=1, seeds=None, S=0, largest=0, ntop=8, sizes=P["sizes"], keep=P["keep"], top=P["top"],
               stats=P["stats"]):
        return lib.ctg_components_select(labels, V, m, seeds, S, largest, ntop, sizes, keep, top, stats, st)

    def apply(vol=P["vol"], labels=P["labels"], keep=P["keep"], V=v, background=0, fill=0, out=P["out"], lvl=P["lvl"]):
        return lib.ctg_components_apply(vol, labels, keep, V, background, fill, 50.0, 400.0, 0, out, lvl, st)

    bad = [label(vol=None), label(labels=None), label(stats=None), label(N=0), label(H=0), label(W=0), label(N=4097), label(H=4097),
           label(W=4097), label(N=4096, H=4096, W=128), label(lo=5, hi=4), label(lo=-32769), label(hi=32768), label(conn=4),
           label(conn=8), label(conn=0), label(vol=P["vol"] + 1), label(labels=P["labels"] + 2), label(stats=P["stats"] + 1),
           select(labels=None), select(sizes=None), select(keep=None), select(stats=None), select(V=0), select(V=2 ** 31),
           select(m=0), select(S=-1), select(S=2, seeds=None), select(largest=-1), select(largest=65), select(ntop=-1),
           select(ntop=65), select(ntop=3, top=None), select(labels=P["labels"] + 2), select(sizes=P["sizes"] + 1),
           select(seeds=P["seeds"] + 2, S=1), select(top=P["top"] + 2), select(stats=P["stats"] + 2),
           apply(vol=None), apply(labels=None), apply(keep=None), apply(out=None, lvl=None), apply(V=0), apply(V=2 ** 31),
           apply(background=2), apply(background=-1), apply(fill=32768), apply(fill=-32769), apply(vol=P["vol"] + 1),
           apply(out=P["out"] + 1), apply(labels=P["labels"] + 2)]
    assert bad == [1] * len(bad), bad      # CTG_EINVAL
    torch.cuda.synchronize()
    for t, sentinel in ((labels, 777), (stats, 777), (sizes, 777), (keep, 77), (top, 777), (out, 12345), (lvl, 123)):
        assert int((t != sentinel).sum()) == 0      # nothing was launched
    # the same calls with everything in order succeed (ntop = 0 takes a null top; S = 0 a null seeds)
    assert label() == 0 and select() == 0 and select(ntop=0, top=None) == 0 and apply() == 0
    torch.cuda.synchronize()
    lab = cnp.label(cpu(vol), LO, HI, 26)
    assert np.array_equal(cpu(labels[:v]).reshape(n, h, w), lab) and int(labels[v]) == 777 and int(stats[8]) == 777
    assert int(sizes[v]) == 777 and int(out[v]) == 12345 and int(stats[6]) == 0


# ---------------------------------------------------------------------------------------------- 8. through the layers
def test_components_volume_and_chunks_in_any_order(ops):
    from cta_gan_amd.infer import VolumeComponents, components_volume, root_voxel
    conn, shape = 18, odd_shape()
    vol, lab, size = labelled("field", shape, DENSITY[conn], conn)
    vol = np.array(vol)
    opts = dict(connectivity=conn, min_voxels=3, largest=4, top=6, labels=True, hu=True, wc=150.0, ww=300.0)
    keep, top, stats = cnp.select(lab, min_voxels=3, largest=4, ntop=6)
    want = cnp.apply(vol, lab, keep, False, -1024)

    def check(out, conv):
        assert np.array_equal(conv(out["values"]), want) and np.array_equal(conv(out["labels"]), lab)
        assert np.array_equal(conv(out["level"]), project_np.level(want, 150.0, 300.0, True))
        assert np.array_equal(conv(out["top"]), top) and conv(out["stats"]).tolist() == stats.tolist()

    out = components_volume(vol, (LO, HI), batch=4, **opts)
    assert isinstance(out["values"], np.ndarray)
    check(out, lambda a: a)
    out = components_volume(torch.from_numpy(vol), (LO, HI), batch=5, **opts)
    assert torch.is_tensor(out["values"]) and not out["values"].is_cuda
    check(out, lambda t: t.numpy())
    out = components_volume(torch.from_numpy(vol).cuda(), (LO, HI), batch=3, **opts)
    assert out["values"].is_cuda and out["stats"].is_cuda
    check(out, cpu)
    z, y, x = root_voxel(top[0, 0], shape[1], shape[2])
    assert lab[z, y, x] == top[0, 0]
    # chunks in shuffled order, a slice missing, a second volume through the same view; despeckle, no level, no labels
    n = shape[0]
    view = VolumeComponents(*shape, (LO, HI), connectivity=conn, min_voxels=3, background=True, level=False, top=0)
    assert view.nbytes == (11 + 2) * vol.size + 32
    dev = torch.from_numpy(vol).cuda()
    order = np.random.RandomState(3).permutation(n)
    for z in order[:-1]:
        view.update(dev[z:z + 1], int(z))
    with pytest.raises(RuntimeError):
        view.result()
    view.update(dev[order[-1]:order[-1] + 1], int(order[-1]))
    k2, _, s2 = cnp.select(lab, min_voxels=3, ntop=0)
    for _ in range(2):
        res = view.result()
        assert res["level"] is None and res["labels"] is None and tuple(res["top"].shape) == (0, 2)
        assert np.array_equal(cpu(res["values"]), cnp.apply(vol, lab, k2, True, 0)) and cpu(res["stats"]).tolist() == s2.tolist()
    seed = root_voxel(top[1, 0], shape[1], shape[2])
    out = components_volume(dev, (LO, HI), connectivity=conn, seeds=[seed, (0, 0, 0)] if lab[0, 0, 0] < 0 else [seed], level=False)
    k3, t3, s3 = cnp.select(lab, seeds=[int(top[1, 0])] + ([0] if lab[0, 0, 0] < 0 else []))
    assert np.array_equal(cpu(out["values"]), cnp.apply(vol, lab, k3, False, 0)) and cpu(out["stats"]).tolist() == s3.tolist()
    with pytest.raises(RuntimeError):
        ops.components_label(torch.from_numpy(vol), LO)      # CPU tensors
    with pytest.raises(RuntimeError):
        ops.components_label(dev.int(), LO)
    with pytest.raises(RuntimeError):
        ops.components_label(dev[:, :, ::2], LO)
    with pytest.raises(RuntimeError):
        ops.components_label(dev, 5, 4)
    with pytest.raises(RuntimeError):
        ops.components_label(dev, LO, HI, 8)


def make_generator(seed=0):
    from cta_gan_amd import synth
    from cta_gan_amd.Model.HdGan import Generator
    return synth.fill_module(Generator(1, 1), seed=seed).cuda()


def synthetic_hu(n, h, w, seed):
    return np.random.RandomState(seed).randint(-1100, 3200, size=(n, h, w)).astype(np.int16)


def sub_threshold(sub):
    """A threshold on the translator's own subtraction volume that leaves a fifth of it foreground."""
    return int(np.percentile(sub, 80))


def test_series_translator_vessels(ops):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        g = make_generator()
        vol = synthetic_hu(7, 64, 64, seed=7)
        base_kw = dict(batch=2, subtract=True, project="max", slab=3)
        base = SeriesTranslator(g, **base_kw)(vol)
        # components=None: the parent's call signature, the same bits, no new key
        off = SeriesTranslator(g, components=None, **base_kw)(vol)
        assert sorted(off) == sorted(base) and "vessels" not in off
        for key in ("pix", "level", "sub", "sub_level"):
            assert np.array_equal(off[key], base[key])
        for a in base["projections"]:
            for plane in base["projections"][a]:
                assert np.array_equal(off["projections"][a][plane], base["projections"][a][plane])
        lo = sub_threshold(base["sub"])
        win = (120.0, 240.0)
        comp = dict(threshold=lo, connectivity=18, min_voxels=4, largest=6, labels=True, top=5)
        tr = SeriesTranslator(g, components=comp, components_source="sub", project_source="vessels", sub_window=win, **base_kw)
        for _ in range(2):      # (a second call on the same object)
            o = tr(vol)
            assert np.array_equal(o["pix"], base["pix"]) and np.array_equal(o["sub"], base["sub"])
            lab = cnp.label(o["sub"], lo, 32767, 18)
            keep, top, stats = cnp.select(lab, min_voxels=4, largest=6, ntop=5)
            assert 1 <= stats[3] <= 6 and stats[1] > stats[3]
            want = cnp.apply(o["sub"], lab, keep, False, -1024)
            ves = o["vessels"]
            assert np.array_equal(ves["values"], want) and np.array_equal(ves["labels"], lab)
            assert np.array_equal(ves["level"], project_np.level(want, win[0], win[1], True))
            assert np.array_equal(ves["top"], top) and ves["stats"].tolist() == stats.tolist()
            axes = dict(zip(("axial", "coronal", "sagittal"), project_np.project(want, "max", 3)))
            for a, w_ in axes.items():
                assert np.array_equal(o["projections"][a]["values"], w_), a
                assert np.array_equal(o["projections"][a]["level"], project_np.level(w_, win[0], win[1], True)), a
        # the components beside the other displays: those keep showing their own source
        o2 = SeriesTranslator(g, components=dict(threshold=1200, background=True, level=False), **base_kw)(torch.from_numpy(vol))
        assert torch.is_tensor(o2["vessels"]["values"]) and o2["vessels"]["level"] is None and o2["vessels"]["labels"] is None
        lab = cnp.label(base["pix"], 1200, 32767, 26)
        keep, _, stats = cnp.select(lab)
        assert np.array_equal(o2["vessels"]["values"].numpy(), cnp.apply(base["pix"], lab, keep, True, 0))
        assert o2["vessels"]["stats"].tolist() == stats.tolist()
        for a in base["projections"]:
            assert np.array_equal(o2["projections"][a]["values"].numpy(), base["projections"][a]["values"])
    finally:
        nets.set_default_compute_dtype(torch.float32)


def test_predict_command_line_vessels(ops, tmp_path):
    from PIL import Image
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator, root_voxel
    vol = synthetic_hu(5, 48, 40, seed=9)
    np.save(tmp_path / "series.npy", vol)
    (tmp_path / "cfg.yaml").write_text("name: HdGan\nsize: 64\ninput_nc: 1\noutput_nc: 1\n")
    nets.set_default_compute_dtype("bf16x3")      # predict.py's default
    try:
        g = make_generator(seed=3)
        torch.save(g.state_dict(), tmp_path / "g.pth")
        want = SeriesTranslator(g, batch=2, size=64, subtract=True, project="max", slab=3, project_source="vessels",
                                components=dict(threshold=(40, 3000), connectivity=6, min_voxels=3, largest=4, seeds=None, labels=True),
                                components_source="sub")(vol)
    finally:
        nets.set_default_compute_dtype(torch.float32)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "predict.py"), "--config", str(tmp_path / "cfg.yaml"), "--weights",
                        str(tmp_path / "g.pth"), "--input", str(tmp_path / "series.npy"), "--batch", "2", "--output",
                        str(tmp_path / "out.npy"), "--sub-output", str(tmp_path / "sub.npy"), "--cc-output", str(tmp_path / "vessels.npy"), "--cc-level-dir", str(tmp_path / "cclv"),
                        "--cc-threshold", "40,3000", "--cc-connectivity", "6", "--cc-min-voxels", "3", "--cc-largest", "4", "--cc-source",
                        "sub", "--cc-labels", str(tmp_path / "labels.npy"), "--mip-dir", str(tmp_path / "mip"), "--mip-source", "vessels",
                        "--slab", "3"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ves = want["vessels"]
    assert ves["stats"][3] >= 1
    assert np.array_equal(np.load(tmp_path / "out.npy"), want["pix"])
    assert np.array_equal(np.load(tmp_path / "vessels.npy"), ves["values"])
    assert np.array_equal(np.load(tmp_path / "labels.npy"), ves["labels"])
    for i in range(5):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "cclv" / ("%06d.png" % i))), ves["level"][i])
    npz = np.load(tmp_path / "components.npz")
    assert np.array_equal(npz["top"], ves["top"]) and np.array_equal(npz["stats"], ves["stats"])
    kept = int(ves["stats"][3])
    zyx = np.stack(root_voxel(ves["top"][:kept, 0], 48, 40), axis=1)
    assert np.array_equal(npz["roots_zyx"][:kept], zyx) and (npz["roots_zyx"][kept:] == -1).all()
    line = [l for l in r.stdout.splitlines() if l.startswith("components:")]
    assert len(line) == 1 and "%d found" % ves["stats"][1] in line[0] and "%d kept" % kept in line[0] \
        and "%d voxels" % ves["stats"][4] in line[0]
    mip = np.load(tmp_path / "mip" / "projections.npz")
    assert np.array_equal(mip["axial"], project_np.project(ves["values"], "max", 3)[0])
