"""GPU: the sliding thin-slab projections (csrc/project_slabs.hip through ops.project_slabs_inplane /
ops.project_accumulate_sliding, cta_gan_amd/infer.py: SeriesSlabs, slab_volume, SeriesTranslator(slabs=...), predict.py
--sts-dir) against the numpy restatement tests/slabs_np.py.  Exact integer arithmetic: every comparison is np.array_equal,
never a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import project_np
import slabs_np
from test_project_gpu import IDENTITY, make_generator, planted, synthetic_hu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["max", "min", "mean"]
INPLANE = ["coronal", "sagittal"]
WINDOWS = [(50.0, 400.0, False), (50.0, 400.0, True), (300.0, 1500.0, False), (300.0, 1500.0, True)]

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


def extent(shape, axis):
    return shape[slabs_np.AXIS[axis]]


def outputs(shape, axis, thick, step, values=12345, level=0xA5):
    """Sentinel-filled (values, level) of a volume of `shape` along an in-plane axis."""
    n, h, w = shape
    j = len(slabs_np.windows(extent(shape, axis), thick, step))
    size = (j, n, w if axis == "coronal" else h)
    return (torch.full(size, values, dtype=torch.int16, device="cuda"), torch.full(size, level, dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------------------------------------- 1. in-plane, one call
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 37, 53), (5, 64, 48), (4, 19, 515), (2, 9, 1032)]
PAIRS = [(1, 1), (3, 1), (3, 2), (4, 2), (5, 5), (17, 5)]      # (17, 5): taller than a 16-row band


def pairs_for(shape):
    w = shape[2]
    extra = [(9, 4)] if w in (515, 1032) else []      # slabs that straddle the 512-pixel segment boundary
    extra += [(600, 64)] if w == 1032 else []         # a slab wider than a segment
    return PAIRS + extra + [(max(shape) + 3, 2)]      # thick >= the axis: one slab


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_inplane_one_call_equals_numpy(ops, shape):
    k, h, w = shape
    vol = planted(k, h, w, seed=k * 1000 + w)
    dev = torch.from_numpy(vol).cuda()
    # the same slices as a view behind one more plane: with odd H W the base pointer itself is only 2-byte aligned
    shifted = torch.cat([dev[:1], dev])[1:]
    assert shifted.is_contiguous() and shifted.data_ptr() == shifted._base.data_ptr() + 2 * h * w
    for axis in INPLANE:
        for thick, step in pairs_for(shape):
            for mode in MODES:
                want = slabs_np.slabs(vol, mode, thick, step, axis)
                if thick > max(shape):
                    assert want.shape[0] == 1
                levels = [project_np.level(want, wc, ww, hu) for wc, ww, hu in WINDOWS]
                for i, pix in enumerate((dev, shifted)):
                    for (wc, ww, hu), lvl in zip(WINDOWS, levels):
                        values, level = outputs(shape, axis, thick, step)
                        assert tuple(values.shape) == want.shape
                        ops.project_slabs_inplane(pix, 0, axis, thick, step, mode, values=values, level=level, wc=wc, ww=ww, hu=hu)
                        assert np.array_equal(cpu(values), want), (axis, thick, step, mode, i)
                        assert np.array_equal(cpu(level), lvl), (axis, thick, step, mode, i, wc, ww, hu)


# ---------------------------------------------------------------------------------------------- 2. in-plane, chunk rows only
@pytest.fixture(scope="module")
def volume7():
    return planted(7, 64, 64, seed=77)


@pytest.mark.parametrize("axis", INPLANE)
@pytest.mark.parametrize("mode", MODES)
def test_inplane_writes_the_chunk_s_rows_and_nothing_else(ops, volume7, axis, mode):
    dev = torch.from_numpy(volume7).cuda()
    thick, step = 5, 3
    want = slabs_np.slabs(volume7, mode, thick, step, axis)
    want_level = project_np.level(want, 50.0, 400.0)
    values, level = outputs(volume7.shape, axis, thick, step)
    ops.project_slabs_inplane(dev[2:4], 2, axis, thick, step, mode, values=values, level=level)
    v, l = cpu(values), cpu(level)
    assert np.array_equal(v[:, 2:4], want[:, 2:4]) and np.array_equal(l[:, 2:4], want_level[:, 2:4])
    for rows in (slice(0, 2), slice(4, 7)):      # the sentinels, in every plane
        assert (v[:, rows] == 12345).all() and (l[:, rows] == 0xA5).all()
    # all chunks, out of order
    values, level = outputs(volume7.shape, axis, thick, step)
    v_only, _ = outputs(volume7.shape, axis, thick, step)
    _, l_only = outputs(volume7.shape, axis, thick, step)
    for s in (4, 0, 6, 2):
        ops.project_slabs_inplane(dev[s:s + 2], s, axis, thick, step, mode, values=values, level=level)
        ops.project_slabs_inplane(dev[s:s + 2], s, axis, thick, step, mode, values=v_only)
        ops.project_slabs_inplane(dev[s:s + 2], s, axis, thick, step, mode, level=l_only)
    assert np.array_equal(cpu(values), want) and np.array_equal(cpu(level), want_level)
    assert torch.equal(v_only, values) and torch.equal(l_only, level)


# ---------------------------------------------------------------------------------------------- 3. axial sliding
AXIAL_PAIRS = [(3, 1), (3, 2), (4, 3), (1, 1), (100, 7)]


def acc_np(vol, mode, thick, step):
    """The int32 accumulators after the whole volume: the sums themselves for "mean"."""
    v = vol.astype(np.int64)
    red = {"max": np.max, "min": np.min, "mean": np.sum}[mode]
    return np.stack([red(v[a:b], axis=0) for a, b in slabs_np.windows(v.shape[0], thick, step)]).astype(np.int32)


def feed_axial(ops, dev, mode, thick, step, starts, chunk):
    n, h, w = dev.shape
    j = len(slabs_np.windows(n, thick, step))
    acc = torch.full((j, h, w), IDENTITY["sum" if mode == "mean" else mode], dtype=torch.int32, device="cuda")
    for s in starts:
        ops.project_accumulate_sliding(dev[s:s + chunk], s, n, thick, step, mode, acc)
    return acc


@pytest.mark.parametrize("mode", MODES)
def test_axial_sliding_chunks_in_any_order(ops, volume7, mode):
    dev = torch.from_numpy(volume7).cuda()
    for thick, step in AXIAL_PAIRS:
        want = acc_np(volume7, mode, thick, step)
        for starts, chunk in (((0, 2, 4, 6), 2), ((4, 0, 6, 2), 2), ((0,), 7)):
            acc = feed_axial(ops, dev, mode, thick, step, starts, chunk)
            assert np.array_equal(cpu(acc), want), (thick, step, starts)
        # finished: the short last slab's own divisor
        wins = slabs_np.windows(7, thick, step)
        values, level = ops.project_finish(acc, mode, min(thick, 7), wins[-1][1] - wins[-1][0], wc=300.0, ww=1500.0, hu=True)
        final = slabs_np.slabs(volume7, mode, thick, step, "axial")
        assert np.array_equal(cpu(values), final), (thick, step)
        assert np.array_equal(cpu(level), project_np.level(final, 300.0, 1500.0, True)), (thick, step)
    # without overlap: ops.project_accumulate's accumulator, bit for bit
    for thick in (3, 1, 100):
        acc = feed_axial(ops, dev, mode, thick, thick, (4, 0, 6, 2), 2)
        old = torch.full(acc.shape, IDENTITY["sum" if mode == "mean" else mode], dtype=torch.int32, device="cuda")
        for s in (0, 2, 4, 6):
            ops.project_accumulate(dev[s:s + 2], s, min(thick, 7), mode, axial=old)
        assert torch.equal(acc, old), thick


@pytest.mark.parametrize("mode", MODES)
def test_axial_sliding_unaligned_rows(ops, mode):
    vol = planted(4, 19, 515, seed=4515)
    dev = torch.from_numpy(vol).cuda()
    shifted = torch.cat([dev[:1], dev])[1:]
    for thick, step in ((3, 1), (3, 2), (4, 4)):
        want = acc_np(vol, mode, thick, step)
        for pix in (dev, shifted):
            for starts, chunk in (((0,), 4), ((3, 0), 3)):
                assert np.array_equal(cpu(feed_axial(ops, pix, mode, thick, step, starts, chunk)), want), (thick, step, starts)


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_slab_refusals(ops):
    from cta_gan_amd import _lib
    pix = torch.zeros((2, 8, 8), dtype=torch.int16)
    vals = torch.full((3, 2, 8), 12345, dtype=torch.int16)      # thick 4, step 2 along 8: 3 slabs
    lvl = torch.full((3, 2, 8), 0xA5, dtype=torch.uint8)
    acc = torch.full((1, 8, 8), 77, dtype=torch.int32)          # thick 2 = step of 2 slices: 1 slab

    def inplane(p=None, n0=0, axis="coronal", thick=4, step=2, mode="max", values=None, level=None):
        ops.project_slabs_inplane(pix.cuda() if p is None else p, n0, axis, thick, step, mode,
                                  values=vals.cuda() if values is None else values, level=level)

    def sliding(p=None, n0=0, n=2, thick=2, step=2, mode="max", axial=None):
        ops.project_accumulate_sliding(pix.cuda() if p is None else p, n0, n, thick, step, mode, acc.cuda() if axial is None else axial)

    inplane()
    sliding()
    bad_inplane = [dict(p=pix), dict(values=vals), dict(p=pix.cuda().float()), dict(values=vals.cuda().int()),
                   dict(level=lvl.cuda().short()), dict(level=torch.zeros((3, 2, 9), dtype=torch.uint8, device="cuda")),
                   dict(values=torch.zeros((3, 2, 16), dtype=torch.int16, device="cuda")[:, :, ::2]),
                   dict(values=torch.zeros((2, 2, 8), dtype=torch.int16, device="cuda")),      # 3 slabs needed
                   dict(values=torch.zeros((3, 2, 7), dtype=torch.int16, device="cuda")),
                   dict(values=torch.zeros((3, 1, 8), dtype=torch.int16, device="cuda")),      # a chunk of 2 in a volume of 1
                   dict(n0=1), dict(n0=-1), dict(step=0), dict(step=5), dict(thick=0), dict(mode="median"), dict(axis="axial"),
                   dict(axis=2)]
    for kw in bad_inplane:
        with pytest.raises(RuntimeError):
            inplane(**kw)
    with pytest.raises(RuntimeError):
        ops.project_slabs_inplane(pix.cuda(), 0, "coronal", 4, 2, "max")      # no output at all
    bad_sliding = [dict(p=pix), dict(axial=acc), dict(p=pix.cuda().float()), dict(axial=acc.cuda().float()),
                   dict(axial=torch.zeros((1, 8, 16), dtype=torch.int32, device="cuda")[:, :, ::2]),
                   dict(axial=torch.zeros((2, 8, 8), dtype=torch.int32, device="cuda")),
                   dict(n0=1), dict(n0=-1), dict(n=1), dict(step=0), dict(step=3), dict(thick=0), dict(mode="median")]
    for kw in bad_sliding:
        with pytest.raises(RuntimeError):
            sliding(**kw)
    # the C level: CTG_EINVAL, and nothing is launched
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    p, v, l, a = pix.cuda(), vals.cuda(), lvl.cuda(), acc.cuda()
    P, V, L, A = p.data_ptr(), v.data_ptr(), l.data_ptr(), a.data_ptr()

    def c_inplane(pix=P, K=2, H=8, W=8, n0=0, N=2, axis=0, thick=4, step=2, mode=0, values=V, level=L):
        return lib.ctg_project_slabs_inplane(pix, K, H, W, n0, N, axis, thick, step, mode, 50.0, 400.0, 0, values, level, st)

    def c_sliding(pix=P, K=2, H=8, W=8, n0=0, N=2, thick=2, step=2, mode=0, axial=A):
        return lib.ctg_project_accumulate_sliding(pix, K, H, W, n0, N, thick, step, mode, axial, st)

    for kw in (dict(pix=None), dict(values=None, level=None), dict(pix=P + 1), dict(values=V + 1), dict(K=0), dict(H=0),
               dict(W=65536), dict(N=65536), dict(thick=0), dict(thick=65536, step=1), dict(step=0), dict(step=5), dict(mode=3),
               dict(mode=-1), dict(axis=2), dict(axis=-1), dict(n0=-1), dict(n0=1), dict(N=1)):
        assert c_inplane(**kw) == 1, kw
    for kw in (dict(pix=None), dict(axial=None), dict(pix=P + 1), dict(axial=A + 2), dict(K=0), dict(H=65536), dict(W=0),
               dict(N=65536), dict(thick=0), dict(step=0), dict(step=3), dict(mode=3), dict(n0=-1), dict(n0=1), dict(N=1)):
        assert c_sliding(**kw) == 1, kw
    torch.cuda.synchronize()
    assert (v == 12345).all() and (l == 0xA5).all() and (a == 77).all()
    assert c_inplane(level=None) == 0 and c_sliding() == 0      # the same calls with legal arguments run
    torch.cuda.synchronize()
    assert (v == 0).all() and (l == 0xA5).all() and (a == 77).all()      # max(77, 0)


# ---------------------------------------------------------------------------------------------- 5. SeriesSlabs
def check_slabs(got, vol, mode, thick, step, wc, ww, hu, axes=("axial", "coronal", "sagittal")):
    assert sorted(got) == sorted(axes)
    for a in axes:
        want = slabs_np.slabs(vol, mode, thick[a], step[a], a)
        values, level = got[a]["values"], got[a]["level"]
        values, level = (cpu(values), cpu(level)) if torch.is_tensor(values) else (values, level)
        assert values.dtype == np.int16 and level.dtype == np.uint8
        assert np.array_equal(values, want), (mode, a)
        assert np.array_equal(level, project_np.level(want, wc, ww, hu)), (mode, a)


def test_series_slabs_reset_axes_and_per_axis_counts(ops):
    from cta_gan_amd.infer import SeriesSlabs
    vol = planted(5, 19, 23, seed=3)
    other = planted(5, 19, 23, seed=4)
    thick, step = {"axial": 3, "coronal": 6, "sagittal": 40}, {"axial": 2, "coronal": 1, "sagittal": 7}
    s = SeriesSlabs(5, 19, 23, thick, step, mode="mean", wc=300.0, ww=1500.0, hu=True)
    assert s.axes == ("axial", "coronal", "sagittal") and s.slabs == {"axial": 2, "coronal": 14, "sagittal": 1}
    assert s.thick == {"axial": 3, "coronal": 6, "sagittal": 23} and s.last_len == {"axial": 3, "coronal": 6, "sagittal": 23}
    # int16 + uint8 planes of every axis, and the int32 axial accumulators
    assert s.nbytes == 3 * (2 * 19 * 23 + 14 * 5 * 23 + 1 * 5 * 19) + 4 * 2 * 19 * 23
    for v in (vol, other):      # reset: the axial accumulators start again, the in-plane rows are simply rewritten
        dev = torch.from_numpy(v).cuda()
        s.update(dev[3:], 3)
        s.update(dev[:3], 0)
        check_slabs(s.result(), v, "mean", thick, step, 300.0, 1500.0, True)
        s.reset()
    with pytest.raises(RuntimeError):
        s.update(dev[3:], 4)      # past the last slice
    # an axis subset, one count for all, no level planes, step=None: slabs that do not overlap
    s = SeriesSlabs(5, 19, 23, 4, mode="min", axes=("sagittal", "axial"), level=False)
    assert s.axes == ("axial", "sagittal") and s.step == {"axial": 4, "sagittal": 4} and s.slabs == {"axial": 2, "sagittal": 6}
    assert s.nbytes == 2 * (2 * 19 * 23 + 6 * 5 * 19) + 4 * 2 * 19 * 23 and s.last_len == {"axial": 1, "sagittal": 3}
    s.update(torch.from_numpy(vol).cuda(), 0)
    out = s.result()
    assert sorted(out) == ["axial", "sagittal"] and out["axial"]["level"] is None and out["sagittal"]["level"] is None
    for a in out:
        assert np.array_equal(cpu(out[a]["values"]), slabs_np.slabs(vol, "min", 4, 4, a))
    assert np.array_equal(cpu(out["axial"]["values"]), project_np.project(vol, "min", 4)[0])
    only = SeriesSlabs(5, 19, 23, {"coronal": 2}, axes=("coronal",))
    assert only.acc is None and only.nbytes == 3 * 10 * 5 * 23
    for bad in (dict(thick=3, step=4), dict(thick=0), dict(thick=3, mode="median"), dict(thick=3, axes=()),
                dict(thick={"axial": 3}), dict(thick=3, step={"axial": 1, "coronal": 1, "sagittal": 4})):
        with pytest.raises(ValueError):
            SeriesSlabs(5, 19, 23, **bad)


# ---------------------------------------------------------------------------------------------- 6. SeriesTranslator(slabs=...)
def test_series_translator_slabs(ops):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator, slab_volume
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        g = make_generator()
        vol = synthetic_hu(7, 64, 64, seed=7)
        plain = SeriesTranslator(g, batch=2)(vol)
        assert "slabs" not in plain and len(np.unique(plain["pix"])) > 100
        thick, step = {"axial": 3, "coronal": 10, "sagittal": 8}, {"axial": 1, "coronal": 5, "sagittal": 8}
        for mode in ("max", "mean"):
            tr = SeriesTranslator(g, batch=2, slabs={"thick": thick, "step": step, "mode": mode})
            out = tr(vol)
            assert np.array_equal(out["pix"], plain["pix"]) and np.array_equal(out["level"], plain["level"])
            assert "projections" not in out and "rotation" not in out
            check_slabs(out["slabs"], out["pix"], mode, thick, step, 50.0, 400.0, False)
            assert out["slabs"]["axial"]["values"].shape == (5, 64, 64) and out["slabs"]["coronal"]["values"].shape == (12, 7, 64)
            again = tr(torch.from_numpy(vol))      # the axial accumulators are reset; a CPU tensor returns tensors
            same = slab_volume(out["pix"], thick, step, mode=mode, batch=3)
            on_dev = slab_volume(torch.from_numpy(out["pix"]).cuda(), thick, step, mode=mode, batch=4)
            for a, d in out["slabs"].items():
                for key in ("values", "level"):
                    assert torch.is_tensor(again["slabs"][a][key]) and not again["slabs"][a][key].is_cuda
                    assert np.array_equal(again["slabs"][a][key].numpy(), d[key]), (a, key)
                    assert isinstance(same[a][key], np.ndarray) and np.array_equal(same[a][key], d[key]), (a, key)
                    assert on_dev[a][key].is_cuda and np.array_equal(cpu(on_dev[a][key]), d[key]), (a, key)
        # a 48 x 40 series through a generator that runs at 64 x 64, HU out, another window, two axes, one count for both
        small = synthetic_hu(7, 48, 40, seed=8)
        plain = SeriesTranslator(g, batch=2, size=64, wc=40.0, ww=350.0, hu=True)(small)
        out = SeriesTranslator(g, batch=2, size=64, wc=40.0, ww=350.0, hu=True, level=False,
                               slabs={"thick": 6, "step": 4, "axes": ("coronal", "sagittal")})(small)
        assert out["level"] is None and out["pix"].shape == (7, 48, 40) and np.array_equal(out["pix"], plain["pix"])
        six, four = dict.fromkeys(("coronal", "sagittal"), 6), dict.fromkeys(("coronal", "sagittal"), 4)
        check_slabs(out["slabs"], out["pix"], "max", six, four, 40.0, 350.0, True, axes=("coronal", "sagittal"))
        # the bone-free thin slabs: the subtraction volume as the source, its levels in sub_window with hu = True
        sub_plain = SeriesTranslator(g, batch=2, subtract=True)(vol)
        out = SeriesTranslator(g, batch=2, subtract=True, project_source="sub", sub_window=(120.0, 250.0),
                               slabs={"thick": thick, "step": step})(vol)
        assert np.array_equal(out["pix"], sub_plain["pix"]) and np.array_equal(out["sub"], sub_plain["sub"])
        assert len(np.unique(out["sub"])) > 50
        check_slabs(out["slabs"], out["sub"], "max", thick, step, 120.0, 250.0, True)
        with pytest.raises(ValueError):
            SeriesTranslator(g, slabs={"step": 2})
        with pytest.raises(ValueError):
            SeriesTranslator(g, slabs={"thick": 2, "slab": 2})
    finally:
        nets.set_default_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------- 7. predict.py --sts-dir
def test_predict_command_line_thin_slabs(ops, tmp_path):
    from PIL import Image
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator
    vol = synthetic_hu(5, 48, 40, seed=9)
    np.save(tmp_path / "series.npy", vol)
    (tmp_path / "cfg.yaml").write_text("name: HdGan\nsize: 64\ninput_nc: 1\noutput_nc: 1\n")
    thick, step = {"axial": 3, "coronal": 20, "sagittal": 16}, {"axial": 2, "coronal": 10, "sagittal": 16}
    nets.set_default_compute_dtype("bf16x3")      # predict.py's default
    try:
        g = make_generator(seed=3)
        torch.save(g.state_dict(), tmp_path / "g.pth")
        want = SeriesTranslator(g, batch=2, size=64, wc=40.0, ww=350.0, slabs={"thick": thick, "step": step, "mode": "min"})(vol)
    finally:
        nets.set_default_compute_dtype(torch.float32)
    base = [sys.executable, os.path.join(ROOT, "predict.py"), "--config", str(tmp_path / "cfg.yaml"), "--weights",
            str(tmp_path / "g.pth"), "--input", str(tmp_path / "series.npy"), "--wc", "40", "--ww", "350", "--batch", "2"]
    r = subprocess.run(base + ["--output", str(tmp_path / "out.npy"), "--sts-dir", str(tmp_path / "sts"), "--sts-thick", "3,20,16",
                               "--sts-step", "2,10,16", "--mip-mode", "min", "--aspect", "2"],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert np.array_equal(np.load(tmp_path / "out.npy"), want["pix"])
    slabs = want["slabs"]
    counts = {"axial": 2, "coronal": 4, "sagittal": 3}      # 5 slices: [0, 3) [2, 5); 48 rows: 0 10 20 30; 40 columns: 0 16 32
    assert {a: len(d["values"]) for a, d in slabs.items()} == counts
    names = ["%s_%03d.png" % (a, i) for a in counts for i in range(counts[a])] + ["slabs.npz"]
    assert sorted(os.listdir(tmp_path / "sts")) == sorted(names)
    for a in counts:
        for i in range(counts[a]):
            img = Image.open(tmp_path / "sts" / ("%s_%03d.png" % (a, i)))
            lvl = slabs[a]["level"][i]
            assert img.mode == "L"
            if a == "axial":
                assert np.array_equal(np.asarray(img), lvl)
            else:      # --aspect 2: every row twice
                assert np.asarray(img).shape[0] == 10 and np.array_equal(np.asarray(img), np.repeat(lvl, 2, axis=0))
    npz = np.load(tmp_path / "sts" / "slabs.npz")
    assert sorted(npz.files) == ["axial", "coronal", "sagittal"]
    for a in npz.files:
        assert npz[a].dtype == np.int16 and np.array_equal(npz[a], slabs[a]["values"])
    # without --sts-dir nothing of this is written
    r = subprocess.run(base + ["--output", str(tmp_path / "out2.npy")], capture_output=True, text=True, timeout=600,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert np.array_equal(np.load(tmp_path / "out2.npy"), want["pix"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cfg.yaml", "g.pth", "out.npy", "out2.npy", "series.npy", "sts"]
