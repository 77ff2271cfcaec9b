"""GPU: the series projections (csrc/project.hip through ops.project_accumulate / ops.project_finish, cta_gan_amd/infer.py:
SeriesProjector, project_volume, SeriesTranslator(project=...), predict.py --mip-dir) against the numpy restatement
tests/project_np.py.  Exact integer arithmetic: every comparison is np.array_equal, never a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import project_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["max", "min", "sum"]
IDENTITY = {"max": -32768, "min": 32767, "sum": 0}

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


def acc_np(vol, mode, thick):
    """The int32 accumulators after the whole volume: the sums themselves for "sum"."""
    v = vol.astype(np.int64)
    red = {"max": np.max, "min": np.min, "sum": np.sum}[mode]
    axial = np.stack([red(v[s:s + thick], axis=0) for s in range(0, v.shape[0], thick)])
    return axial.astype(np.int32), red(v, axis=1).astype(np.int32), red(v, axis=2).astype(np.int32)


def fresh(ops, mode, n, h, w, thick, which=("axial", "coronal", "sagittal")):
    shapes = {"axial": ((n + thick - 1) // thick, h, w), "coronal": (n, w), "sagittal": (n, h)}
    return {a: torch.full(shapes[a], IDENTITY[mode], dtype=torch.int32, device="cuda") for a in which}


def planted(k, h, w, seed):
    rng = np.random.RandomState(seed)
    vol = rng.randint(-32768, 32768, size=(k, h, w)).astype(np.int16)
    lo, hi = np.int16(-32768), np.int16(32767)
    for i in range(k):      # both extremes at the first pixel, the last pixel, in the last column and in the last row
        a, b = (lo, hi) if i % 2 == 0 else (hi, lo)
        vol[i, h // 2, w - 1], vol[i, h - 1, w // 2] = a, b
        vol[i, 0, 0], vol[i, h - 1, w - 1] = b, a
    return vol


# ---------------------------------------------------------------------------------------------- 1. one call equals numpy
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 37, 53), (5, 64, 48), (4, 19, 515), (2, 9, 1032)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_project_accumulate_equals_numpy(ops, shape):
    k, h, w = shape
    base = planted(k, h, w, seed=k * 1000 + w)
    floor, ceil = base.copy(), base.copy()
    floor[0] = -32768           # a slice that is the max identity
    ceil[k - 1] = 32767         # a slice that is the min identity, and the largest sums
    for vol in (base, floor, ceil):
        dev = torch.from_numpy(vol).cuda()
        # the same slices as a view behind one more plane: with odd H W the base pointer itself is only 2-byte aligned
        shifted = torch.cat([dev[:1], dev])[1:]
        assert shifted.is_contiguous() and shifted.data_ptr() == shifted._base.data_ptr() + 2 * h * w
        for mode in MODES:
            want = acc_np(vol, mode, k)
            for pix in (dev, shifted):
                acc = fresh(ops, mode, k, h, w, k)
                ops.project_accumulate(pix, 0, k, mode, **acc)
                for name, wnt in zip(("axial", "coronal", "sagittal"), want):
                    assert np.array_equal(cpu(acc[name]), wnt), (mode, name, pix is shifted)


# ---------------------------------------------------------------------------------------------- 2. chunks and slabs
@pytest.fixture(scope="module")
def volume7():
    return planted(7, 64, 64, seed=77)


def feed(ops, vol, mode, thick, chunk=2, which=("axial", "coronal", "sagittal")):
    n, h, w = vol.shape
    acc = fresh(ops, mode, n, h, w, thick, which)
    dev = torch.from_numpy(vol).cuda()
    for s in range(0, n, chunk):
        ops.project_accumulate(dev[s:s + chunk], s, thick, mode, **acc)
    return {a: cpu(t) for a, t in acc.items()}


@pytest.mark.parametrize("mode", MODES)
def test_chunks_and_slabs_straddle_each_other(ops, volume7, mode):
    # thick 3: slabs {0-2, 3-5, 6}, chunks {0-1, 2-3, 4-5, 6} -- a slab closes inside a chunk and the last slab is short;
    # thick 1: every slice its own slab; thick 100: the whole volume
    for thick in (3, 1, 100):
        want = dict(zip(("axial", "coronal", "sagittal"), acc_np(volume7, mode, thick)))
        got = feed(ops, volume7, mode, thick)
        assert got["axial"].shape[0] == {3: 3, 1: 7, 100: 1}[thick]
        for a in want:
            assert np.array_equal(got[a], want[a]), (thick, a)
        again = feed(ops, volume7, mode, thick)      # fresh accumulators: the same bits whatever the arrival order
        assert all(np.array_equal(again[a], got[a]) for a in got)
    want = dict(zip(("axial", "coronal", "sagittal"), acc_np(volume7, mode, 3)))
    only = feed(ops, volume7, mode, 3, which=("coronal",))
    assert list(only) == ["coronal"] and np.array_equal(only["coronal"], want["coronal"])
    only = feed(ops, volume7, mode, 3, which=("axial",))
    assert list(only) == ["axial"] and np.array_equal(only["axial"], want["axial"])
    # the chunks in another order: the slab index comes from n0
    n, h, w = volume7.shape
    acc = fresh(ops, mode, n, h, w, 3)
    dev = torch.from_numpy(volume7).cuda()
    for s in (4, 0, 6, 2):
        ops.project_accumulate(dev[s:s + 2], s, 3, mode, **acc)
    assert all(np.array_equal(cpu(acc[a]), want[a]) for a in want)


# ---------------------------------------------------------------------------------------------- 3. project_finish
WINDOWS = [(50.0, 400.0), (300.0, 1500.0)]


@pytest.mark.parametrize("wc,ww", WINDOWS)
@pytest.mark.parametrize("hu", [False, True])
def test_project_finish_values_and_levels(ops, wc, ww, hu):
    rng = np.random.RandomState(5)
    # max: the accumulator is the value -- the 12-bit range of the reference and the whole int16 range
    acc = np.concatenate([rng.randint(0, 4096, size=(2, 37, 53)), rng.randint(-32768, 32768, size=(1, 37, 53))]).astype(np.int32)
    if hu:
        acc = np.maximum(acc - 1024, -32768)
    values, level = ops.project_finish(torch.from_numpy(acc).cuda(), "max", wc=wc, ww=ww, hu=hu)
    assert values.dtype == torch.int16 and level.dtype == torch.uint8 and values.shape == level.shape == acc.shape
    assert np.array_equal(cpu(values), acc.astype(np.int16))
    assert np.array_equal(cpu(level), project_np.level(acc, wc, ww, hu))
    # mean: sums of 3 slices, of 2 in the last slab; negative sums truncate toward zero
    sums = np.concatenate([rng.randint(-3 * 32768, 3 * 32767 + 1, size=(2, 19, 23)),
                           rng.randint(-2 * 32768, 2 * 32767 + 1, size=(1, 19, 23))]).astype(np.int32)
    sums.reshape(-1)[:6] = [-5, -4, -3, -2, -1, 5]
    sums[2].reshape(-1)[:6] = [-5, -4, -3, -2, -1, 5]
    want = np.sign(sums.astype(np.int64)) * (np.abs(sums.astype(np.int64)) // np.array([3, 3, 2]).reshape(3, 1, 1))
    assert want.reshape(-1)[:6].tolist() == [-1, -1, -1, 0, 0, 1] and want[2].reshape(-1)[:6].tolist() == [-2, -2, -1, -1, 0, 2]
    values, level = ops.project_finish(torch.from_numpy(sums).cuda(), "mean", 3, 2, wc=wc, ww=ww, hu=hu)
    assert np.array_equal(cpu(values), want.astype(np.int16))
    assert np.array_equal(cpu(level), project_np.level(want, wc, ww, hu))
    # a 2-d accumulator (coronal, sagittal) is one plane: div_last is its divisor
    flat = torch.from_numpy(sums[2]).cuda()
    v2, l2 = ops.project_finish(flat, "sum", 2, wc=wc, ww=ww, hu=hu)
    assert np.array_equal(cpu(v2), want[2].astype(np.int16)) and np.array_equal(cpu(l2), cpu(level)[2])


@pytest.mark.parametrize("wc,ww", WINDOWS)
def test_project_finish_on_the_level_boundaries(ops, wc, ww):
    cand = np.arange(-1024, 8192, dtype=np.int64)
    lv = project_np.level(cand, wc, ww).astype(int)
    stored = [0, 1]
    for lvl in range(256):      # the smallest stored value that reaches each level, and its neighbour below
        first = int(cand[np.argmax(lv >= lvl)]) if lvl else int(cand[0]) + 1
        assert project_np.level(np.array([first]), wc, ww)[0] == lvl or first == 0
        stored += [first - 1, first]
    stored = np.array(stored, dtype=np.int32).reshape(1, -1)
    want = project_np.level(stored, wc, ww)
    assert np.unique(want).size == 256
    values, level = ops.project_finish(torch.from_numpy(stored).cuda(), "max", wc=wc, ww=ww)
    assert np.array_equal(cpu(values), stored.astype(np.int16)) and np.array_equal(cpu(level), want)
    # hu: an accumulator that holds the same volume minus 1024 gives the same levels
    _, level_hu = ops.project_finish(torch.from_numpy(stored - 1024).cuda(), "max", wc=wc, ww=ww, hu=True)
    assert np.array_equal(cpu(level_hu), want)
    # the level of a projected pixel is the level export_slices gives a pixel of that stored value
    x = torch.from_numpy((np.arange(4096, dtype=np.float64) / 4095 * 2 - 1).astype(np.float32)).cuda().reshape(1, 64, 64)
    pix, lvl = ops.export_slices(x, wc, ww)
    _, lvl2 = ops.project_finish(pix.int(), "max", wc=wc, ww=ww)
    exact = (pix.float() == ((x + 1) * 0.5) * 4095)      # where the float stored value is the integer itself
    assert int(exact.sum()) > 1000 and torch.equal(lvl[exact], lvl2[exact])


def test_project_finish_skipped_outputs(ops):
    from cta_gan_amd import _lib
    acc = torch.arange(-300, 4000, dtype=torch.int32, device="cuda").reshape(1, -1)
    values, level = ops.project_finish(acc, "max")
    v_only, none = ops.project_finish(acc, "max", want_level=False)
    assert none is None and torch.equal(v_only, values)
    none, l_only = ops.project_finish(acc, "max", want_values=False)
    assert none is None and torch.equal(l_only, level)
    with pytest.raises(RuntimeError):
        ops.project_finish(acc, "max", want_values=False, want_level=False)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.ctg_project_finish(acc.data_ptr(), 1, acc.numel(), 0, 1, 1, 50.0, 400.0, 0, None, None, st) == 1      # CTG_EINVAL
    _lib.check(lib.ctg_project_finish(acc.data_ptr(), 1, acc.numel(), 0, 1, 1, 50.0, 400.0, 0, None, l_only.data_ptr(), st),
               "ctg_project_finish")
    assert torch.equal(l_only, level)


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_project_refusals(ops):
    from cta_gan_amd import _lib
    pix = torch.zeros((2, 8, 8), dtype=torch.int16)
    acc = torch.zeros((1, 8, 8), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.project_accumulate(pix, 0, 2, "max", axial=acc.cuda())      # CPU pix
    with pytest.raises(RuntimeError):
        ops.project_accumulate(pix.cuda(), 0, 2, "max", axial=acc)      # CPU accumulator
    with pytest.raises(RuntimeError):
        ops.project_finish(acc, "max")
    pix, acc = pix.cuda(), acc.cuda()
    with pytest.raises(RuntimeError):
        ops.project_accumulate(pix, 0, 2, "max")      # no accumulator at all
    with pytest.raises(RuntimeError):
        ops.project_accumulate(pix, 0, 0, "max", axial=acc)      # thick = 0
    with pytest.raises(RuntimeError):
        ops.project_accumulate(pix.float(), 0, 2, "max", axial=acc)
    with pytest.raises(RuntimeError):
        ops.project_accumulate(pix, 0, 2, "max", axial=acc.float())
    with pytest.raises(RuntimeError):
        ops.project_accumulate(pix, 0, 2, "max", axial=torch.zeros((1, 8, 16), dtype=torch.int32, device="cuda")[:, :, ::2])
    with pytest.raises(RuntimeError):
        ops.project_accumulate(pix, 0, 2, "max", coronal=torch.zeros((1, 8), dtype=torch.int32, device="cuda"))      # 2 rows needed
    with pytest.raises(RuntimeError):
        ops.project_accumulate(pix, 0, 2, "median", axial=acc)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.ctg_project_accumulate(pix.data_ptr(), 2, 8, 8, 0, 2, 0, None, None, None, st) == 1      # CTG_EINVAL
    assert lib.ctg_project_accumulate(pix.data_ptr(), 2, 8, 8, 0, 0, 0, acc.data_ptr(), None, None, st) == 1
    assert lib.ctg_project_accumulate(pix.data_ptr(), 2, 8, 8, -1, 2, 0, acc.data_ptr(), None, None, st) == 1
    assert lib.ctg_project_accumulate(pix.data_ptr(), 2, 8, 65536, 0, 2, 0, acc.data_ptr(), None, None, st) == 1
    assert lib.ctg_project_accumulate(pix.data_ptr(), 2, 8, 8, 0, 2, 3, acc.data_ptr(), None, None, st) == 1
    torch.cuda.synchronize()
    assert int(acc.abs().sum()) == 0      # nothing was launched


# ---------------------------------------------------------------------------------------------- 5. SeriesTranslator(project=...)
def make_generator(seed=0):
    from cta_gan_amd import synth
    from cta_gan_amd.Model.HdGan import Generator
    return synth.fill_module(Generator(1, 1), seed=seed).cuda()


def synthetic_hu(n, h, w, seed):
    return np.random.RandomState(seed).randint(-1100, 3200, size=(n, h, w)).astype(np.int16)


def check_projections(proj, pix, mode, slab, wc, ww, hu):
    want = dict(zip(("axial", "coronal", "sagittal"), project_np.project(pix, mode, slab)))
    assert sorted(proj) == sorted(want)
    for a in want:
        assert proj[a]["values"].dtype == np.int16 and proj[a]["level"].dtype == np.uint8
        assert np.array_equal(proj[a]["values"], want[a]), (mode, a)
        assert np.array_equal(proj[a]["level"], project_np.level(want[a], wc, ww, hu)), (mode, a)


def test_series_translator_projections(ops):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator, project_volume
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        g = make_generator()
        vol = synthetic_hu(7, 64, 64, seed=7)
        plain = SeriesTranslator(g, batch=2)(vol)
        assert "projections" not in plain and len(np.unique(plain["pix"])) > 100
        for mode, slab in (("max", 3), ("mean", None)):
            tr = SeriesTranslator(g, batch=2, project=mode, slab=slab)
            out = tr(vol)
            assert np.array_equal(out["pix"], plain["pix"]) and np.array_equal(out["level"], plain["level"])
            check_projections(out["projections"], out["pix"], mode, slab, 50.0, 400.0, False)
            assert out["projections"]["axial"]["values"].shape == ((3, 64, 64) if slab else (1, 64, 64))
            again = tr(torch.from_numpy(vol))      # the projector is reset; a CPU tensor returns tensors
            for a, d in again["projections"].items():
                assert torch.is_tensor(d["values"]) and not d["values"].is_cuda
                assert np.array_equal(d["values"].numpy(), out["projections"][a]["values"])
                assert np.array_equal(d["level"].numpy(), out["projections"][a]["level"])
            same = project_volume(out["pix"], mode=mode, slab=slab, batch=3)
            on_dev = project_volume(torch.from_numpy(out["pix"]).cuda(), mode=mode, slab=slab, batch=4)
            for a, d in out["projections"].items():
                assert np.array_equal(same[a]["values"], d["values"]) and np.array_equal(same[a]["level"], d["level"])
                assert on_dev[a]["values"].is_cuda and np.array_equal(cpu(on_dev[a]["values"]), d["values"])
                assert np.array_equal(cpu(on_dev[a]["level"]), d["level"])
        # a 48 x 40 series through a generator that runs at 64 x 64, HU out, another window, no per-slice level plane
        small = synthetic_hu(7, 48, 40, seed=8)
        plain = SeriesTranslator(g, batch=2, size=64, wc=40.0, ww=350.0, hu=True)(small)
        out = SeriesTranslator(g, batch=2, size=64, wc=40.0, ww=350.0, hu=True, level=False, project="max", slab=3)(small)
        assert out["level"] is None and out["pix"].shape == (7, 48, 40) and np.array_equal(out["pix"], plain["pix"])
        check_projections(out["projections"], out["pix"], "max", 3, 40.0, 350.0, True)
        same = project_volume(out["pix"], mode="max", slab=3, wc=40.0, ww=350.0, hu=True)
        for a, d in out["projections"].items():
            assert np.array_equal(same[a]["values"], d["values"]) and np.array_equal(same[a]["level"], d["level"])
    finally:
        nets.set_default_compute_dtype(torch.float32)


def test_series_projector_reset_and_axes(ops):
    from cta_gan_amd.infer import SeriesProjector
    vol = planted(5, 19, 23, seed=3)
    dev = torch.from_numpy(vol).cuda()
    p = SeriesProjector(5, 19, 23, mode="min", slab=2, axes=("sagittal", "axial"))
    assert p.axes == ("axial", "sagittal") and p.acc["axial"].shape == (3, 19, 23)
    for _ in range(2):
        p.update(dev[3:], 3)
        p.update(dev[:3], 0)
        out = p.result(50.0, 400.0, level=False)
        want = project_np.project(vol, "min", 2)
        assert sorted(out) == ["axial", "sagittal"] and out["axial"]["level"] is None
        assert np.array_equal(cpu(out["axial"]["values"]), want[0]) and np.array_equal(cpu(out["sagittal"]["values"]), want[2])
        p.reset()
    with pytest.raises(RuntimeError):
        p.update(dev[3:], 4)      # past the last slice
    with pytest.raises(ValueError):
        SeriesProjector(5, 19, 23, mode="median")


# ---------------------------------------------------------------------------------------------- 6. predict.py --mip-dir
def test_predict_command_line_projections(ops, tmp_path):
    from PIL import Image
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator
    vol = synthetic_hu(5, 48, 40, seed=9)
    np.save(tmp_path / "series.npy", vol)
    (tmp_path / "cfg.yaml").write_text("name: HdGan\nsize: 64\ninput_nc: 1\noutput_nc: 1\n")
    nets.set_default_compute_dtype("bf16x3")      # predict.py's default
    try:
        g = make_generator(seed=3)
        torch.save(g.state_dict(), tmp_path / "g.pth")
        want = SeriesTranslator(g, batch=2, size=64, wc=40.0, ww=350.0, project="max", slab=3)(vol)
    finally:
        nets.set_default_compute_dtype(torch.float32)
    base = [sys.executable, os.path.join(ROOT, "predict.py"), "--config", str(tmp_path / "cfg.yaml"), "--weights",
            str(tmp_path / "g.pth"), "--input", str(tmp_path / "series.npy"), "--wc", "40", "--ww", "350", "--batch", "2"]
    r = subprocess.run(base + ["--output", str(tmp_path / "out.npy"), "--mip-dir", str(tmp_path / "mip"), "--slab", "3",
                               "--aspect", "2"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert np.array_equal(np.load(tmp_path / "out.npy"), want["pix"])
    proj = want["projections"]
    assert sorted(os.listdir(tmp_path / "mip")) == ["axial_000.png", "axial_001.png", "coronal.png", "projections.npz", "sagittal.png"]
    for i in range(2):
        img = Image.open(tmp_path / "mip" / ("axial_%03d.png" % i))
        assert img.mode == "L" and np.array_equal(np.asarray(img), proj["axial"]["level"][i])
    for axis in ("coronal", "sagittal"):      # --aspect 2: every row twice
        got = np.asarray(Image.open(tmp_path / "mip" / (axis + ".png")))
        assert got.shape[0] == 10 and np.array_equal(got, np.repeat(proj[axis]["level"], 2, axis=0))
    npz = np.load(tmp_path / "mip" / "projections.npz")
    assert sorted(npz.files) == ["axial", "coronal", "sagittal"]
    for axis in npz.files:
        assert npz[axis].dtype == np.int16 and np.array_equal(npz[axis], proj[axis]["values"])
    # without --mip-dir nothing of this is written
    r = subprocess.run(base + ["--output", str(tmp_path / "out2.npy")], capture_output=True, text=True, timeout=600,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert np.array_equal(np.load(tmp_path / "out2.npy"), want["pix"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cfg.yaml", "g.pth", "mip", "out.npy", "out2.npy", "series.npy"]
