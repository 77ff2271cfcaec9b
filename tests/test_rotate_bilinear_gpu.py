"""GPU: bilinear sampling and oversampled rays of the rotating projections (csrc/project_rotate.hip: ctg_project_rotate_bilinear
through ops.project_rotate(sampling="bilinear"); oversampled tables through both entry points; SeriesRotator, rotate_volume,
SeriesTranslator(rotate_sampling=, rotate_oversample=), predict.py --rot-sampling / --rot-oversample) against the numpy
restatements tests/rotate_lerp_np.py and tests/rotate_np.py.  Exact integer arithmetic: every comparison is np.array_equal, never a
tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rotate_lerp_np
import rotate_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["max", "min", "mean"]
ANGLES = [0, 90, 180, 270, 45, 10, 137.5, -30, 359.9]
WINDOWS = [(50.0, 400.0), (300.0, 1500.0)]

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


def planted(n, h, w, seed):
    """Random int16 with both extremes planted at the corners and edges of every slice; the last slice is all 32767 (the largest
    sums a mean can meet, and the accumulator's upper end) when there is more than one."""
    rng = np.random.RandomState(seed)
    vol = rng.randint(-32768, 32768, size=(n, h, w)).astype(np.int16)
    lo, hi = np.int16(-32768), np.int16(32767)
    for i in range(n):
        a, b = (lo, hi) if i % 2 == 0 else (hi, lo)
        vol[i, h // 2, w - 1], vol[i, h - 1, w // 2] = a, b
        vol[i, 0, 0], vol[i, h - 1, w - 1] = b, a
    if n > 1:
        vol[n - 1] = hi
    return vol


def table(h, w, u, t, s=1, angles=ANGLES):
    """Rays of t voxels in t s steps."""
    return np.array([rotate_lerp_np.coefficients(a, h, w, u, t, s) for a in angles], dtype=np.int64)


def run(ops, dev, n0, coef, n, u, steps, mode, sampling="bilinear", fill=None, wc=50.0, ww=400.0, hu=False, values=True, level=True,
        out=None):
    """One ops.project_rotate call into fresh (or the given) planes -> (values, level) as numpy."""
    a = len(coef)
    if out is None:
        out = (torch.full((a, n, u), 12345, dtype=torch.int16, device="cuda") if values else None,
               torch.full((a, n, u), 77, dtype=torch.uint8, device="cuda") if level else None)
    ops.project_rotate(dev, n0, coef, steps, mode, values=out[0], level=out[1], fill=fill, wc=wc, ww=ww, hu=hu, sampling=sampling)
    return tuple(None if o is None else cpu(o) for o in out)


# ---------------------------------------------------------------------------------------------- 1. one call equals numpy
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 33, 31), (2, 37, 53), (4, 19, 515)]


@pytest.mark.parametrize("s", [1, 2, 3], ids=lambda s: "s%d" % s)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_bilinear_equals_numpy(ops, shape, s):
    n, h, w = shape
    vol = planted(n, h, w, seed=n * 1000 + w)
    assert vol.min() == -32768 or shape == (1, 1, 1)
    dev = torch.from_numpy(vol).cuda()
    d = rotate_np.detector(h, w)
    for u, t in ((d, d), (w, h)):      # the default detector, and the slice's own width and height
        coef = table(h, w, u, t, s)
        tab = ops.RotateTable(coef)
        empty = (rotate_np.count(h, w, coef, u, t * s) == 0)[:, None, :]
        refs = rotate_lerp_np.rotate_modes(vol, coef, u, t * s, MODES, fill=0)
        for mode in MODES:
            for hu in (False, True):
                want = np.where(empty, np.int16(-1024 if hu else 0), refs[mode])      # the default fill: air
                for wc, ww in WINDOWS:
                    values, level = run(ops, dev, 0, tab, n, u, t * s, mode, wc=wc, ww=ww, hu=hu)
                    assert np.array_equal(values, want), (u, t, mode, hu)
                    assert np.array_equal(level, rotate_np.level(want, wc, ww, hu)), (u, t, mode, hu, wc, ww)
            # an explicit fill, and the host table itself instead of the uploaded one
            values, level = run(ops, dev, 0, coef, n, u, t * s, mode, fill=-32768)
            want = np.where(empty, np.int16(-32768), refs[mode])
            assert np.array_equal(values, want) and np.array_equal(level, rotate_np.level(want, 50.0, 400.0))
    if shape == (4, 19, 515):
        assert d == 516      # three detector segments of 256 columns, the last with 4 live ones


@pytest.mark.parametrize("s", [2, 3], ids=lambda s: "s%d" % s)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_nearest_takes_an_oversampled_table(ops, shape, s):
    """The existing entry under a table of steps of 1 / s voxel, against the nearest restatement with that table."""
    n, h, w = shape
    vol = planted(n, h, w, seed=n * 1000 + w)
    dev = torch.from_numpy(vol).cuda()
    d = rotate_np.detector(h, w)
    for u, t in ((d, d), (w, h)):
        coef = table(h, w, u, t, s)
        tab = ops.RotateTable(coef)
        for mode in MODES:
            want = rotate_np.rotate(vol, coef, u, t * s, mode, fill=-1024)
            values, level = run(ops, dev, 0, tab, n, u, t * s, mode, sampling="nearest", hu=True, wc=300.0, ww=1500.0)
            assert np.array_equal(values, want), (u, t, mode)
            assert np.array_equal(level, rotate_np.level(want, 300.0, 1500.0, True)), (u, t, mode)


def test_the_two_samplings_differ_and_share_their_empty_rays(ops):
    n, h, w = 2, 33, 31
    vol = planted(n, h, w, seed=5)
    dev = torch.from_numpy(vol).cuda()
    d = rotate_np.detector(h, w)
    coef = table(h, w, d, d, 1, angles=[45, 10])
    near = run(ops, dev, 0, coef, n, d, d, "max", sampling="nearest", fill=-7)[0]
    lerp = run(ops, dev, 0, coef, n, d, d, "max", sampling="bilinear", fill=-7)[0]
    assert not np.array_equal(near[:, 0], lerp[:, 0])
    empty = rotate_np.count(h, w, coef, d, d) == 0
    assert empty.any() and (near[:, 1][empty] == -7).all() and (lerp[:, 1][empty] == -7).all()
    assert (near[:, 1][~empty] == 32767).all() and (lerp[:, 1][~empty] == 32767).all()      # the constant slice


# ---------------------------------------------------------------------------------------------- 2. chunks, views, rows
@pytest.fixture(scope="module")
def volume7():
    return planted(7, 33, 31, seed=77)


@pytest.fixture(scope="module")
def whole7(volume7):
    """The restatement of volume7 under the default detector at two steps per voxel, every mode: computed once, never changed."""
    n, h, w = volume7.shape
    d = rotate_np.detector(h, w)
    coef = table(h, w, d, d, 2)
    ref = rotate_lerp_np.rotate_modes(volume7, coef, d, 2 * d, MODES)
    for v in ref.values():
        v.setflags(write=False)
    return d, coef, ref


@pytest.mark.parametrize("mode", MODES)
def test_chunks_in_any_order_and_a_two_byte_aligned_view(ops, volume7, whole7, mode):
    n, h, w = volume7.shape
    d, coef, ref = whole7
    tab = ops.RotateTable(coef)
    dev = torch.from_numpy(volume7).cuda()
    whole = run(ops, dev, 0, tab, n, d, 2 * d, mode)
    assert np.array_equal(whole[0], ref[mode])
    assert np.array_equal(whole[1], rotate_np.level(ref[mode], 50.0, 400.0))
    # chunks of 2 (the last of 1) in shuffled order: every call writes its own rows
    out = (torch.full((len(coef), n, d), 12345, dtype=torch.int16, device="cuda"),
           torch.full((len(coef), n, d), 77, dtype=torch.uint8, device="cuda"))
    for s in (4, 0, 6, 2):
        got = run(ops, dev[s:s + 2], s, tab, n, d, 2 * d, mode, out=out)
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    # the same slices one element into a buffer: only 2-byte aligned, so no pair of neighbours may be one 32-bit load
    buf = torch.empty(n * h * w + 1, dtype=torch.int16, device="cuda")
    shifted = buf[1:].view(n, h, w)
    shifted.copy_(dev)
    assert shifted.is_contiguous() and shifted.data_ptr() % 4 == 2
    got = run(ops, shifted, 0, tab, n, d, 2 * d, mode)
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    # rows outside n0 .. n0+K-1 keep the sentinel
    got = run(ops, dev[2:4], 2, tab, n, d, 2 * d, mode)
    for g, w_, s in ((got[0], whole[0], 12345), (got[1], whole[1], 77)):
        assert np.array_equal(g[:, 2:4], w_[:, 2:4]) and (g[:, :2] == s).all() and (g[:, 4:] == s).all()


def test_values_only_and_level_only(ops, volume7, whole7):
    n, h, w = volume7.shape
    d, coef, _ = whole7
    tab = ops.RotateTable(coef)
    dev = torch.from_numpy(volume7).cuda()
    values, level = run(ops, dev, 0, tab, n, d, 2 * d, "mean", hu=True, wc=300.0, ww=1500.0)
    v_only, none = run(ops, dev, 0, tab, n, d, 2 * d, "mean", hu=True, wc=300.0, ww=1500.0, level=False)
    assert none is None and np.array_equal(v_only, values)
    none, l_only = run(ops, dev, 0, tab, n, d, 2 * d, "mean", hu=True, wc=300.0, ww=1500.0, values=False)
    assert none is None and np.array_equal(l_only, level)


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_bilinear_refusals(ops):
    from cta_gan_amd import _lib
    n, h, w, u, t = 4, 8, 8, 12, 12
    coef = table(h, w, u, t, 1, angles=[0, 30])
    pix = torch.zeros((2, h, w), dtype=torch.int16, device="cuda")
    values = torch.full((2, n, u), 12345, dtype=torch.int16, device="cuda")
    level = torch.full((2, n, u), 77, dtype=torch.uint8, device="cuda")
    tab = ops.RotateTable(coef)
    assert sorted(ops.ROTATE_SAMPLINGS) == ["bilinear", "nearest"]
    bad = [
        dict(sampling="cubic"), dict(sampling=None), dict(sampling=1),    # not a sampling
        dict(pix=pix.cpu()),                                              # a CPU tensor
        dict(values=values.cpu()), dict(level=level.cpu()),               # outputs on another device than pix
        dict(pix=pix.int()), dict(pix=pix.float()),                       # a wrong dtype
        dict(values=values.int()), dict(level=level.to(torch.int8)),
        dict(pix=pix[0]),                                                 # a wrong shape
        dict(values=values[0]), dict(level=level[:, :, :-1]),
        dict(values=values[:1], level=level[:1]),                         # one plane for two angles
        dict(values=values.transpose(1, 2)),                              # not contiguous
        dict(values=None, level=None),                                    # nothing to write
        dict(n0=3), dict(n0=-1), dict(n0=n),                              # a chunk outside the volume
        dict(mode="median"), dict(mode=3),
        dict(fill=32768), dict(fill=-32769),
        dict(t=0), dict(t=4097),
        dict(coef=tab.dev),                                               # a bare device table: it cannot be checked
        dict(coef=coef[:, :5]), dict(coef=coef.astype(np.float64)),
    ]
    for i, j, v in ((0, 1, 65537), (0, 2, -65537), (1, 4, 65537), (1, 5, -65537), (0, 0, 1 << 29), (1, 3, -(1 << 29))):
        c = coef.copy()
        c[i, j] = v                                                       # a coefficient outside its range
        bad.append(dict(coef=c))
    for kw in bad:
        args = dict(pix=pix, n0=0, coef=tab, t=t, mode="max", values=values, level=level, sampling="bilinear")
        args.update(kw)
        with pytest.raises(RuntimeError):
            ops.project_rotate(**args)
    torch.cuda.synchronize()
    assert (values == 12345).all() and (level == 77).all()      # nothing was launched
    # the extreme values of the ranges are taken: the sums wrap nowhere, and whatever they give, every address is in the slice
    c = coef.copy()
    c[0] = [(1 << 29) - 1, 65536, -65536, -(1 << 29) + 1, -65536, 65536]
    ops.project_rotate(pix, 2, c, t, "max", values=values.clone(), level=level.clone(), sampling="bilinear")

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    P, C, V, L = pix.data_ptr(), tab.dev.data_ptr(), values.data_ptr(), level.data_ptr()

    def call(pix=P, K=2, H=h, W=w, n0=0, N=n, coef=C, A=2, U=u, T=t, mode=0, fill=0, values=V, level=L):
        return lib.ctg_project_rotate_bilinear(pix, K, H, W, n0, N, coef, A, U, T, mode, fill, 50.0, 400.0, 0, values, level, st)

    refused = [dict(pix=None), dict(coef=None), dict(values=None, level=None), dict(K=0), dict(n0=-1), dict(n0=3), dict(K=5),
               dict(H=0), dict(H=4097), dict(W=0), dict(W=4097), dict(U=0), dict(U=4097), dict(T=0), dict(T=4097),
               dict(A=0), dict(A=4097), dict(mode=-1), dict(mode=3), dict(fill=32768), dict(fill=-32769),
               dict(pix=P + 1), dict(coef=C + 2), dict(values=V + 1)]
    for kw in refused:
        assert call(**kw) == 1, kw      # CTG_EINVAL
    torch.cuda.synchronize()
    assert (values == 12345).all() and (level == 77).all()      # nothing was launched
    assert call() == 0 and call(values=None) == 0 and call(level=None) == 0
    torch.cuda.synchronize()
    assert (values[:, :2] == 0).all() and (values[:, 2:] == 12345).all()


# ---------------------------------------------------------------------------------------------- 4. SeriesRotator, rotate_volume
def test_series_rotator_and_rotate_volume(ops):
    from cta_gan_amd.infer import SeriesRotator, rotate_volume, view_angles
    vol = planted(5, 19, 23, seed=3)
    n, h, w = vol.shape
    dev = torch.from_numpy(vol).cuda()
    angles = view_angles(4, span=180.0, start=15.0)
    d = rotate_np.detector(h, w)
    coef = table(h, w, d, d, 2, angles)
    want = rotate_lerp_np.rotate(vol, coef, d, 2 * d, "min", fill=-1024)
    r = SeriesRotator(n, h, w, angles, mode="min", hu=True, wc=40.0, ww=350.0, sampling="bilinear", oversample=2)
    assert np.array_equal(r.table.host, coef) and r.fill == -1024 and (r.u, r.t, r.steps) == (d, d, 2 * d)
    assert (r.sampling, r.oversample) == ("bilinear", 2)
    for _ in range(2):
        r.update(dev[3:], 3)
        r.update(dev[:3], 0)
        out = r.result()
        assert sorted(out) == ["angles", "level", "values"] and all(t.is_cuda for t in out.values())
        assert np.array_equal(cpu(out["values"]), want) and cpu(out["angles"]).tolist() == angles
        assert np.array_equal(cpu(out["level"]), rotate_np.level(want, 40.0, 350.0, True))
        r.reset()
    # the defaults are nearest sampling at unit steps
    r = SeriesRotator(n, h, w, angles, mode="min")
    assert (r.sampling, r.oversample, r.t, r.steps) == ("nearest", 1, d, d)
    r.update(dev, 0)
    assert np.array_equal(cpu(r.result()["values"]), rotate_np.rotate(vol, table(h, w, d, d, 1, angles), d, d, "min"))
    for kw in (dict(sampling="cubic"), dict(oversample=0), dict(oversample=1.5)):
        with pytest.raises(ValueError):
            SeriesRotator(n, h, w, angles, **kw)
    with pytest.raises(ValueError):
        SeriesRotator(n, h, w, angles, detector=(30, 2049), oversample=2)      # 4098 steps
    # an explicit detector and fill, no level planes, three steps per voxel
    r = SeriesRotator(n, h, w, [0, 90], mode="mean", detector=(30, 40), fill=-7, level=False, sampling="bilinear", oversample=3)
    assert (r.t, r.steps) == (40, 120)
    r.update(dev, 0)
    out = r.result()
    assert out["level"] is None
    assert np.array_equal(cpu(out["values"]), rotate_lerp_np.rotate(vol, table(h, w, 30, 40, 3, [0, 90]), 30, 120, "mean", fill=-7))

    # rotate_volume: a host array, a CPU tensor and a device tensor come back as their own kind
    want = rotate_lerp_np.rotate(vol, table(h, w, d, d, 2, view_angles(3)), d, 2 * d, "max")
    got = rotate_volume(vol, 3, batch=2, sampling="bilinear", oversample=2)
    assert isinstance(got["values"], np.ndarray) and got["angles"].tolist() == [0.0, 120.0, 240.0]
    assert np.array_equal(got["values"], want) and np.array_equal(got["level"], rotate_np.level(want, 50.0, 400.0))
    got = rotate_volume(torch.from_numpy(vol), view_angles(3), batch=4, sampling="bilinear", oversample=2)
    assert torch.is_tensor(got["values"]) and not got["values"].is_cuda and not got["angles"].is_cuda
    assert np.array_equal(got["values"].numpy(), want) and np.array_equal(got["level"].numpy(), rotate_np.level(want, 50.0, 400.0))
    got = rotate_volume(dev, view_angles(3), level=False, sampling="bilinear", oversample=2)
    assert got["values"].is_cuda and got["level"] is None and np.array_equal(cpu(got["values"]), want)
    # nearest sampling, oversampled
    got = rotate_volume(dev, view_angles(3), level=False, oversample=2)
    assert np.array_equal(cpu(got["values"]), rotate_np.rotate(vol, table(h, w, d, d, 2, view_angles(3)), d, 2 * d, "max"))


# ---------------------------------------------------------------------------------------------- 5. SeriesTranslator
def make_generator(seed=0):
    from cta_gan_amd import synth
    from cta_gan_amd.Model.HdGan import Generator
    return synth.fill_module(Generator(1, 1), seed=seed).cuda()


def synthetic_hu(n, h, w, seed):
    return np.random.RandomState(seed).randint(-1100, 3200, size=(n, h, w)).astype(np.int16)


def test_series_translator_bilinear_rotation(ops):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator, view_angles
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        g = make_generator()
        vol = synthetic_hu(5, 64, 64, seed=7)
        d = rotate_np.detector(64, 64)
        angles = view_angles(5)
        tr = SeriesTranslator(g, batch=2, size=64, rotate=5, rotate_sampling="bilinear", rotate_oversample=2)
        out = tr(vol)
        pix, rot = out["pix"], out["rotation"]
        assert len(np.unique(pix)) > 100 and sorted(rot) == ["angles", "level", "values"]
        want = rotate_lerp_np.rotate(pix, table(64, 64, d, d, 2, angles), d, 2 * d, "max")
        assert rot["values"].dtype == np.int16 and rot["values"].shape == (5, 5, d) and np.array_equal(rot["values"], want)
        assert rot["level"].dtype == np.uint8 and np.array_equal(rot["level"], rotate_np.level(want, 50.0, 400.0))
        assert np.asarray(rot["angles"]).tolist() == angles
        # the kept rotator is rebuilt for another shape, with the same sampling
        small = synthetic_hu(3, 48, 40, seed=8)
        out = tr(small)
        ds = rotate_np.detector(48, 40)
        assert (tr._views["rotation"].n, tr._views["rotation"].sampling, tr._views["rotation"].steps) == (3, "bilinear", 2 * ds)
        want = rotate_lerp_np.rotate(out["pix"], table(48, 40, ds, ds, 2, angles), ds, 2 * ds, "max")
        assert np.array_equal(out["rotation"]["values"], want)
        # the defaults: today's rotation, nearest sampling at unit steps
        plain = SeriesTranslator(g, batch=2, rotate=5)(vol)
        assert np.array_equal(plain["pix"], pix)
        want = rotate_np.rotate(pix, table(64, 64, d, d, 1, angles), d, d, "max")
        assert np.array_equal(plain["rotation"]["values"], want)
        assert np.array_equal(plain["rotation"]["level"], rotate_np.level(want, 50.0, 400.0))
        for kw in (dict(rotate_sampling="cubic"), dict(rotate_oversample=0)):
            with pytest.raises(ValueError):
                SeriesTranslator(g, rotate=3, **kw)
    finally:
        nets.set_default_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------- 6. predict.py
def test_predict_command_line_bilinear_rotation(ops, tmp_path):
    from PIL import Image
    vol = synthetic_hu(5, 48, 40, seed=9)
    np.save(tmp_path / "series.npy", vol)
    (tmp_path / "cfg.yaml").write_text("name: HdGan\nsize: 64\ninput_nc: 1\noutput_nc: 1\n")
    torch.save(make_generator(seed=3).state_dict(), tmp_path / "g.pth")
    cmd = [sys.executable, os.path.join(ROOT, "predict.py"), "--config", str(tmp_path / "cfg.yaml"), "--weights",
           str(tmp_path / "g.pth"), "--input", str(tmp_path / "series.npy"), "--wc", "40", "--ww", "350", "--batch", "2",
           "--output", str(tmp_path / "out.npy"), "--rot-dir", str(tmp_path / "rot"), "--rot-angles", "4", "--rot-span", "180",
           "--rot-sampling", "bilinear", "--rot-oversample", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    pix = np.load(tmp_path / "out.npy")
    assert pix.shape == vol.shape and pix.dtype == np.int16 and len(np.unique(pix)) > 100
    angles = [0.0, 45.0, 90.0, 135.0]
    d = rotate_np.detector(48, 40)
    want = rotate_lerp_np.rotate(pix, table(48, 40, d, d, 2, angles), d, 2 * d, "max")
    want_level = rotate_np.level(want, 40.0, 350.0)
    assert sorted(os.listdir(tmp_path / "rot")) == ["rot_%03d.png" % i for i in range(4)] + ["rotation.npz"]
    for i in range(4):
        img = Image.open(tmp_path / "rot" / ("rot_%03d.png" % i))
        assert img.mode == "L" and np.array_equal(np.asarray(img), want_level[i])
    npz = np.load(tmp_path / "rot" / "rotation.npz")
    assert sorted(npz.files) == ["angles", "level", "values"] and npz["angles"].tolist() == angles
    assert npz["values"].dtype == np.int16 and np.array_equal(npz["values"], want)
    assert npz["level"].dtype == np.uint8 and np.array_equal(npz["level"], want_level)
