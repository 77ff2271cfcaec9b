"""GPU: the rotating projections (csrc/project_rotate.hip through ops.project_rotate, cta_gan_amd/infer.py: SeriesRotator,
rotate_volume, SeriesTranslator(rotate=...), predict.py --rot-dir) against the numpy restatement tests/rotate_np.py.  Exact
integer arithmetic: every comparison is np.array_equal, never a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import project_np
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
    sums a mean can meet) when there is more than one."""
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


def table(h, w, u, t, angles=ANGLES):
    return np.array([rotate_np.coefficients(a, h, w, u, t) for a in angles], dtype=np.int64)


def run(ops, dev, n0, coef, n, u, t, mode, fill=None, wc=50.0, ww=400.0, hu=False, values=True, level=True, out=None):
    """One ops.project_rotate call into fresh (or the given) planes -> (values, level) as numpy."""
    a = len(coef)
    if out is None:
        out = (torch.full((a, n, u), 12345, dtype=torch.int16, device="cuda") if values else None,
               torch.full((a, n, u), 77, dtype=torch.uint8, device="cuda") if level else None)
    ops.project_rotate(dev, n0, coef, t, mode, values=out[0], level=out[1], fill=fill, wc=wc, ww=ww, hu=hu)
    return tuple(None if o is None else cpu(o) for o in out)


# ---------------------------------------------------------------------------------------------- 1. one call equals numpy
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 33, 31), (2, 37, 53), (4, 19, 515), (2, 9, 1032)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_project_rotate_equals_numpy(ops, shape):
    n, h, w = shape
    vol = planted(n, h, w, seed=n * 1000 + w)
    assert vol.min() == -32768 or shape == (1, 1, 1)
    dev = torch.from_numpy(vol).cuda()
    d = rotate_np.detector(h, w)
    for u, t in ((d, d), (w, h)):      # the default detector, and the slice's own width and height
        coef = table(h, w, u, t)
        tab = ops.RotateTable(coef)
        empty = (rotate_np.count(h, w, coef, u, t) == 0)[:, None, :]
        for mode in MODES:
            ref = rotate_np.rotate(vol, coef, u, t, mode, fill=0)
            for hu in (False, True):
                want = np.where(empty, np.int16(-1024 if hu else 0), ref)      # the default fill: air
                for wc, ww in WINDOWS:
                    values, level = run(ops, dev, 0, tab, n, u, t, mode, wc=wc, ww=ww, hu=hu)
                    assert np.array_equal(values, want), (u, t, mode, hu)
                    assert np.array_equal(level, rotate_np.level(want, wc, ww, hu)), (u, t, mode, hu, wc, ww)
            # an explicit fill, and the host table itself instead of the uploaded one
            values, level = run(ops, dev, 0, coef, n, u, t, mode, fill=-32768)
            want = np.where(empty, np.int16(-32768), ref)
            assert np.array_equal(values, want) and np.array_equal(level, rotate_np.level(want, 50.0, 400.0))
    if shape == (4, 19, 515):
        assert d == 516      # three detector segments of 256 columns


# ---------------------------------------------------------------------------------------------- 2. chunks, views, rows
@pytest.fixture(scope="module")
def volume7():
    return planted(7, 33, 31, seed=77)


@pytest.mark.parametrize("mode", MODES)
def test_chunks_in_any_order_and_a_two_byte_aligned_view(ops, volume7, mode):
    n, h, w = volume7.shape
    d = rotate_np.detector(h, w)
    coef = table(h, w, d, d)
    tab = ops.RotateTable(coef)
    dev = torch.from_numpy(volume7).cuda()
    whole = run(ops, dev, 0, tab, n, d, d, mode)
    assert np.array_equal(whole[0], rotate_np.rotate(volume7, coef, d, d, mode))
    assert np.array_equal(whole[1], rotate_np.level(whole[0], 50.0, 400.0))
    # chunks of 2 (the last of 1) in shuffled order: every call writes its own rows
    out = (torch.full((len(coef), n, d), 12345, dtype=torch.int16, device="cuda"),
           torch.full((len(coef), n, d), 77, dtype=torch.uint8, device="cuda"))
    for s in (4, 0, 6, 2):
        got = run(ops, dev[s:s + 2], s, tab, n, d, d, mode, out=out)
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    # the same slices one element into a buffer: only 2-byte aligned
    buf = torch.empty(n * h * w + 1, dtype=torch.int16, device="cuda")
    shifted = buf[1:].view(n, h, w)
    shifted.copy_(dev)
    assert shifted.is_contiguous() and shifted.data_ptr() % 4 == 2
    got = run(ops, shifted, 0, tab, n, d, d, mode)
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    # rows outside n0 .. n0+K-1 keep the sentinel
    got = run(ops, dev[2:4], 2, tab, n, d, d, mode)
    for g, w_, s in ((got[0], whole[0], 12345), (got[1], whole[1], 77)):
        assert np.array_equal(g[:, 2:4], w_[:, 2:4]) and (g[:, :2] == s).all() and (g[:, 4:] == s).all()


def test_values_only_and_level_only(ops, volume7):
    n, h, w = volume7.shape
    d = rotate_np.detector(h, w)
    tab = ops.RotateTable(table(h, w, d, d))
    dev = torch.from_numpy(volume7).cuda()
    values, level = run(ops, dev, 0, tab, n, d, d, "mean", hu=True, wc=300.0, ww=1500.0)
    v_only, none = run(ops, dev, 0, tab, n, d, d, "mean", hu=True, wc=300.0, ww=1500.0, level=False)
    assert none is None and np.array_equal(v_only, values)
    none, l_only = run(ops, dev, 0, tab, n, d, d, "mean", hu=True, wc=300.0, ww=1500.0, values=False)
    assert none is None and np.array_equal(l_only, level)


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_project_rotate_refusals(ops):
    from cta_gan_amd import _lib
    n, h, w, u, t = 4, 8, 8, 12, 12
    coef = table(h, w, u, t, angles=[0, 30])
    pix = torch.zeros((2, h, w), dtype=torch.int16, device="cuda")
    values = torch.full((2, n, u), 12345, dtype=torch.int16, device="cuda")
    level = torch.full((2, n, u), 77, dtype=torch.uint8, device="cuda")
    tab = ops.RotateTable(coef)
    bad = [
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
        args = dict(pix=pix, n0=0, coef=tab, t=t, mode="max", values=values, level=level)
        args.update(kw)
        with pytest.raises(RuntimeError):
            ops.project_rotate(**args)
    with pytest.raises(RuntimeError):
        ops.RotateTable(coef, device="cpu")
    # the extreme values of the ranges are taken
    c = coef.copy()
    c[0] = [(1 << 29) - 1, 65536, -65536, -(1 << 29) + 1, -65536, 65536]
    ops.project_rotate(pix, 2, c, t, "max", values=values.clone(), level=level.clone())

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    P, C, V, L = pix.data_ptr(), tab.dev.data_ptr(), values.data_ptr(), level.data_ptr()

    def call(pix=P, K=2, H=h, W=w, n0=0, N=n, coef=C, A=2, U=u, T=t, mode=0, fill=0, values=V, level=L):
        return lib.ctg_project_rotate(pix, K, H, W, n0, N, coef, A, U, T, mode, fill, 50.0, 400.0, 0, values, level, st)

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
    coef = table(h, w, d, d, angles)
    want = rotate_np.rotate(vol, coef, d, d, "min", fill=-1024)
    r = SeriesRotator(n, h, w, angles, mode="min", hu=True, wc=40.0, ww=350.0)
    assert np.array_equal(r.table.host, coef) and r.fill == -1024 and (r.u, r.t) == (d, d)
    for _ in range(2):
        r.update(dev[3:], 3)
        r.update(dev[:3], 0)
        out = r.result()
        assert sorted(out) == ["angles", "level", "values"] and all(t.is_cuda for t in out.values())
        assert np.array_equal(cpu(out["values"]), want) and cpu(out["angles"]).tolist() == angles
        assert np.array_equal(cpu(out["level"]), rotate_np.level(want, 40.0, 350.0, True))
        r.reset()
    with pytest.raises(RuntimeError):
        r.update(dev[3:], 4)      # past the last slice
    with pytest.raises(ValueError):
        SeriesRotator(n, h, w, angles, mode="median")
    with pytest.raises(ValueError):
        SeriesRotator(n, h, w, [])
    # an explicit detector and fill, no level planes
    r = SeriesRotator(n, h, w, [0, 90], mode="mean", detector=(30, 40), fill=-7, level=False)
    r.update(dev, 0)
    out = r.result()
    assert out["level"] is None
    assert np.array_equal(cpu(out["values"]), rotate_np.rotate(vol, table(h, w, 30, 40, [0, 90]), 30, 40, "mean", fill=-7))

    # rotate_volume: a host array, a CPU tensor and a device tensor come back as their own kind
    want = rotate_np.rotate(vol, table(h, w, d, d, view_angles(3)), d, d, "max")
    got = rotate_volume(vol, 3, batch=2)
    assert isinstance(got["values"], np.ndarray) and got["angles"].tolist() == [0.0, 120.0, 240.0]
    assert np.array_equal(got["values"], want) and np.array_equal(got["level"], rotate_np.level(want, 50.0, 400.0))
    got = rotate_volume(torch.from_numpy(vol), view_angles(3), batch=4)
    assert torch.is_tensor(got["values"]) and not got["values"].is_cuda and not got["angles"].is_cuda
    assert np.array_equal(got["values"].numpy(), want) and np.array_equal(got["level"].numpy(), rotate_np.level(want, 50.0, 400.0))
    got = rotate_volume(dev, view_angles(3), level=False)
    assert got["values"].is_cuda and got["level"] is None and np.array_equal(cpu(got["values"]), want)
    with pytest.raises(RuntimeError):
        rotate_volume(vol.astype(np.int32), 3)


# ---------------------------------------------------------------------------------------------- 5. SeriesTranslator(rotate=...)
def make_generator(seed=0):
    from cta_gan_amd import synth
    from cta_gan_amd.Model.HdGan import Generator
    return synth.fill_module(Generator(1, 1), seed=seed).cuda()


def synthetic_hu(n, h, w, seed):
    return np.random.RandomState(seed).randint(-1100, 3200, size=(n, h, w)).astype(np.int16)


def check_rotation(rot, pix, angles, mode, wc, ww, hu):
    n, h, w = pix.shape
    d = rotate_np.detector(h, w)
    want = rotate_np.rotate(pix, table(h, w, d, d, angles), d, d, mode, fill=-1024 if hu else 0)
    assert sorted(rot) == ["angles", "level", "values"]
    assert np.asarray(rot["angles"]).dtype == np.float64 and np.asarray(rot["angles"]).tolist() == list(angles)
    assert rot["values"].dtype == np.int16 and rot["values"].shape == (len(angles), n, d)
    assert np.array_equal(rot["values"], want)
    assert rot["level"].dtype == np.uint8 and np.array_equal(rot["level"], rotate_np.level(want, wc, ww, hu))


def test_series_translator_rotation(ops):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator, view_angles
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        g = make_generator()
        vol = synthetic_hu(5, 64, 64, seed=7)
        plain = SeriesTranslator(g, batch=2, project="max")(vol)
        assert "rotation" not in plain and len(np.unique(plain["pix"])) > 100
        none = SeriesTranslator(g, batch=2, rotate=None)(vol)
        assert "rotation" not in none and "projections" not in none and np.array_equal(none["pix"], plain["pix"])
        tr = SeriesTranslator(g, batch=2, rotate=5, project="max")
        out = tr(vol)
        assert np.array_equal(out["pix"], plain["pix"]) and np.array_equal(out["level"], plain["level"])
        check_rotation(out["rotation"], out["pix"], view_angles(5), "max", 50.0, 400.0, False)
        for a, dct in plain["projections"].items():      # the projections are what they were
            assert np.array_equal(out["projections"][a]["values"], dct["values"])
            assert np.array_equal(out["projections"][a]["level"], dct["level"])
        again = tr(torch.from_numpy(vol))      # the rotator is kept; a CPU tensor returns tensors
        assert all(torch.is_tensor(t) and not t.is_cuda for t in again["rotation"].values())
        assert np.array_equal(again["rotation"]["values"].numpy(), out["rotation"]["values"])
        assert np.array_equal(again["rotation"]["level"].numpy(), out["rotation"]["level"])
        # degrees given one by one, a mode of its own, a 48 x 40 series through a generator that runs at 64 x 64, HU out
        small = synthetic_hu(5, 48, 40, seed=8)
        out = SeriesTranslator(g, batch=2, size=64, wc=40.0, ww=350.0, hu=True, level=False, rotate=[0.0, 33.5, 90.0],
                               rotate_mode="mean")(small)
        assert out["level"] is None and "projections" not in out and out["pix"].shape == (5, 48, 40)
        check_rotation(out["rotation"], out["pix"], [0.0, 33.5, 90.0], "mean", 40.0, 350.0, True)
        with pytest.raises(ValueError):
            SeriesTranslator(g, rotate=3, rotate_mode="median")
    finally:
        nets.set_default_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------- 6. predict.py --rot-dir
def test_predict_command_line_rotation(ops, tmp_path):
    from PIL import Image
    vol = synthetic_hu(5, 48, 40, seed=9)
    np.save(tmp_path / "series.npy", vol)
    (tmp_path / "cfg.yaml").write_text("name: HdGan\nsize: 64\ninput_nc: 1\noutput_nc: 1\n")
    torch.save(make_generator(seed=3).state_dict(), tmp_path / "g.pth")
    cmd = [sys.executable, os.path.join(ROOT, "predict.py"), "--config", str(tmp_path / "cfg.yaml"), "--weights",
           str(tmp_path / "g.pth"), "--input", str(tmp_path / "series.npy"), "--wc", "40", "--ww", "350", "--batch", "2",
           "--output", str(tmp_path / "out.npy"), "--rot-dir", str(tmp_path / "rot"), "--rot-angles", "4", "--rot-span", "180",
           "--mip-mode", "min", "--aspect", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    pix = np.load(tmp_path / "out.npy")
    assert pix.shape == vol.shape and pix.dtype == np.int16 and len(np.unique(pix)) > 100
    angles = [0.0, 45.0, 90.0, 135.0]
    d = rotate_np.detector(48, 40)
    want = rotate_np.rotate(pix, table(48, 40, d, d, angles), d, d, "min")
    want_level = rotate_np.level(want, 40.0, 350.0)
    assert sorted(os.listdir(tmp_path / "rot")) == ["rot_%03d.png" % i for i in range(4)] + ["rotation.npz"]
    for i in range(4):      # --aspect 2: every row twice
        img = Image.open(tmp_path / "rot" / ("rot_%03d.png" % i))
        assert img.mode == "L" and np.asarray(img).shape == (10, d)
        assert np.array_equal(np.asarray(img), np.repeat(want_level[i], 2, axis=0))
    npz = np.load(tmp_path / "rot" / "rotation.npz")
    assert sorted(npz.files) == ["angles", "level", "values"] and npz["angles"].tolist() == angles
    assert npz["values"].dtype == np.int16 and np.array_equal(npz["values"], want)
    assert npz["level"].dtype == np.uint8 and np.array_equal(npz["level"], want_level)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cfg.yaml", "g.pth", "out.npy", "rot", "series.npy"]
