"""GPU: the subtraction volume (csrc/subtract.hip through ops.subtract_slices, cta_gan_amd/infer.py: subtract_volume,
SeriesTranslator(subtract=True), predict.py --sub-output) against the numpy restatement tests/subtract_np.py.  Exact integer
arithmetic: every comparison is np.array_equal, never a tolerance."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import project_np
import rotate_np
import subtract_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MIN = -2 ** 31

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


def planted_pair(b, h, w, seed):
    """(ct, cta): ct uniform in -1100 .. 3200, cta in 0 .. 4095, the int16 extremes at the four corners and mid-edges of each plane."""
    rng = np.random.RandomState(seed)
    ct = rng.randint(-1100, 3201, size=(b, h, w)).astype(np.int16)
    cta = rng.randint(0, 4096, size=(b, h, w)).astype(np.int16)
    lo, hi = np.int16(-32768), np.int16(32767)
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)]
    for i in range(b):
        for j, (y, x) in enumerate(spots):      # (later spots win where they coincide on a small plane)
            up = (i + j) % 2 == 0
            ct[i, y, x], cta[i, y, x] = (lo, hi) if up else (hi, lo)
    return ct, cta


def tie_pair(b, h, w, seed):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 4, size=(b, h, w)) - 1024).astype(np.int16), rng.randint(0, 4, size=(b, h, w)).astype(np.int16)


# ---------------------------------------------------------------------------------------------- 1. one call equals numpy
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 1, 9), (2, 9, 1), (2, 37, 53), (5, 64, 48), (4, 19, 515), (2, 9, 1032)]
SETTINGS = [(None, (None, None)), (60, (-900, 400))]      # (floor, ct_range): everything kept; the floor and the band


def reference(cta, ct, hu, median, floor, ct_range):
    return subtract_np.subtract(cta, ct, hu, median, floor, ct_range[0], ct_range[1])


@functools.lru_cache(maxsize=None)
def cases(shape):
    """[(kind, ct, cta, [(median, floor, ct_range, want), ...]), ...] of a shape: the references are computed once."""
    b, h, w = shape
    out = []
    for kind, (ct, cta) in (("planted", planted_pair(b, h, w, seed=b * 1000 + w)), ("ties", tie_pair(b, h, w, seed=h + w))):
        out.append((kind, ct, cta, [(median, floor, ct_range, reference(cta, ct, False, median, floor, ct_range))
                                    for median in (True, False) for floor, ct_range in SETTINGS]))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_subtract_slices_equals_numpy(ops, shape):
    b, h, w = shape
    for kind, ct, cta, settings in cases(shape):
        d_ct, d_cta = torch.from_numpy(ct).cuda(), torch.from_numpy(cta).cuda()
        cta_hu = np.maximum(cta.astype(np.int32) - 1024, -32768).astype(np.int16)
        exact_hu = (cta_hu.astype(np.int32) + 1024 == cta).all()      # (the planted -32768 cannot be shifted down)
        inputs = [(d_cta, d_ct), (shifted(d_cta), shifted(d_ct))]
        for median, floor, ct_range, want in settings:
            if floor == 60 and kind == "planted" and b * h * w > 1000:
                share = float((want != 0).mean())
                assert 0.05 < share < 0.5, share      # the mask test cannot pass on an all-zero or an all-kept plane
            for xa, xc in inputs:
                sub, level = ops.subtract_slices(xa, xc, median=median, floor=floor, ct_range=ct_range)
                assert sub.dtype == torch.int16 and level.dtype == torch.uint8 and sub.shape == level.shape == xa.shape
                assert np.array_equal(cpu(sub), want), (kind, median, floor, xa is not d_cta)
                assert np.array_equal(cpu(level), subtract_np.level(want)), (kind, median, floor)
            # the hu convention: the input shifted by -1024 gives the same sub
            want_hu = want if exact_hu else reference(cta_hu, ct, True, median, floor, ct_range)
            sub_hu, _ = ops.subtract_slices(torch.from_numpy(cta_hu).cuda(), d_ct, cta_is_hu=True, median=median, floor=floor,
                                            ct_range=ct_range, want_level=False)
            assert np.array_equal(cpu(sub_hu), want_hu), (kind, median, floor)
    # floor = INT_MIN and the int16 band spelled out are the switched-off settings
    sub, _ = ops.subtract_slices(d_cta, d_ct, floor=INT_MIN, ct_range=(-32768, 32767), want_level=False)
    assert np.array_equal(cpu(sub), reference(cta, ct, False, True, None, (None, None)))


# ---------------------------------------------------------------------------------------------- 2. boundaries
def test_floor_and_band_keep_equality_and_drop_the_neighbours(ops):
    floor, ct_min, ct_max = 60, -900, 400
    # row 0: ct inside the band, d = floor - 1, floor, floor + 1;  row 1: d = 500, ct = ct_min - 1, ct_min, ct_max, ct_max + 1
    ct = np.array([[[0, 0, 0, 0], [ct_min - 1, ct_min, ct_max, ct_max + 1]]], dtype=np.int16)
    a = np.maximum(ct.astype(np.int32) + 1024, 0)
    d = np.array([[[floor - 1, floor, floor + 1, floor + 1], [500, 500, 500, 500]]])
    cta = (a + d).astype(np.int16)
    want = np.array([[[0, floor, floor + 1, floor + 1], [0, 500, 500, 0]]], dtype=np.int16)
    assert np.array_equal(subtract_np.subtract(cta, ct, False, False, floor, ct_min, ct_max), want)
    sub, _ = ops.subtract_slices(torch.from_numpy(cta).cuda(), torch.from_numpy(ct).cuda(), median=False, floor=floor,
                                 ct_range=(ct_min, ct_max))
    assert np.array_equal(cpu(sub), want)
    # a negative floor keeps negative differences down to itself
    ct2 = np.full((1, 1, 3), -1024, dtype=np.int16)
    cta2 = np.array([[[-6, -5, -4]]], dtype=np.int16)
    sub, _ = ops.subtract_slices(torch.from_numpy(cta2).cuda(), torch.from_numpy(ct2).cuda(), median=False, floor=-5)
    assert cpu(sub).tolist() == [[[0, -5, -4]]]


# ---------------------------------------------------------------------------------------------- 3. level
@pytest.mark.parametrize("wc,ww", [(150.0, 300.0), (50.0, 400.0)])
def test_level_is_the_projection_level_of_the_value(ops, wc, ww):
    ramp = np.arange(-1024, 8192, dtype=np.int16).reshape(1, 96, 96)      # 9216 values
    planes = [ramp] + [want for shape in SHAPES for _, _, _, settings in cases(shape) for _, _, _, want in settings]
    for want in planes:
        # cta = the wanted value as a stored value over ct = -1024 (a = 0): sub is the value itself
        cta = torch.from_numpy(want).cuda()
        ct = torch.full(want.shape, -1024, dtype=torch.int16, device="cuda")
        sub, level = ops.subtract_slices(cta, ct, median=False, floor=None, wc=wc, ww=ww)
        assert np.array_equal(cpu(sub), want)
        _, fin = ops.project_finish(sub.int(), "max", wc=wc, ww=ww, hu=True)
        assert torch.equal(level, fin)      # equality on the device
        assert np.array_equal(cpu(level), subtract_np.level(want, wc, ww))
    assert np.unique(subtract_np.level(ramp, wc, ww)).size == 256


def test_skipped_outputs(ops):
    ct, cta = planted_pair(2, 37, 53, seed=4)
    d_ct, d_cta = torch.from_numpy(ct).cuda(), torch.from_numpy(cta).cuda()
    sub, level = ops.subtract_slices(d_cta, d_ct)
    s_only, none = ops.subtract_slices(d_cta, d_ct, want_level=False)
    assert none is None and torch.equal(s_only, sub)
    none, l_only = ops.subtract_slices(d_cta, d_ct, want_sub=False)
    assert none is None and torch.equal(l_only, level)
    with pytest.raises(RuntimeError):
        ops.subtract_slices(d_cta, d_ct, want_sub=False, want_level=False)


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_subtract_refusals(ops):
    from cta_gan_amd import _lib
    ct, cta = planted_pair(2, 8, 8, seed=1)
    ct, cta = torch.from_numpy(ct), torch.from_numpy(cta)
    with pytest.raises(RuntimeError):
        ops.subtract_slices(cta, ct.cuda())      # CPU tensors
    with pytest.raises(RuntimeError):
        ops.subtract_slices(cta.cuda(), ct)
    ct, cta = ct.cuda(), cta.cuda()
    with pytest.raises(RuntimeError):
        ops.subtract_slices(cta.float(), ct)
    with pytest.raises(RuntimeError):
        ops.subtract_slices(cta, ct.int())
    with pytest.raises(RuntimeError):
        ops.subtract_slices(cta, ct[:1])      # shape mismatch
    wide = torch.zeros((2, 8, 16), dtype=torch.int16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.subtract_slices(wide[:, :, ::2], ct)      # strided
    with pytest.raises(RuntimeError):
        ops.subtract_slices(cta, wide[:, :, ::2])
    with pytest.raises(RuntimeError):
        ops.subtract_slices(cta, ct, ct_range=(5, 4))
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    canary = torch.full((2, 8, 8), 12345, dtype=torch.int16, device="cuda")
    lvl = torch.full((2, 8, 8), 123, dtype=torch.uint8, device="cuda")
    a, c, s, l = cta.data_ptr(), ct.data_ptr(), canary.data_ptr(), lvl.data_ptr()

    def call(cta=a, ct=c, B=2, H=8, W=8, ct_min=-32768, ct_max=32767, sub=s, level=l):
        return lib.ctg_subtract_slices(cta, ct, B, H, W, 0, 1, 0, ct_min, ct_max, 150.0, 300.0, sub, level, st)

    assert call(cta=None) == 1 and call(ct=None) == 1      # CTG_EINVAL
    assert call(sub=None, level=None) == 1
    for bad in (0, -1, 65536):
        assert call(B=bad) == 1 and call(H=bad) == 1 and call(W=bad) == 1
    assert call(ct_min=5, ct_max=4) == 1
    assert call(cta=a + 1) == 1 and call(ct=c + 1) == 1 and call(sub=s + 1) == 1      # misaligned
    torch.cuda.synchronize()
    assert int((canary != 12345).sum()) == 0 and int((lvl != 123).sum()) == 0      # nothing was launched
    assert call() == 0 and call(level=None) == 0 and call(sub=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(cpu(canary), subtract_np.subtract(cpu(cta), cpu(ct)))


# ---------------------------------------------------------------------------------------------- 5. repeatability
def test_the_same_call_twice_gives_the_same_bits(ops):
    ct, cta = planted_pair(4, 19, 515, seed=11)
    d_ct, d_cta = torch.from_numpy(ct).cuda(), torch.from_numpy(cta).cuda()
    first = ops.subtract_slices(d_cta, d_ct, floor=60, ct_range=(-900, 400))
    again = ops.subtract_slices(d_cta, d_ct, floor=60, ct_range=(-900, 400))
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


# ---------------------------------------------------------------------------------------------- 6. SeriesTranslator(subtract=True)
def make_generator(seed=0):
    from cta_gan_amd import synth
    from cta_gan_amd.Model.HdGan import Generator
    return synth.fill_module(Generator(1, 1), seed=seed).cuda()


def synthetic_hu(n, h, w, seed):
    return np.random.RandomState(seed).randint(-1100, 3200, size=(n, h, w)).astype(np.int16)


def check_sub(out, vol, hu, level=True, **kw):
    want = subtract_np.subtract(out["pix"], vol, hu, **kw)
    assert out["sub"].dtype == np.int16 and np.array_equal(out["sub"], want)
    if level:
        assert out["sub_level"].dtype == np.uint8 and np.array_equal(out["sub_level"], subtract_np.level(want))
    else:
        assert out["sub_level"] is None
    return want


def test_series_translator_subtraction(ops):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator, subtract_volume
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        g = make_generator()
        vol = synthetic_hu(7, 64, 64, seed=7)
        plain = SeriesTranslator(g, batch=2)(vol)
        assert "sub" not in plain and "sub_level" not in plain
        tr = SeriesTranslator(g, batch=2, subtract=True)
        out = tr(vol)
        assert np.array_equal(out["pix"], plain["pix"]) and np.array_equal(out["level"], plain["level"])
        want = check_sub(out, vol, False)
        assert len(np.unique(out["sub"])) >= 100
        again = tr(torch.from_numpy(vol))      # a second call on the same object; a CPU tensor returns tensors
        assert torch.is_tensor(again["sub"]) and not again["sub"].is_cuda and torch.is_tensor(again["sub_level"])
        assert np.array_equal(again["sub"].numpy(), want) and np.array_equal(again["sub_level"].numpy(), out["sub_level"])
        assert np.array_equal(again["pix"].numpy(), plain["pix"])
        # other settings reach the kernel
        out2 = SeriesTranslator(g, batch=3, subtract=True, sub_median=False, sub_floor=60, sub_ct_range=(-900, 400))(vol)
        check_sub(out2, vol, False, median=False, floor=60, ct_min=-900, ct_max=400)
        # volumes that already exist, on the host and on the device
        same = subtract_volume(out["pix"], vol, batch=3)
        assert np.array_equal(same["sub"], out["sub"]) and np.array_equal(same["level"], out["sub_level"])
        on_dev = subtract_volume(torch.from_numpy(out["pix"]).cuda(), torch.from_numpy(vol).cuda(), batch=4, level=False)
        assert on_dev["sub"].is_cuda and on_dev["level"] is None and np.array_equal(cpu(on_dev["sub"]), out["sub"])
        # the bone-free projections: the projector and the rotator see the subtraction chunk, levels in sub_window with hu
        win = (120.0, 240.0)
        view = SeriesTranslator(g, batch=2, subtract=True, sub_window=win, project_source="sub", project="max", slab=3, rotate=4)
        o = view(vol)
        assert np.array_equal(o["pix"], plain["pix"]) and np.array_equal(o["sub"], want)
        assert np.array_equal(o["sub_level"], subtract_np.level(want, *win))
        axes = dict(zip(("axial", "coronal", "sagittal"), project_np.project(o["sub"], "max", 3)))
        assert sorted(o["projections"]) == sorted(axes)
        for a, w_ in axes.items():
            assert np.array_equal(o["projections"][a]["values"], w_), a
            assert np.array_equal(o["projections"][a]["level"], project_np.level(w_, win[0], win[1], True)), a
        d = rotate_np.detector(64, 64)
        coef = [rotate_np.coefficients(ang, 64, 64) for ang in (0.0, 90.0, 180.0, 270.0)]
        rot = rotate_np.rotate(o["sub"], coef, d, d, "max", -1024)
        assert np.array_equal(o["rotation"]["values"], rot)
        assert np.array_equal(o["rotation"]["level"], project_np.level(rot, win[0], win[1], True))
        # project_source="cta" with subtract=True projects the synthesized volume as before
        o2 = SeriesTranslator(g, batch=2, subtract=True, project="max", slab=3)(vol)
        base = SeriesTranslator(g, batch=2, project="max", slab=3)(vol)
        for a in base["projections"]:
            assert np.array_equal(o2["projections"][a]["values"], base["projections"][a]["values"])
            assert np.array_equal(o2["projections"][a]["level"], base["projections"][a]["level"])
        # a 48 x 40 series through a generator that runs at 64 x 64, HU out, no 8-bit planes
        small = synthetic_hu(7, 48, 40, seed=8)
        plain = SeriesTranslator(g, batch=2, size=64, hu=True)(small)
        o3 = SeriesTranslator(g, batch=2, size=64, hu=True, level=False, subtract=True)(small)
        assert o3["level"] is None and o3["pix"].shape == (7, 48, 40) and np.array_equal(o3["pix"], plain["pix"])
        check_sub(o3, small, True, level=False)
        with pytest.raises(ValueError):
            SeriesTranslator(g, project_source="sub")
    finally:
        nets.set_default_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------- 7. predict.py --sub-output
def test_predict_command_line_subtraction(ops, tmp_path):
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
        want = SeriesTranslator(g, batch=2, size=64, subtract=True, sub_floor=30, sub_ct_range=(-900, None), sub_window=(100.0, 200.0),
                                project_source="sub", project="max", slab=3)(vol)
    finally:
        nets.set_default_compute_dtype(torch.float32)
    base = [sys.executable, os.path.join(ROOT, "predict.py"), "--config", str(tmp_path / "cfg.yaml"), "--weights",
            str(tmp_path / "g.pth"), "--input", str(tmp_path / "series.npy"), "--batch", "2"]
    r = subprocess.run(base + ["--output", str(tmp_path / "out.npy"), "--sub-output", str(tmp_path / "sub.npy"), "--sub-level-dir",
                               str(tmp_path / "sublv"), "--sub-floor", "30", "--sub-ct-min", "-900", "--sub-wc", "100", "--sub-ww",
                               "200", "--mip-dir", str(tmp_path / "mip"), "--mip-source", "sub", "--slab", "3"],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert np.array_equal(np.load(tmp_path / "out.npy"), want["pix"])
    sub = np.load(tmp_path / "sub.npy")
    assert sub.dtype == np.int16 and np.array_equal(sub, want["sub"]) and len(np.unique(sub)) > 50
    assert sorted(os.listdir(tmp_path / "sublv")) == ["%06d.png" % i for i in range(5)]
    for i in range(5):
        img = Image.open(tmp_path / "sublv" / ("%06d.png" % i))
        assert img.mode == "L" and np.array_equal(np.asarray(img), want["sub_level"][i])
    proj = want["projections"]
    assert sorted(os.listdir(tmp_path / "mip")) == ["axial_000.png", "axial_001.png", "coronal.png", "projections.npz", "sagittal.png"]
    for i in range(2):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "mip" / ("axial_%03d.png" % i))), proj["axial"]["level"][i])
    npz = np.load(tmp_path / "mip" / "projections.npz")
    for axis in npz.files:
        assert np.array_equal(npz[axis], proj[axis]["values"])
    assert np.array_equal(npz["axial"], project_np.project(sub, "max", 3)[0])
    # without the new flags the listing is what it was
    r = subprocess.run(base + ["--output", str(tmp_path / "out2.npy")], capture_output=True, text=True, timeout=600,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert np.array_equal(np.load(tmp_path / "out2.npy"), want["pix"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cfg.yaml", "g.pth", "mip", "out.npy", "out2.npy", "series.npy", "sub.npy",
                                                          "sublv"]
