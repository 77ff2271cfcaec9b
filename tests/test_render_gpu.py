"""GPU: the volume-rendered rotating views (ctg_project_render through ops.project_render / ops.TransferTable;
cta_gan_amd/infer.py: SeriesRenderer, render_volume, SeriesTranslator(render=...); predict.py --vr-dir) against the numpy
restatement tests/render_np.py, which has no lanes, trips or packed alphas.  Exact integer arithmetic: every comparison is
np.array_equal, never a tolerance."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_np
import rotate_lerp_np
import rotate_np
from test_depth_gpu import PAIRS
from test_render import TABLES, WC, WW
from test_rotate_gpu import ANGLES, make_generator, planted, synthetic_hu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("rgb", "opacity", "depth")
DTYPES = {"rgb": torch.uint8, "opacity": torch.uint8, "depth": torch.int16}
SENTINEL = {"rgb": 201, "opacity": 77, "depth": -321}
BG = (10, 200, 30)
STOPS = (0, 128)
SURFACES = (1, 16384, 32768)
ONE = 32768

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


def table(h, w, u, t, s=1, angles=ANGLES):
    return np.array([rotate_lerp_np.coefficients(a, h, w, u, t, s) for a in angles], dtype=np.int64)


def sentinels(a, n, u, which=PLANES):
    return {p: torch.full((a, n, u, 3) if p == "rgb" else (a, n, u), SENTINEL[p], dtype=DTYPES[p], device="cuda") if p in which
            else None for p in PLANES}


def run(ops, dev, n0, coef, lut, n, u, steps, out=None, which=PLANES, **kw):
    """One ops.project_render call into fresh (or the given) planes -> {plane: numpy or None}."""
    if out is None:
        out = sentinels(len(coef.host) if hasattr(coef, "host") else len(coef), n, u, which)
    kw.setdefault("wc", WC)
    kw.setdefault("ww", WW)
    ops.project_render(dev, n0, coef, steps, lut, **out, **kw)
    return {p: None if t is None else cpu(t) for p, t in out.items()}


def same(got, want, what=()):
    for p in PLANES:
        assert got[p].dtype == want[p].dtype and np.array_equal(got[p], want[p]), (p,) + tuple(what)


# ---------------------------------------------------------------------------------------------- 1. one call equals numpy
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 33, 31), (2, 37, 53), (4, 19, 515)]
CASES = [(shape, sampling, s) for shape in SHAPES for sampling in ("nearest", "bilinear") for s in (1, 2)
         if not (shape == (4, 19, 515) and s == 2)]      # three detector segments: at one step per voxel only


@pytest.mark.parametrize("shape,sampling,oversample", CASES, ids=lambda v: "%dx%dx%d" % v if isinstance(v, tuple) else str(v))
def test_project_render_equals_numpy(ops, shape, sampling, oversample):
    """Both detectors, all ANGLES, hu both ways, every table, both stops; the three surfaces take turns (a surface moves the depth
    plane alone).  The conditions are read from the oracle at the default detector, where the rays of one call range from ones
    that miss the slice to ones that cross its diagonal; with the detector (w, h) nearly every ray crosses the whole slice."""
    n, h, w = shape
    vol = planted(n, h, w, seed=n * 1000 + w)
    dev = torch.from_numpy(vol).cuda()
    d = rotate_np.detector(h, w)
    names = ("mixed", "fog") if shape == (4, 19, 515) else ("mixed", "fog", "opaque", "wild")
    luts = {name: ops.TransferTable(TABLES[name]) for name in names}
    turn = 0
    for u, t in ((d, d), (w, h)):
        steps = t * oversample
        coef = table(h, w, u, t, oversample)
        tab = ops.RotateTable(coef)
        for hu in (False, True):
            cls, ok = render_np.classes(vol, coef, u, steps, sampling, WC, WW, hu)
            for name in names:
                fog = {}
                for stop in STOPS:
                    surface = SURFACES[turn % 3]
                    turn += 1
                    want = render_np.composite(cls, ok, TABLES[name], stop, surface, BG)
                    got = run(ops, dev, 0, tab, luts[name], n, u, steps, background=BG, stop=stop, surface=surface, hu=hu,
                              sampling=sampling)
                    same(got, want, (u, t, hu, name, stop, surface))
                    early = want["taken"] < want["counted"]
                    whole = (want["taken"] == want["counted"]) & (want["counted"] > 0)
                    if name == "mixed" and (u, t) == (d, d) and shape != (1, 1, 1):      # (one voxel: one class a ray)
                        assert early.any() and whole.any() and (want["depth"] == -1).any() and (want["depth"] >= 0).any()
                    if name == "fog":
                        fog[stop] = (want, early)
                if name == "fog":
                    assert not fog[0][1].any()      # wgt < Tr below an opaque alpha: Tr never reaches 0
                    if (u, t) == (d, d) and shape in ((2, 33, 31), (2, 37, 53), (4, 19, 515)):      # rays long enough for the threshold
                        assert fog[128][1].any() and not np.array_equal(fog[0][0]["rgb"], fog[128][0]["rgb"])
    if shape == (4, 19, 515):
        assert d == 516      # 17 workgroups of 32 columns a slice and angle, the last with 4 live columns


def test_a_host_table_serves_as_well_as_an_uploaded_one(ops):
    n, h, w = 3, 5, 7
    vol = planted(n, h, w, seed=1)
    dev = torch.from_numpy(vol).cuda()
    d = rotate_np.detector(h, w)
    coef = table(h, w, d, d)
    want = render_np.render(vol, coef, d, d, TABLES["mixed"], "nearest", 128, 16384, (0, 0, 0), 50.0, 400.0)
    out = sentinels(len(coef), n, d)
    ops.project_render(dev, 0, coef, d, TABLES["mixed"], **out)      # the defaults: black, stop 128, surface 16384, window (50, 400)
    same({p: cpu(t) for p, t in out.items()}, want)
    got = run(ops, dev, 0, torch.from_numpy(coef), torch.from_numpy(TABLES["mixed"].astype(np.int32)), n, d, d, wc=50.0, ww=400.0)
    same(got, want)


# ---------------------------------------------------------------------------------------------- 2. order
@pytest.mark.parametrize("sampling", ["nearest", "bilinear"])
def test_the_nearer_of_two_opaque_voxels_is_the_one_shown(ops, sampling):
    """U = W, T = H: at 0 degrees sample (u, t) is pixel (u, t), at 180 degrees pixel (W-1-u, H-1-t): the far one becomes the near
    one.  Slice 0 has red in front of green (seen from 0 degrees), slice 1 green in front of red; everything else is transparent."""
    n, h, w = 2, 37, 53
    vol = np.random.RandomState(11).randint(-32768, -25000, size=(n, h, w)).astype(np.int16)
    red, green = 10000, 20000
    cr, cg = int(rotate_np.level(np.array([red]), WC, WW)[0]), int(rotate_np.level(np.array([green]), WC, WW)[0])
    assert rotate_np.level(vol, WC, WW).max() == 0 and 0 < cr < cg
    lut = np.zeros((256, 4), dtype=np.uint16)
    lut[cr], lut[cg] = (255, 0, 0, ONE), (0, 255, 0, ONE)
    for (r0, r1), c in PAIRS:
        vol[0, r0, c], vol[0, r1, c] = red, green
        vol[1, r0, c], vol[1, r1, c] = green, red
    coef = table(h, w, w, h, angles=[0, 180])
    assert coef[0].tolist() == [32768, 65536, 0, 32768, 0, 65536] and coef[1, 1] == -65536 and coef[1, 5] == -65536
    got = run(ops, torch.from_numpy(vol).cuda(), 0, coef, lut, n, w, h, sampling=sampling, background=BG, stop=0, surface=ONE)
    same(got, render_np.render(vol, coef, w, h, lut, sampling, 0, ONE, BG, WC, WW))
    R, G = [255, 0, 0], [0, 255, 0]
    for (r0, r1), c in PAIRS:
        assert got["rgb"][0, 0, c].tolist() == R and got["depth"][0, 0, c] == r0, (r0, r1)
        assert got["rgb"][1, 0, w - 1 - c].tolist() == G and got["depth"][1, 0, w - 1 - c] == h - 1 - r1, (r0, r1)
        assert got["rgb"][0, 1, c].tolist() == G and got["rgb"][1, 1, w - 1 - c].tolist() == R
        assert got["opacity"][0, 0, c] == 255 and got["opacity"][1, 1, w - 1 - c] == 255
    hit = np.zeros((2, n, w), dtype=bool)
    for _, c in PAIRS:
        hit[0, :, c] = hit[1, :, w - 1 - c] = True
    assert (got["rgb"][~hit] == BG).all() and (got["opacity"][~hit] == 0).all() and (got["depth"][~hit] == -1).all()


# ---------------------------------------------------------------------------------------------- 3. chunks, views, rows, outputs
@pytest.fixture(scope="module")
def volume7():
    return planted(7, 33, 31, seed=77)


@pytest.fixture(scope="module")
def whole7(volume7):
    """The oracle's planes of volume7 under every table: bilinear, the default detector, ANGLES, stop 128, surface 16384."""
    n, h, w = volume7.shape
    d = rotate_np.detector(h, w)
    cls, ok = render_np.classes(volume7, table(h, w, d, d), d, d, "bilinear", WC, WW)
    return {name: render_np.composite(cls, ok, lut, 128, 16384, BG) for name, lut in TABLES.items()}


def test_chunks_in_any_order_a_two_byte_aligned_view_and_the_rows_written(ops, volume7, whole7):
    n, h, w = volume7.shape
    d = rotate_np.detector(h, w)
    tab = ops.RotateTable(table(h, w, d, d))
    lut = ops.TransferTable(TABLES["mixed"])
    kw = dict(sampling="bilinear", background=BG)
    dev = torch.from_numpy(volume7).cuda()
    whole = run(ops, dev, 0, tab, lut, n, d, d, **kw)
    same(whole, whole7["mixed"])
    out = sentinels(len(tab), n, d)
    for s in (4, 0, 6, 2):      # chunks of 2 (the last of 1) in shuffled order: every call writes its own rows
        got = run(ops, dev[s:s + 2], s, tab, lut, n, d, d, out=out, **kw)
    same(got, whole)
    buf = torch.empty(n * h * w + 1, dtype=torch.int16, device="cuda")      # one element into a buffer: only 2-byte aligned
    shifted = buf[1:].view(n, h, w)
    shifted.copy_(dev)
    assert shifted.is_contiguous() and shifted.data_ptr() % 4 == 2
    same(run(ops, shifted, 0, tab, lut, n, d, d, **kw), whole)
    got = run(ops, dev[2:4], 2, tab, lut, n, d, d, **kw)      # rows outside n0 .. n0+K-1 keep the sentinel
    for p in PLANES:
        assert np.array_equal(got[p][:, 2:4], whole[p][:, 2:4]) and (got[p][:, :2] == SENTINEL[p]).all() \
            and (got[p][:, 4:] == SENTINEL[p]).all(), p


def test_any_subset_of_the_outputs_and_a_wild_table(ops, volume7, whole7):
    n, h, w = volume7.shape
    d = rotate_np.detector(h, w)
    tab = ops.RotateTable(table(h, w, d, d))
    dev = torch.from_numpy(volume7).cuda()
    kw = dict(sampling="bilinear", background=BG)
    for r in range(1, 4):
        for which in itertools.combinations(PLANES, r):
            got = run(ops, dev, 0, tab, TABLES["fog"], n, d, d, which=which, **kw)
            for p in PLANES:
                assert (got[p] is None) if p not in which else np.array_equal(got[p], whole7["fog"][p]), (which, p)
    got = run(ops, dev, 0, tab, TABLES["wild"], n, d, d, **kw)      # 65535 everywhere reads as white and opaque
    same(got, whole7["wild"])
    clamped = np.empty((256, 4), dtype=np.uint16)
    clamped[:, :3], clamped[:, 3] = 255, ONE
    same(run(ops, dev, 0, tab, clamped, n, d, d, **kw), got)
    seen = whole7["wild"]["counted"] > 0
    assert (got["rgb"][seen] == 255).all() and (got["opacity"][seen] == 255).all() and (got["rgb"][~seen] == BG).all()


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_launch_nothing(ops, volume7):
    from cta_gan_amd import _lib
    n, h, w = volume7.shape
    d = rotate_np.detector(h, w)
    tab = ops.RotateTable(table(h, w, d, d, angles=[0, 30]))
    lut = ops.TransferTable(TABLES["mixed"])
    dev = torch.from_numpy(volume7).cuda()
    out = sentinels(2, n, d)
    for kw in (dict(rgb=None, opacity=None, depth=None), dict(stop=-1), dict(stop=32768), dict(stop=1.5), dict(surface=0),
               dict(surface=32769), dict(background=(0, 0, 256)), dict(background=(0, -1, 0)), dict(background=(0, 0)),
               dict(sampling="cubic"), dict(sampling=2), dict(t=4097), dict(t=0), dict(n0=1), dict(n0=-1), dict(pix=dev.cpu()),
               dict(pix=dev.int()), dict(depth=out["depth"].int()), dict(opacity=out["opacity"][:1]), dict(rgb=out["opacity"]),
               dict(rgb=out["rgb"][..., :2]), dict(lut=TABLES["mixed"][:255]), dict(lut=TABLES["mixed"].astype(np.float32)),
               dict(lut=lut.dev), dict(coef=tab.dev)):
        args = dict(pix=dev, n0=0, coef=tab, t=d, lut=lut, **out)
        args.update(kw)
        with pytest.raises(RuntimeError):
            ops.project_render(**args)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    P, C, L = dev.data_ptr(), tab.dev.data_ptr(), lut.dev.data_ptr()
    RGB, O, D = (out[p].data_ptr() for p in PLANES)

    def call(K=n, T=d, n0=0, lut=L, sampling=0, stop=128, surface=16384, bg=(0, 0, 0), rgb=RGB, opacity=O, depth=D, pix=P):
        return lib.ctg_project_render(pix, K, h, w, n0, n, C, 2, d, T, lut, sampling, stop, surface, bg[0], bg[1], bg[2], 50.0,
                                      400.0, 0, rgb, opacity, depth, st)

    for kw in (dict(rgb=None, opacity=None, depth=None), dict(stop=-1), dict(stop=32768), dict(surface=0), dict(surface=32769),
               dict(bg=(256, 0, 0)), dict(bg=(0, 256, 0)), dict(bg=(0, 0, 256)), dict(bg=(0, 0, -1)), dict(sampling=2),
               dict(sampling=-1), dict(T=4097), dict(T=0), dict(K=n + 1), dict(K=0), dict(n0=1), dict(depth=D + 1), dict(lut=L + 1),
               dict(lut=None), dict(pix=None), dict(pix=P + 1)):
        assert call(**kw) == 1, kw      # CTG_EINVAL
    torch.cuda.synchronize()
    assert all((out[p] == SENTINEL[p]).all() for p in PLANES)      # nothing was launched
    assert call() == 0 and call(rgb=None, opacity=None) == 0 and call(stop=0, surface=32768, bg=(255, 255, 255), sampling=1) == 0
    torch.cuda.synchronize()
    assert not (out["depth"] == SENTINEL["depth"]).any()


# ---------------------------------------------------------------------------------------------- 5. the host layer
def check_render(ren, pix, angles, lut, sampling="nearest", oversample=1, stop=128, surface=16384, bg=(0, 0, 0), wc=300.0, ww=1500.0,
                 hu=False, depth=True):
    n, h, w = pix.shape
    d = rotate_np.detector(h, w)
    want = render_np.render(pix, table(h, w, d, d, oversample, angles), d, d * oversample, lut, sampling, stop, surface, bg, wc, ww, hu)
    assert sorted(ren) == sorted(["angles", "opacity", "rgb"] + (["depth"] if depth else []))
    got = {k: np.asarray(t.cpu() if torch.is_tensor(t) else t) for k, t in ren.items()}
    assert got["angles"].dtype == np.float64 and got["angles"].tolist() == [float(a) for a in angles]
    assert got["rgb"].shape == (len(angles), n, d, 3)
    for p in PLANES if depth else PLANES[:2]:
        assert got[p].dtype == want[p].dtype and np.array_equal(got[p], want[p]), p
    return want


def test_series_renderer_and_render_volume(ops, monkeypatch):
    from cta_gan_amd.infer import TRANSFER_PRESETS, SeriesRenderer, render_volume, transfer_function, view_angles
    vol = planted(5, 19, 23, seed=3)
    n, h, w = vol.shape
    dev = torch.from_numpy(vol).cuda()
    angles = view_angles(4, span=180.0, start=15.0)
    calls = []
    monkeypatch.setattr(ops, "project_render", (lambda f: lambda *a, **k: (calls.append("project_render"), f(*a, **k))[1])(ops.project_render))
    r = SeriesRenderer(n, h, w, angles, transfer=TABLES["mixed"], wc=WC, ww=WW, hu=True, sampling="bilinear", background=BG, stop=0,
                       surface=ONE)
    r.update(dev[3:], 3)
    r.update(dev[:3], 0)
    r.update(dev[:0], 0)      # an empty chunk launches nothing
    assert calls == ["project_render"] * 2      # one launch per chunk
    check_render(r.result(), vol, angles, TABLES["mixed"], "bilinear", 1, 0, ONE, BG, WC, WW, True)
    assert r.lut.dev.dtype == torch.uint16 and tuple(r.lut.dev.shape) == (256, 4) and np.array_equal(r.lut.host, TABLES["mixed"])
    r.reset()
    with pytest.raises(RuntimeError):
        r.update(dev, 1)
    # a point list and a preset name go through transfer_function with the renderer's oversample; depth=False drops the plane
    points = [(0, 0, 0, 0, 0.0), (120, 200, 30, 20, 0.1), (255, 255, 255, 255, 0.9)]
    r = SeriesRenderer(n, h, w, angles, transfer=points, wc=WC, ww=WW, oversample=2, depth=False)
    r.update(dev, 0)
    assert r.depth_plane is None and r.steps == 2 * r.t
    check_render(r.result(), vol, angles, transfer_function(points, 2), "nearest", 2, wc=WC, ww=WW, depth=False)
    got = render_volume(vol, angles, batch=2, transfer="bone", wc=WC, ww=WW, oversample=2, sampling="bilinear")
    assert all(isinstance(t, np.ndarray) for t in got.values())
    want = check_render(got, vol, angles, transfer_function(TRANSFER_PRESETS["bone"], 2), "bilinear", 2, wc=WC, ww=WW)
    assert (want["opacity"] > 0).any() and (want["depth"] >= 0).any()
    got = render_volume(torch.from_numpy(vol), 3, batch=4, transfer=TABLES["fog"], wc=WC, ww=WW, background=BG)
    assert all(torch.is_tensor(t) and not t.is_cuda for t in got.values())
    check_render(got, vol, view_angles(3), TABLES["fog"], bg=BG, wc=WC, ww=WW)
    got = render_volume(dev, [0.0, 33.5], transfer=TABLES["mixed"], wc=WC, ww=WW)
    assert all(t.is_cuda for t in got.values())
    check_render(got, vol, [0.0, 33.5], TABLES["mixed"], wc=WC, ww=WW)
    with pytest.raises(RuntimeError):
        render_volume(vol.astype(np.int32), 3)


def test_series_translator_render(ops, monkeypatch):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator, view_angles
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        g = make_generator()
        vol = synthetic_hu(5, 64, 64, seed=7)
        calls = []
        monkeypatch.setattr(ops, "project_render", (lambda f: lambda *a, **k: (calls.append("project_render"), f(*a, **k))[1])(ops.project_render))
        plain_tr = SeriesTranslator(g, batch=2, rotate=3)
        plain = plain_tr(vol)
        assert "render" not in plain and not calls and "render" not in plain_tr._views and "render" not in plain_tr._view_host
        options = {"transfer": TABLES["mixed"], "wc": 1000.0, "ww": 4200.0, "background": BG}      # stored values 0 .. 4095
        tr = SeriesTranslator(g, batch=2, rotate=3, render=3, render_options=options)
        for out in (tr(vol), tr(vol)):      # the second call reuses the renderer and the page-locked planes
            assert np.array_equal(out["pix"], plain["pix"]) and np.array_equal(out["level"], plain["level"])
            assert np.array_equal(out["rotation"]["values"], plain["rotation"]["values"])
            want = check_render(out["render"], out["pix"], view_angles(3), TABLES["mixed"], bg=BG, wc=1000.0, ww=4200.0)
            assert (want["opacity"] > 0).any()
        assert calls == ["project_render"] * 6      # one launch per chunk
        out = SeriesTranslator(g, batch=2, hu=True, subtract=True, project_source="sub", render=[0.0, 33.5],
                               render_options={"transfer": TABLES["fog"], "wc": 0.0, "ww": 3000.0, "sampling": "bilinear",
                                               "depth": False})(torch.from_numpy(vol))
        assert all(torch.is_tensor(t) for t in out["render"].values())
        want = check_render(out["render"], out["sub"].numpy(), [0.0, 33.5], TABLES["fog"], "bilinear", wc=0.0, ww=3000.0, hu=True,
                            depth=False)      # a subtraction value is a HU difference: hu=True whatever the translator's own
        assert (want["opacity"] > 0).any()
    finally:
        nets.set_default_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------- 6. predict.py --vr-dir
def test_predict_command_line_render(ops, tmp_path):
    from PIL import Image
    from cta_gan_amd.infer import TRANSFER_PRESETS, transfer_function
    vol = synthetic_hu(5, 48, 40, seed=9)
    np.save(tmp_path / "series.npy", vol)
    (tmp_path / "cfg.yaml").write_text("name: HdGan\nsize: 64\ninput_nc: 1\noutput_nc: 1\n")
    torch.save(make_generator(seed=3).state_dict(), tmp_path / "g.pth")
    cmd = [sys.executable, os.path.join(ROOT, "predict.py"), "--config", str(tmp_path / "cfg.yaml"), "--weights",
           str(tmp_path / "g.pth"), "--input", str(tmp_path / "series.npy"), "--batch", "2", "--output", str(tmp_path / "out.npy"),
           "--vr-dir", str(tmp_path / "vr"), "--vr-angles", "4", "--vr-span", "180", "--vr-preset", "grey", "--vr-wc", "1000",
           "--vr-ww", "4200", "--vr-sampling", "bilinear", "--vr-oversample", "2", "--vr-background", "10,200,30", "--aspect", "1.5"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    pix = np.load(tmp_path / "out.npy")
    assert sorted(os.listdir(tmp_path / "vr")) == ["render.npz"] + ["vr_%03d.png" % i for i in range(4)]
    npz = np.load(tmp_path / "vr" / "render.npz")
    assert sorted(npz.files) == ["angles", "depth", "lut", "opacity", "rgb"]
    lut = transfer_function(TRANSFER_PRESETS["grey"], 2)
    assert npz["lut"].dtype == np.uint16 and np.array_equal(npz["lut"], lut)
    want = check_render({k: npz[k] for k in npz.files if k != "lut"}, pix, [0.0, 45.0, 90.0, 135.0], lut, "bilinear", 2, bg=BG,
                        wc=1000.0, ww=4200.0)
    assert (want["opacity"] > 0).any()
    from cta_gan_amd.infer import aspect_rows
    img = Image.open(tmp_path / "vr" / "vr_000.png")
    assert img.mode == "RGB" and np.array_equal(np.asarray(img), npz["rgb"][0][aspect_rows(5, 1.5)])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cfg.yaml", "g.pth", "out.npy", "series.npy", "vr"]
