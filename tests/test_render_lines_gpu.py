"""GPU: shaded volume rendering along lines in any direction (ctg_render_lines through ops.render_lines / ops.LightTable;
cta_gan_amd/infer.py: VolumeRenderer, render_lines_volume, SeriesTranslator(render3d=...); predict.py --vr3d-dir) against the numpy
restatement tests/render_lines_np.py, which is a plain loop over the steps of a ray with live and counted masks, and against
ctg_project_render where a line table can express its view.  Exact integer arithmetic: every comparison is np.array_equal, never a
tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_lines_np
from test_reformat_gpu import raw_table
from test_render import TABLES, WC, WW
from test_render_lines import ANGLES, BG, PLANES, hu_like, planted
from test_rotate_gpu import make_generator, synthetic_hu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (3, 5, 7), (5, 13, 11), (6, 19, 37)]      # (6, 19, 37): default cols 43 .. 45, two segments, the last partly live
STOPS = (0, 128)
SURFACES = (1, 16384, 32768)
DTYPES = {"rgb": torch.uint8, "opacity": torch.uint8, "depth": torch.int16}
SENTINEL = {"rgb": 201, "opacity": 77, "depth": -321}
HU_WINDOW = (1000.0, 4300.0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib, ops
    _lib.load()
    return ops


def cpu(t):
    return None if t is None else t.cpu().numpy()


def same(got, want, what=()):
    for p, t in zip(PLANES, got):
        assert t.dtype == DTYPES[p] and tuple(t.shape) == want[p].shape, (p, what)
        assert np.array_equal(cpu(t), want[p]), (p, what)


class Turns:
    """The options that take turns from one call to the next."""

    def __init__(self):
        self.i = 0

    def next(self):
        i = self.i
        self.i += 1
        names = ("mixed", "fog", "opaque", "wild")
        return names[i % 4], STOPS[i % 2], SURFACES[i % 3], bool((i // 2) % 2)


def check_table(ops, vol, dev, made, aspect, window, gmin2, turns, light=None, what=()):
    """Both samplings, shaded and unshaded, of one line table; table, stop, surface and hu take turns.  -> whether any ray met the
    volume (a view of a single voxel may miss it)."""
    from cta_gan_amd.infer import headlight
    lines, steps, u = made[0], made[1], made.cols
    table = ops.LineTable(lines, u, steps)
    light = headlight(made, aspect) if light is None else light
    lamp = ops.LightTable(light, table.count)
    zscale = int(np.floor(256.0 / aspect + 0.5))
    hit = False
    for sampling in ("nearest", "trilinear"):
        for shaded in (False, True):
            name, stop, surface, hu = turns.next()
            kw = dict(sampling=sampling, stop=stop, surface=surface, wc=window[0], ww=window[1], hu=hu)
            want = render_lines_np.render(vol, lines, u, steps, TABLES[name], bg=BG, light=light if shaded else None, zscale=zscale,
                                          ambient=64, gmin2=gmin2, **kw)
            hit = hit or (want["counted"] > 0).any()
            got = ops.render_lines(dev, table, u, steps, TABLES[name], light=lamp if shaded else None, zscale=zscale, ambient=64,
                                   gmin2=gmin2, background=BG, **kw)
            same(got, want, what + (sampling, shaded, name, stop, surface, hu))
    return hit


# ---------------------------------------------------------------------------------------------- 1. one call equals numpy
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_views_of_every_kind_equal_numpy(ops, shape):
    """z orbit, x tumble and an oblique axis at three aspects and two oversamples, on a clamp-heavy and a HU-like volume."""
    from cta_gan_amd.infer import orbit_lines
    n, h, w = shape
    turns, hits = Turns(), []
    for vol, window, gmin2, views in (
            (planted(n, h, w, seed=n * 100 + w), (WC, WW), 1600, (("z", 1.0, 1), ((1, 1, 0), 0.25, 2))),
            (hu_like(shape), HU_WINDOW, 3000 * 3000, (("x", 2.5, 1), ("x", 1.0, 2)))):
        dev = torch.from_numpy(vol).cuda()
        for axis, aspect, s in views:
            made = orbit_lines(n, h, w, [30.0, 200.0], axis=axis, aspect=aspect, oversample=s)
            hits.append(check_table(ops, vol, dev, made, aspect, window, gmin2, turns, what=(shape, axis, aspect, s)))
    assert all(hits) if min(shape) > 1 else any(hits), hits


def test_three_segments_a_ragged_trip_and_a_plain_plane(ops):
    """rows = 3, cols = 70, T = 33: three column segments and a ray that is no multiple of the trip of 32 steps; T = 1 with an
    explicit light, through the same kernel."""
    from cta_gan_amd.infer import LineSet
    shape = (5, 13, 11)
    turns = Turns()
    rng = np.random.RandomState(3)
    for vol, window, gmin2 in ((planted(*shape, seed=9), (WC, WW), 1600), (hu_like(shape), HU_WINDOW, 3000 * 3000)):
        dev = torch.from_numpy(vol).cuda()
        for lines, u, t in ((3, 70, 33), (10, 33, 1)):
            made = LineSet(raw_table(shape, lines, u, t), t, u)
            light = rng.randint(-4096, 4097, size=(lines, 3)) if t == 1 else None
            assert check_table(ops, vol, dev, made, 1.0, window, gmin2, turns, light=light, what=(lines, u, t))


def test_each_plane_alone_and_nothing_else_is_written(ops):
    """Through the raw C ABI into buffers with sentinels behind the planes: every subset of one plane, and all three."""
    from cta_gan_amd import _lib
    from cta_gan_amd.infer import headlight, orbit_lines
    lib = _lib.load()
    vol = hu_like((6, 19, 37))
    n, h, w = vol.shape
    dev = torch.from_numpy(vol).cuda()
    made = orbit_lines(n, h, w, [30.0], axis="x", aspect=2.5)
    lines, steps, u = made[0], made[1], made.cols
    table, lut = ops.LineTable(lines, u, steps), ops.TransferTable(TABLES["mixed"])
    light = headlight(made, 2.5)
    lamp = ops.LightTable(light, table.count)
    want = render_lines_np.render(vol, lines, u, steps, TABLES["mixed"], "trilinear", 128, 16384, BG, *HU_WINDOW, True, light, 102, 64,
                                  3000 * 3000)
    st = torch.cuda.current_stream().cuda_stream
    items = {"rgb": table.count * u * 3, "opacity": table.count * u, "depth": table.count * u}
    for wanted in (("rgb",), ("opacity",), ("depth",), PLANES):
        buf = {p: torch.full((items[p] + 64,), SENTINEL[p], dtype=DTYPES[p], device="cuda") for p in PLANES}
        ptr = {p: buf[p].data_ptr() if p in wanted else None for p in PLANES}
        assert lib.ctg_render_lines(dev.data_ptr(), n, h, w, table.dev.data_ptr(), table.count, u, steps, lut.dev.data_ptr(), 1, 128, 16384,
                                    BG[0], BG[1], BG[2], HU_WINDOW[0], HU_WINDOW[1], 1, lamp.dev.data_ptr(), 102, 64, 3000 * 3000,
                                    ptr["rgb"], ptr["opacity"], ptr["depth"], st) == 0
        torch.cuda.synchronize()
        for p in PLANES:
            got = cpu(buf[p])
            assert (got[items[p]:] == SENTINEL[p]).all(), (wanted, p)
            if p in wanted:
                assert np.array_equal(got[:items[p]], want[p].reshape(-1)), (wanted, p)
            else:
                assert (got == SENTINEL[p]).all(), (wanted, p)
    # the binding leaves out what is not wanted
    rgb, opacity, depth = ops.render_lines(dev, table, u, steps, lut, light=lamp, zscale=102, ambient=64, gmin2=3000 * 3000,
                                           sampling="trilinear", background=BG, wc=HU_WINDOW[0], ww=HU_WINDOW[1], hu=True, want_rgb=False,
                                           want_depth=False)
    assert rgb is None and depth is None and np.array_equal(cpu(opacity), want["opacity"])


# ---------------------------------------------------------------------------------------------- 2. merged kernels as the yardstick
@pytest.mark.parametrize("sampling,rotating", [("nearest", "nearest"), ("trilinear", "bilinear")])
def test_an_orbit_about_z_equals_project_render(ops, sampling, rotating):
    """fz = 0 on every sample of an orbit about z, so trilinear is the bilinear render; ctg_project_render is the parent commit's."""
    from cta_gan_amd.infer import default_detector, orbit_lines, rotation_coefficients
    for shape in ((2, 33, 31), (3, 5, 7)):
        n, h, w = shape
        vol = planted(n, h, w, seed=h)
        dev = torch.from_numpy(vol).cuda()
        d = default_detector(h, w)
        for s in (1, 2):
            made = orbit_lines(n, h, w, ANGLES, axis="z", rows=n, cols=d, depth=d, oversample=s)
            coef = ops.RotateTable([rotation_coefficients(a, h, w, oversample=s) for a in ANGLES])
            for name in ("mixed", "fog"):
                out = {"rgb": torch.empty((len(ANGLES), n, d, 3), dtype=torch.uint8, device="cuda"),
                       "opacity": torch.empty((len(ANGLES), n, d), dtype=torch.uint8, device="cuda"),
                       "depth": torch.empty((len(ANGLES), n, d), dtype=torch.int16, device="cuda")}
                ops.project_render(dev, 0, coef, made[1], TABLES[name], background=BG, wc=WC, ww=WW, sampling=rotating, **out)
                got = ops.render_lines(dev, made[0], d, made[1], TABLES[name], background=BG, wc=WC, ww=WW, sampling=sampling)
                for p, t in zip(PLANES, got):
                    assert torch.equal(t, out[p]), (shape, s, name, p)
                assert len(torch.unique(out["opacity"])) > 3


def test_a_transparent_table_shows_the_background(ops):
    from cta_gan_amd.infer import headlight, orbit_lines
    vol = hu_like()
    made = orbit_lines(*vol.shape, [30.0], axis="x")
    lut = TABLES["mixed"].copy()
    lut[:, 3] = 0
    for light in (None, headlight(made)):
        rgb, opacity, depth = ops.render_lines(torch.from_numpy(vol).cuda(), made[0], made.cols, made[1], lut, light=light, background=BG,
                                               stop=0, surface=1)
        assert (cpu(rgb) == BG).all() and (cpu(opacity) == 0).all() and (cpu(depth) == -1).all()


# ---------------------------------------------------------------------------------------------- 3. wild inputs and refusals
def test_wild_tables_and_refusals_through_the_raw_abi(ops):
    from cta_gan_amd import _lib
    from cta_gan_amd.infer import orbit_lines
    lib = _lib.load()
    vol = planted(5, 13, 11, seed=4)
    n, h, w = vol.shape
    dev = torch.from_numpy(vol).cuda()
    made = orbit_lines(n, h, w, [30.0], axis=(1, 1, 0))
    lines, steps, u = made[0], made[1], made.cols
    table, lut = ops.LineTable(lines, u, steps), ops.TransferTable(TABLES["mixed"])
    count = table.count
    wild = np.random.RandomState(1).choice([2 ** 31 - 1, -(2 ** 31 - 1), 0, 5000, -5000], size=(count, 3)).astype(np.int32)
    wild_dev = torch.from_numpy(wild).cuda()
    lead = tuple(lines.shape[:-1])
    rgb = torch.full(lead + (u, 3), 201, dtype=torch.uint8, device="cuda")
    opacity = torch.full(lead + (u,), 77, dtype=torch.uint8, device="cuda")
    depth = torch.full(lead + (u,), -321, dtype=torch.int16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    P, C, T, G = dev.data_ptr(), table.dev.data_ptr(), lut.dev.data_ptr(), wild_dev.data_ptr()
    R, O, D = rgb.data_ptr(), opacity.data_ptr(), depth.data_ptr()

    def call(vol=P, N=n, H=h, W=w, lines=C, Ln=count, U=u, Tn=steps, lut=T, sampling=1, stop=128, surface=16384, bg=BG, light=G,
             zscale=256, ambient=64, gmin2=1600, rgb=R, opacity=O, depth=D):
        return lib.ctg_render_lines(vol, N, H, W, lines, Ln, U, Tn, lut, sampling, stop, surface, bg[0], bg[1], bg[2], WC, WW, 0, light,
                                    zscale, ambient, gmin2, rgb, opacity, depth, st)

    for kw in (dict(vol=None), dict(lines=None), dict(lut=None), dict(rgb=None, opacity=None, depth=None), dict(N=0), dict(N=4097),
               dict(H=0), dict(H=4097), dict(W=0), dict(W=4097), dict(U=0), dict(U=4097), dict(Tn=0), dict(Tn=4097), dict(Ln=0),
               dict(Ln=-1), dict(sampling=-1), dict(sampling=2), dict(stop=-1), dict(stop=32768), dict(surface=0), dict(surface=32769),
               dict(bg=(256, 0, 0)), dict(bg=(0, -1, 0)), dict(bg=(0, 0, 256)), dict(zscale=0), dict(zscale=4097), dict(ambient=-1),
               dict(ambient=257), dict(gmin2=0), dict(gmin2=(1 << 26) + 1), dict(vol=P + 1), dict(lines=C + 2), dict(lut=T + 1),
               dict(light=G + 2), dict(depth=D + 1), dict(Ln=2 ** 31 - 1, U=33)):
        assert call(**kw) == 1, kw      # CTG_EINVAL
    torch.cuda.synchronize()
    assert (rgb == 201).all() and (opacity == 77).all() and (depth == -321).all()      # nothing was launched
    # light entries of +-(2^31 - 1): the kernel clamps them, and so does the restatement
    assert call() == 0
    want = render_lines_np.render(vol, lines, u, steps, TABLES["mixed"], "trilinear", 128, 16384, BG, WC, WW, False, wild.reshape(
        lines.shape[:-1] + (3,)), 256, 64, 1600)
    assert (want["lit"] > 0).any()
    same((rgb, opacity, depth), want)
    # a table whose every sample misses the volume: the background, whatever the light
    away = lines.copy()
    away[..., 0] += 1 << 27
    away_table = ops.LineTable(away, u, steps)
    assert call(lines=away_table.dev.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (cpu(rgb) == BG).all() and (cpu(opacity) == 0).all() and (cpu(depth) == -1).all()
    # the binding's own refusals
    for kw in (dict(want_rgb=False, want_opacity=False, want_depth=False), dict(sampling="bilinear"), dict(stop=32768), dict(surface=0),
               dict(background=(0, 0)), dict(zscale=0), dict(zscale=4097), dict(ambient=257), dict(ambient=0.3), dict(gmin2=0),
               dict(vol=dev.cpu()), dict(vol=dev.int()), dict(lines=table.dev), dict(u=u + 1), dict(light=wild_dev),
               dict(light=wild.astype(np.int64)), dict(light=np.zeros((count + 1, 3), dtype=np.int64)), dict(lut=lut.dev)):
        args = dict(vol=dev, lines=table, u=u, t=steps, lut=lut)
        args.update(kw)
        with pytest.raises(RuntimeError):
            ops.render_lines(**args)


# ---------------------------------------------------------------------------------------------- 4. the host layer
def tables_for(aspect=1.0):
    from cta_gan_amd.infer import orbit_lines
    return {"tumble": lambda n, h, w: orbit_lines(n, h, w, [0.0, 40.0], axis="x", aspect=aspect),
            "oblique": lambda n, h, w: orbit_lines(n, h, w, [75.0], axis=(1, 1, 0), aspect=aspect, oversample=2)}


def check_views(got, vol, tables, lut, sampling, window, hu, shading, aspect, depth=True):
    from cta_gan_amd.infer import headlight
    assert sorted(got) == sorted(tables)
    for name, d in got.items():
        made = tables[name](*vol.shape)
        kw = {}
        if shading is not None:
            kw = dict(light=headlight(made, aspect), zscale=int(np.floor(256.0 / aspect + 0.5)), ambient=shading[0], gmin2=shading[1])
        want = render_lines_np.render(vol, made[0], made.cols, made[1], lut, sampling, 128, 16384, (0, 0, 0), window[0], window[1], hu, **kw)
        assert (want["counted"] > 0).any()
        for p in PLANES:
            plane = d[p]
            if p == "depth" and not depth:
                assert plane is None
                continue
            plane = plane.cpu().numpy() if torch.is_tensor(plane) else plane
            assert plane.dtype == want[p].dtype and np.array_equal(plane, want[p]), (name, p)


def test_volume_renderer_in_shuffled_chunks_and_render_lines_volume(ops, monkeypatch):
    from cta_gan_amd.infer import VolumeRenderer, render_lines_volume
    vol = hu_like((7, 19, 23), seed=3)
    n, h, w = vol.shape
    dev = torch.from_numpy(vol).cuda()
    tables = tables_for(aspect=2.5)
    calls = []
    monkeypatch.setattr(ops, "render_lines", (lambda f: lambda *a, **k: (calls.append("render_lines"), f(*a, **k))[1])(ops.render_lines))
    options = dict(transfer=TABLES["mixed"], wc=HU_WINDOW[0], ww=HU_WINDOW[1], hu=True, shading={"ambient": 0.25, "gmin": 3000}, aspect=2.5)
    view = VolumeRenderer(n, h, w, tables, **options)
    nbytes = view.nbytes
    assert view.volume is None and nbytes > 2 * vol.size      # known before the first chunk
    for s in (4, 0, 6, 2):      # chunks of 2 (the last of 1) in shuffled order
        view.update(dev[s:s + 2], s)
        if s != 2:
            with pytest.raises(RuntimeError, match="exactly once"):
                view.result()
    view.update(dev[:0], 0)      # an empty chunk changes nothing
    assert not calls
    got = view.result()
    assert calls == ["render_lines"] * 2 and view.nbytes == nbytes      # one launch per table
    assert all(t.is_cuda for d in got.values() for t in d.values())
    check_views(got, vol, tables, TABLES["mixed"], "trilinear", HU_WINDOW, True, (64, 3000 * 3000), 2.5)
    whole = render_lines_volume(dev, tables, **options)
    for name in tables:
        assert all(torch.equal(whole[name][p], got[name][p]) for p in PLANES)
    view.update(dev[:2], 0)      # a slice twice
    with pytest.raises(RuntimeError, match="exactly once"):
        view.result()
    view.reset()
    view.update(dev, 0)
    assert torch.equal(view.result()["tumble"]["rgb"], got["tumble"]["rgb"])
    with pytest.raises(RuntimeError):
        view.update(dev, 1)
    got = render_lines_volume(vol, tables_for(), batch=3, transfer=TABLES["fog"], sampling="nearest", depth=False)      # a host array
    assert all(isinstance(d["rgb"], np.ndarray) for d in got.values())
    check_views(got, vol, tables_for(), TABLES["fog"], "nearest", (300.0, 1500.0), False, None, 1.0, depth=False)
    got = render_lines_volume(torch.from_numpy(vol), tables_for(), transfer=TABLES["fog"])
    assert torch.is_tensor(got["tumble"]["rgb"]) and not got["tumble"]["rgb"].is_cuda      # a CPU tensor returns tensors
    check_views(got, vol, tables_for(), TABLES["fog"], "trilinear", (300.0, 1500.0), False, None, 1.0)
    with pytest.raises(RuntimeError):
        render_lines_volume(vol.astype(np.int32), tables)


def test_series_translator_render3d(ops, monkeypatch):
    from cta_gan_amd import _lib, nets
    from cta_gan_amd.infer import SeriesTranslator
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        g = make_generator()
        vol = synthetic_hu(5, 64, 64, seed=7)
        launched = set()
        monkeypatch.setattr(_lib, "check", (lambda f: lambda status, what: (launched.add(what), f(status, what))[1])(_lib.check))
        plain_tr = SeriesTranslator(g, batch=2, rotate=3)
        plain_tr(vol)      # (the generator's first forward also packs its weights)
        launched.clear()
        plain = plain_tr(vol)
        before = set(launched)
        launched.clear()
        none_tr = SeriesTranslator(g, batch=2, rotate=3, render3d=None)
        none = none_tr(vol)
        # with render3d=None the result and the launches are what they were, and nothing is kept
        assert sorted(none) == sorted(plain) == ["level", "pix", "rotation"] and launched == before and "ctg_render_lines" not in before
        assert "render3d" not in none_tr._views and "render3d" not in none_tr._view_host and "render3d" not in plain_tr._views
        tables = tables_for()
        options = {"transfer": TABLES["mixed"], "wc": 300.0, "ww": 3000.0, "shading": {"ambient": 0.25, "gmin": 20}}
        tr = SeriesTranslator(g, batch=2, rotate=3, render3d=tables, render3d_options=options)
        launched.clear()
        for out in (tr(vol), tr(vol)):      # the second call reuses the renderer and the page-locked planes
            assert np.array_equal(out["pix"], plain["pix"]) and np.array_equal(out["level"], plain["level"])
            assert np.array_equal(out["rotation"]["values"], plain["rotation"]["values"])
            check_views(out["render3d"], out["pix"], tables, TABLES["mixed"], "trilinear", (300.0, 3000.0), False, (64, 400), 1.0)
        assert launched == before | {"ctg_render_lines"}
        whole = SeriesTranslator(g, batch=2, hu=True, subtract=True, project_source="sub", render3d=tables,
                                 render3d_options={"transfer": TABLES["fog"], "wc": 0.0, "ww": 600.0})(torch.from_numpy(vol))
        assert all(torch.is_tensor(t) for d in whole["render3d"].values() for t in d.values())
        check_views(whole["render3d"], whole["sub"].numpy(), tables, TABLES["fog"], "trilinear", (0.0, 600.0), True, None, 1.0)
    finally:
        nets.set_default_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------- 5. predict.py
def test_predict_command_line_vr3d(ops, tmp_path):
    from PIL import Image
    from cta_gan_amd.infer import TRANSFER_PRESETS, headlight, orbit_lines, transfer_function, view_angles
    vol = synthetic_hu(6, 48, 40, seed=9)
    np.save(tmp_path / "series.npy", vol)
    (tmp_path / "cfg.yaml").write_text("name: HdGan\nsize: 64\ninput_nc: 1\noutput_nc: 1\n")
    torch.save(make_generator(seed=3).state_dict(), tmp_path / "g.pth")
    cmd = [sys.executable, os.path.join(ROOT, "predict.py"), "--config", str(tmp_path / "cfg.yaml"), "--weights",
           str(tmp_path / "g.pth"), "--input", str(tmp_path / "series.npy"), "--batch", "4", "--output", str(tmp_path / "out.npy"),
           "--aspect", "2.5", "--vr3d-dir", str(tmp_path / "vr3d"), "--vr-angles", "3", "--vr-span", "180", "--vr-preset", "grey",
           "--vr-wc", "1000", "--vr-ww", "4200", "--vr-oversample", "2", "--vr-background", "10,200,30", "--vr3d-shade",
           "--vr3d-ambient", "0.25", "--vr3d-gmin", "20"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    pix = np.load(tmp_path / "out.npy")
    n, h, w = pix.shape
    angles = view_angles(3, 180.0)
    made = orbit_lines(n, h, w, angles, axis="x", oversample=2, aspect=2.5)
    lut = transfer_function(TRANSFER_PRESETS["grey"], 2)
    light = headlight(made, 2.5)
    assert sorted(os.listdir(tmp_path / "vr3d")) == sorted(["vr3d_%03d.png" % i for i in range(3)] + ["render3d.npz"])
    npz = np.load(tmp_path / "vr3d" / "render3d.npz")
    assert sorted(npz.files) == ["angles", "depth", "light", "lines", "lut", "opacity", "rgb"]
    want = render_lines_np.render(pix, made[0], made.cols, made[1], lut, "trilinear", 128, 16384, (10, 200, 30), 1000.0, 4200.0, False,
                                  light, 102, 64, 400)
    assert (want["counted"] > 0).any() and (want["opacity"] > 0).any()
    for p in PLANES:
        assert npz[p].dtype == want[p].dtype and np.array_equal(npz[p], want[p]), p
    assert npz["angles"].tolist() == angles and np.array_equal(npz["lut"], lut)
    assert np.array_equal(npz["lines"], made[0]) and np.array_equal(npz["light"], light)
    for i in range(3):
        img = Image.open(tmp_path / "vr3d" / ("vr3d_%03d.png" % i))
        assert img.mode == "RGB" and np.array_equal(np.asarray(img), npz["rgb"][i])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cfg.yaml", "g.pth", "out.npy", "series.npy", "vr3d"]
