"""CPU: the shaded volume rendering along lines in any direction without a GPU -- the pins of the numpy restatement
tests/render_lines_np.py that the GPU tests lean on (the z orbit reproduces the rotating render, shading switched off, the ramps,
the HU-like volume), cta_gan_amd/infer.py: headlight / line_voxel / VolumeRenderer's host checks, ops.light_table_host, the entry
point's signature and predict.py's --vr3d flags.  Also home of the HU-like volume the GPU file renders (hu_like)."""
import os
import sys

import numpy as np
import pytest

import reformat_np
import render_lines_np
import render_np
from test_render import TABLES, WC, WW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLES = [0, 90, 180, 270, 45, 10, 137.5, -30, 359.9]
ONE = 32768
BG = (10, 200, 30)
PLANES = ("rgb", "opacity", "depth")


def planted(n, h, w, seed):
    """Random int16 with both extremes planted; the last slice is all 32767 when there are several."""
    vol = np.random.RandomState(seed).randint(-32768, 32768, size=(n, h, w)).astype(np.int16)
    vol[0, 0, 0], vol[0, h - 1, w - 1], vol[n // 2, h // 2, w // 2] = -32768, 32767, -32768
    if n > 2:
        vol[n - 1] = 32767
    return vol


def hu_like(shape=(5, 13, 11), seed=7):
    return np.random.RandomState(seed).randint(-1100, 3200, size=shape).astype(np.int16)


def same(got, want, what=""):
    for p in PLANES:
        assert got[p].dtype == want[p].dtype and np.array_equal(got[p], want[p]), (p, what)


# ---------------------------------------------------------------------------------------------- 1. the oracle's pins
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (2, 33, 31)], ids=lambda s: "%dx%dx%d" % s)
def test_oracle_the_z_orbit_reproduces_the_rotating_render(shape):
    from cta_gan_amd.infer import default_detector, orbit_lines, rotation_coefficients
    n, h, w = shape
    vol = planted(n, h, w, seed=h)
    d = default_detector(h, w)
    made = orbit_lines(n, h, w, ANGLES, axis="z", rows=n, cols=d, depth=d)
    coef = np.array([rotation_coefficients(a, h, w) for a in ANGLES], dtype=np.int64)
    for name in ("mixed", "fog"):
        for mine, theirs in (("nearest", "nearest"), ("trilinear", "bilinear")):      # fz = 0: the trilinear value is the bilinear one
            got = render_lines_np.render(vol, made[0], made.cols, made[1], TABLES[name], mine, 128, 16384, BG, WC, WW)
            want = render_np.render(vol, coef, d, d, TABLES[name], theirs, 128, 16384, BG, WC, WW)
            same(got, want, (name, mine))
            assert np.array_equal(got["tr"], want["tr"]) and np.array_equal(got["taken"], want["taken"])
            assert (got["lit"] == 0).all() and (got["gated"] == 0).all()


def hu_case(aspect, **options):
    from cta_gan_amd.infer import headlight, orbit_lines
    vol = hu_like()
    made = orbit_lines(*vol.shape, [0, 30, 90, 200], axis="x", aspect=aspect)
    kw = dict(sampling="trilinear", stop=128, surface=16384, bg=BG, wc=1000.0, ww=4300.0, hu=True)
    kw.update(options)
    flat = render_lines_np.render(vol, made[0], made.cols, made[1], TABLES["mixed"], **kw)
    return vol, made, headlight(made, aspect), kw, flat


@pytest.mark.parametrize("aspect", [1.0, 2.5])
def test_oracle_shading_switched_off_equals_unshaded(aspect):
    vol, made, light, kw, flat = hu_case(aspect)
    zscale = int(np.floor(256.0 / aspect + 0.5))
    for off in ({"ambient": 256, "gmin2": 1}, {"ambient": 0, "gmin2": 1 << 26}):
        got = render_lines_np.render(vol, made[0], made.cols, made[1], TABLES["mixed"], light=light, zscale=zscale, **off, **kw)
        same(got, flat, off)


def ramp_case(axis, step, shape=(4, 6, 9)):
    from cta_gan_amd.infer import orbit_lines
    vol = (np.arange(shape[axis], dtype=np.int64) * step).reshape([-1 if a == axis else 1 for a in range(3)])
    vol = np.ascontiguousarray(np.broadcast_to(vol, shape)).astype(np.int16)
    lut = np.empty((256, 4), dtype=np.uint16)
    lut[:, :3], lut[:, 3] = (200, 255, 7), ONE
    made = orbit_lines(*shape, [0, 30, 90], axis="x")
    return vol, lut, made


def test_oracle_the_x_ramp():
    vol, lut, made = ramp_case(2, 100)
    L = made[0].shape[:-1]
    flat = render_lines_np.render(vol, made[0], made.cols, made[1], lut)
    hit = flat["counted"] > 0
    assert hit.any() and (~hit).any() and (flat["rgb"][hit] == (200, 255, 7)).all()      # opaque: the first counted sample is the pixel

    def lit(vec, ambient):
        return render_lines_np.render(vol, made[0], made.cols, made[1], lut, light=np.broadcast_to(np.array(vec), L + (3,)), ambient=ambient)

    along = lit((4096, 0, 0), 64)      # the light along the gradient: fully lit
    same(along, flat)
    assert (along["gated"] == 0).all() and (along["lit"][hit] == ONE).all()      # dx = 200 inside, 100 at the edges: above the gate
    across = lit((0, 4096, 0), 64)      # the light across it: the ambient share
    assert np.array_equal(across["rgb"], ((flat["rgb"].astype(np.int64) * 64 + 128) >> 8).astype(np.uint8))
    assert (across["rgb"][hit] == (50, 64, 2)).all()
    assert (lit((2896, 2896, 0), 64)["rgb"][hit][:, 0] == 156).all()      # 45 degrees: diff = 181
    assert np.array_equal(lit((-4096, 0, 0), 64)["rgb"], along["rgb"])      # two-sided
    for other in (across, lit((2896, 2896, 0), 64)):
        assert np.array_equal(other["opacity"], flat["opacity"]) and np.array_equal(other["depth"], flat["depth"])


def test_oracle_the_z_ramp_and_the_gate_under_anisotropy():
    vol, lut, made = ramp_case(0, 300)
    n, h, w = vol.shape
    zi, yi, xi = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
    light = np.array([0, 0, 4096])
    sh, shaded = render_lines_np.shade(*render_lines_np.gradient(vol, xi, yi, zi, 256), light, 0, 200 * 200)
    assert shaded.all() and (sh == 256).all()      # dz = 600 inside, 300 at the ends: every voxel lit, and fully
    sh, shaded = render_lines_np.shade(*render_lines_np.gradient(vol, xi, yi, zi, 102), light, 0, 200 * 200)
    assert not shaded[0].any() and not shaded[-1].any() and shaded[1:-1].all()      # aspect 2.5: gz = 120 at the ends, 239 inside
    assert (sh == 256).all()
    L = made[0].shape[:-1]
    for zscale, gated in ((256, False), (102, True)):
        got = render_lines_np.render(vol, made[0], made.cols, made[1], lut, light=np.broadcast_to(light, L + (3,)), zscale=zscale,
                                     ambient=0, gmin2=200 * 200)
        assert (got["lit"] > 0).any() and (got["gated"] > 0).any() == gated
    # the light across the gradient, no ambient: black where lit, the colour where gated
    got = render_lines_np.render(vol, made[0], made.cols, made[1], lut, light=np.broadcast_to(np.array([4096, 0, 0]), L + (3,)),
                                 zscale=102, ambient=0, gmin2=200 * 200)
    assert (got["rgb"][got["lit"] == ONE] == 0).all() and (got["rgb"][got["gated"] == ONE] == (200, 255, 7)).all()


@pytest.mark.parametrize("aspect", [1.0, 2.5])
def test_oracle_the_hu_like_volume(aspect):
    vol, made, light, kw, flat = hu_case(aspect)
    zscale = int(np.floor(256.0 / aspect + 0.5))
    got = render_lines_np.render(vol, made[0], made.cols, made[1], TABLES["mixed"], light=light, zscale=zscale, ambient=64,
                                 gmin2=3000 * 3000, **kw)
    assert (got["lit"] > 0).any() and (got["gated"] > 0).any()      # both lit and gated samples carry weight
    assert (got["taken"] < got["counted"]).any()                    # some rays end early
    assert not np.array_equal(got["rgb"], flat["rgb"])
    assert np.array_equal(got["opacity"], flat["opacity"]) and np.array_equal(got["depth"], flat["depth"])
    assert np.array_equal(got["tr"], flat["tr"]) and np.array_equal(got["taken"], flat["taken"])


def test_oracle_isqrt_is_the_exact_floor():
    m = np.concatenate([np.arange(0, 5000), np.arange(1, 8193) ** 2, np.arange(1, 8193) ** 2 - 1, [3 * 4095 * 4095, (1 << 26) - 1]])
    n = render_lines_np.isqrt(m)
    assert ((n * n <= m) & ((n + 1) ** 2 > m)).all()


# ---------------------------------------------------------------------------------------------- 2. the geometry helpers
def test_headlight_is_the_unit_ray_whatever_the_oversample():
    from cta_gan_amd.infer import headlight, oblique_lines, orbit_lines, view_lines
    for aspect in (0.25, 1.0, 2.5):
        one = orbit_lines(5, 13, 11, [0, 30, 90, 200], axis=(1, 1, 0), aspect=aspect)
        two = orbit_lines(5, 13, 11, [0, 30, 90, 200], axis=(1, 1, 0), aspect=aspect, oversample=2)
        a, b = headlight(one, aspect), headlight(two, aspect)
        assert a.dtype == np.int64 and a.shape == one[0].shape[:-1] + (3,)
        assert np.abs(np.sqrt((a.astype(np.float64) ** 2).sum(axis=-1)) - 4096.0).max() < 1.0      # unit length within the rounding
        assert np.abs(a).max() <= 4096 and np.abs(a - b).max() <= 1      # (the tables' own coefficients are rounded apart)
        assert np.array_equal(headlight(one[0], aspect), a)      # a bare table
    z = orbit_lines(3, 5, 7, [0.0, 90.0], axis="z")
    assert np.array_equal(headlight(z)[0], np.broadcast_to([0, 4096, 0], (3, 3)))
    assert np.array_equal(np.abs(headlight(z)[1]), np.broadcast_to([4096, 0, 0], (3, 3)))
    with pytest.raises(ValueError, match="no ray"):
        headlight(oblique_lines(3, 5, 7, (0, 0, 1), count=3))      # T = 1
    still = view_lines(3, 5, 7, (1, 0, 0), (0, 0, 1), (0, 1, 0), 3, 5, depth=4)
    table = still[0].copy()
    table[1, 2::3] = 0
    with pytest.raises(ValueError, match="no ray direction"):
        headlight((table, 4))
    with pytest.raises(ValueError):
        headlight(still, aspect=0.0)
    with pytest.raises(ValueError):
        headlight(np.zeros((3, 6), dtype=np.int64))


def test_line_voxel_maps_a_depth_back_to_its_voxel():
    from cta_gan_amd.infer import line_voxel, orbit_lines
    vol = hu_like()
    made = orbit_lines(*vol.shape, [30.0], axis="x")
    lut = np.empty((256, 4), dtype=np.uint16)
    lut[:, :3], lut[:, 3] = np.arange(256)[:, None], ONE      # opaque grey: the pixel is the class of the first counted sample
    got = render_lines_np.render(vol, made[0], made.cols, made[1], lut, "nearest", surface=ONE, wc=1000.0, ww=4300.0, hu=True)
    rows, cols = np.nonzero(got["depth"][0] >= 0)
    assert len(rows) > 20
    for r, i in zip(rows[::7], cols[::7]):
        z, y, x = line_voxel(made[0][0, r], int(i), int(got["depth"][0, r, i]))
        assert got["rgb"][0, r, i, 0] == reformat_np.level(vol[z, y, x], 1000.0, 4300.0, True)
    z, y, x = line_voxel(made[0][0, 3], np.arange(made.cols), np.zeros(made.cols, dtype=np.int64))
    assert z.shape == (made.cols,) and z.dtype == np.int64
    with pytest.raises(ValueError):
        line_voxel([1, 2, 3], 0, 0)


# ---------------------------------------------------------------------------------------------- 3. refusals before a device is touched
def test_light_table_refusals_need_no_device():
    from cta_gan_amd import ops
    ok = ops.light_table_host(np.full((2, 3, 3), 4096, dtype=np.int64), 6)
    assert ok.dtype == np.int32 and ok.shape == (6, 3)
    for bad, count in ((np.zeros((6, 2), dtype=np.int64), 6), (np.zeros((6, 3)), 6), (np.zeros((5, 3), dtype=np.int64), 6),
                       (np.full((6, 3), 4097, dtype=np.int64), 6), (np.full((6, 3), -4097, dtype=np.int64), 6),
                       (np.full((1, 3), 2 ** 63, dtype=np.uint64), 1)):
        with pytest.raises(RuntimeError, match="render_lines"):
            ops.light_table_host(bad, count)
    with pytest.raises(RuntimeError, match="GPU device"):
        ops.LightTable(ok, 6, device="cpu")
    vol = np.zeros((2, 3, 4), dtype=np.int16)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        import torch
        ops.render_lines(torch.from_numpy(vol), np.zeros((1, 9), dtype=np.int64), 1, 1, TABLES["mixed"])


def test_volume_renderer_checks_its_arguments_on_the_host():
    from cta_gan_amd.infer import VolumeRenderer, headlight, oblique_lines, orbit_lines
    tables = {"tumble": lambda n, h, w: orbit_lines(n, h, w, [0.0, 40.0], axis="x", aspect=2.5)}
    view = VolumeRenderer(5, 13, 11, tables, shading={}, aspect=2.5)      # device=None: nothing touches a device before the first chunk
    assert view.volume is None and view.tables is None and view.device is None
    assert (view.zscale, view.ambient, view.gmin2) == (102, 77, 1600)
    made = tables["tumble"](5, 13, 11)
    lines = made[0].size // 9
    assert view.nbytes == 2 * 5 * 13 * 11 + 2048 + lines * (9 * 4 + 12 + 6 * made.cols)      # known before the first chunk
    assert np.array_equal(view.lights["tumble"].reshape(made[0].shape[:-1] + (3,)), headlight(made, 2.5))
    flat = VolumeRenderer(5, 13, 11, tables, depth=False)
    assert flat.lights is None and flat.nbytes == 2 * 5 * 13 * 11 + 2048 + lines * (9 * 4 + 4 * made.cols)
    fixed = VolumeRenderer(5, 13, 11, tables, shading={"light": (0, 3, 4), "ambient": 1.0, "gmin": 0})
    assert (fixed.lights["tumble"] == (0, 2458, 3277)).all() and (fixed.ambient, fixed.gmin2) == (256, 1)
    for bad in ({"sampling": "bilinear"}, {"shading": {"speculars": 1}}, {"shading": {"ambient": 1.5}}, {"shading": {"gmin": 9000}},
                {"shading": {"light": (0, 0, 0)}}, {"shading": "head"}, {"aspect": 0.0}, {"aspect": 1000.0}, {"aspect": 0.01},
                {"background": (0, 0, 256)}, {"stop": 32768}, {"surface": 0}, {"transfer": "arteries"}):
        with pytest.raises(ValueError):
            VolumeRenderer(5, 13, 11, tables, **bad)
    with pytest.raises(ValueError, match="no ray"):      # a plain plane has no ray for a headlight
        VolumeRenderer(5, 13, 11, {"p": lambda n, h, w: oblique_lines(n, h, w, (0, 0, 1))}, shading={})
    with pytest.raises(ValueError):
        VolumeRenderer(5000, 13, 11, tables)
    with pytest.raises(ValueError):
        VolumeRenderer(5, 13, 11, {})
    with pytest.raises(RuntimeError, match="GPU device"):
        VolumeRenderer(5, 13, 11, tables, device="cpu")


def test_volume_reformatter_is_refused_and_accepted_as_before():
    """The resident-volume bookkeeping moved to a base both views share: the same inputs are refused with the same words."""
    from cta_gan_amd.infer import VolumeReformatter, VolumeRenderer, orbit_lines
    tables = {"tumble": lambda n, h, w: orbit_lines(n, h, w, [0.0], axis="x")}
    ref = VolumeReformatter(5, 13, 11, tables, mode="mean")
    made = tables["tumble"](5, 13, 11)
    assert ref.volume is None and ref.tables is None and ref.device is None and (ref.source.seen == 0).all()
    assert ref.nbytes == 2 * 5 * 13 * 11 + (made[0].size // 9) * (36 + 3 * made.cols)
    with pytest.raises(ValueError, match="VolumeReformatter: n, h, w in 1 .. 4096 expected, got 5000 13 11"):
        VolumeReformatter(5000, 13, 11, tables)
    with pytest.raises(ValueError, match="VolumeReformatter: tables: a dict"):
        VolumeReformatter(5, 13, 11, [])
    with pytest.raises(ValueError, match="VolumeReformatter: table 'a': a LineSet, or a pair"):
        VolumeReformatter(5, 13, 11, {"a": (made[0], 2)})
    with pytest.raises(ValueError, match="mode"):
        VolumeReformatter(5, 13, 11, tables, mode="median")
    with pytest.raises(RuntimeError, match="VolumeReformatter: a GPU device is required"):
        VolumeReformatter(5, 13, 11, tables, device="cpu")
    for view in (ref, VolumeRenderer(5, 13, 11, tables)):
        with pytest.raises(RuntimeError, match="%s: every slice must have arrived exactly once: 5 of 5 missing, 0 more than once"
                           % type(view).__name__):
            view.result()
        view.source.seen[:] = 1
        view.source.seen[2] = 2
        with pytest.raises(RuntimeError, match="0 of 5 missing, 1 more than once"):
            view.result()
        view.reset()
        assert (view.source.seen == 0).all()


def test_series_translator_checks_render3d_in_its_constructor():
    from cta_gan_amd.infer import RENDER3D_OPTIONS, SeriesTranslator
    assert set(RENDER3D_OPTIONS) >= {"transfer", "wc", "ww", "hu", "sampling", "shading", "aspect", "background", "stop", "surface", "depth"}
    with pytest.raises(ValueError, match="render3d_options need render3d"):
        SeriesTranslator(None, render3d_options={"sampling": "nearest"})
    with pytest.raises(ValueError, match="at least one table"):
        SeriesTranslator(None, render3d={})
    with pytest.raises(ValueError, match="render3d_options"):
        SeriesTranslator(None, render3d={"a": None}, render3d_options={"oversample": 2})


# ---------------------------------------------------------------------------------------------- 4. the entry point and the flags
def test_the_symbol_and_its_signature():
    from cta_gan_amd import _lib
    assert _lib.SIGNATURES["ctg_render_lines"] == "piiipiiipiiiiiiffipiiipppp"
    assert _lib.ABI_VERSION == 15
    assert hasattr(_lib.load(), "ctg_render_lines")
    csrc = os.path.join(ROOT, "cta_gan_amd", "csrc")
    assert 'extern "C" int ctg_render_lines' in open(os.path.join(csrc, "render_lines.hip")).read()
    # one definition of the trilinear value: the struct lives in the shared header, and both kernels include it
    assert "struct RfmSample" in open(os.path.join(csrc, "reformat_sample.h")).read()
    for f in ("reformat.hip", "render_lines.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "reformat_sample.h"' in text and "struct RfmSample" not in text


def test_predict_has_the_vr3d_flags():
    sys.path.insert(0, ROOT)
    try:
        import predict
    finally:
        sys.path.remove(ROOT)
    base = ["--config", "c", "--weights", "w", "--input", "i", "--output", "o"]
    opts = predict.parse_args(base)
    assert opts.vr3d_dir is None and opts.vr3d_axis == "x" and opts.vr3d_sampling == "trilinear" and not opts.vr3d_shade
    assert (opts.vr3d_ambient, opts.vr3d_gmin) == (0.3, 40.0)
    opts = predict.parse_args(base + ["--vr3d-dir", "d", "--vr3d-axis", "1,1,0", "--vr3d-sampling", "nearest", "--vr3d-shade",
                                      "--vr3d-ambient", "0.5", "--vr3d-gmin", "10"])
    assert opts.vr3d_dir == "d" and opts.vr3d_axis == (1.0, 1.0, 0.0) and opts.vr3d_sampling == "nearest" and opts.vr3d_shade
    assert (opts.vr3d_ambient, opts.vr3d_gmin) == (0.5, 10.0)
    for bad in (["--vr3d-axis", "w"], ["--vr3d-axis", "0,0,0"], ["--vr3d-axis", "1,2"], ["--vr3d-sampling", "bilinear"],
                ["--vr3d-ambient", "2"], ["--vr3d-gmin", "-1"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
