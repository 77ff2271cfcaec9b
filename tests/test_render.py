"""CPU: the volume-rendered views without a GPU -- properties of the numpy restatement tests/render_np.py that the GPU tests lean
on, cta_gan_amd/infer.py: transfer_function / TRANSFER_PRESETS, and the host argument checks (ops.TransferTable, preset names,
predict.py's --vr flags).  Also home of the transfer tables the GPU file renders with (TABLES)."""
import os
import sys

import numpy as np
import pytest

import render_np
import rotate_lerp_np
import rotate_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WC, WW = 300.0, 40000.0      # the transfer window of the tests: random int16 values spread over all the classes
ONE = 32768


def make_tables(seed=5):
    """mixed: random colours, classes < 40 transparent, classes >= 200 opaque, the rest alpha < 4000; fog: no opaque class, alpha
    < 9000; opaque: every class opaque; wild: every field 65535 (the kernel reads 255, 255, 255 and opaque)."""
    rng = np.random.RandomState(seed)
    mixed = np.empty((256, 4), dtype=np.uint16)
    mixed[:, :3] = rng.randint(0, 256, size=(256, 3))
    mixed[:, 3] = rng.randint(0, 4000, size=256)
    mixed[:40, 3], mixed[200:, 3] = 0, ONE
    fog = np.empty((256, 4), dtype=np.uint16)
    fog[:, :3] = rng.randint(0, 256, size=(256, 3))
    fog[:, 3] = rng.randint(0, 9000, size=256)
    opaque = np.empty((256, 4), dtype=np.uint16)
    opaque[:, :3] = rng.randint(0, 256, size=(256, 3))
    opaque[:, 3] = ONE
    return {"mixed": mixed, "fog": fog, "opaque": opaque, "wild": np.full((256, 4), 65535, dtype=np.uint16)}


TABLES = make_tables()


def small_volume(n=3, h=19, w=23, seed=2):
    return np.random.RandomState(seed).randint(-32768, 32768, size=(n, h, w)).astype(np.int16)


def table(h, w, u, t, s=1, angles=(0, 90, 45, 10, 137.5)):
    return np.array([rotate_lerp_np.coefficients(a, h, w, u, t, s) for a in angles], dtype=np.int64)


# ---------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("sampling", ["nearest", "bilinear"])
def test_oracle_weights_telescope_and_the_stop_ends_rays(sampling):
    vol = small_volume()
    n, h, w = vol.shape
    d = rotate_np.detector(h, w)
    cls, ok = render_np.classes(vol, table(h, w, d, d), d, d, sampling, WC, WW)
    assert len(np.unique(cls)) > 200      # the window spreads the samples over the classes
    for name in ("mixed", "fog"):
        for stop in (0, 128):
            out = render_np.composite(cls, ok, TABLES[name], stop=stop, surface=16384, bg=(10, 200, 30))
            assert np.array_equal(out["weight"], ONE - out["tr"])
            assert (out["taken"] <= out["counted"]).all()
            early = out["taken"] < out["counted"]
            assert (out["tr"][early] <= stop).all()      # only the threshold ends a ray
            missed = out["counted"] == 0
            assert missed.any() and (out["rgb"][missed] == (10, 200, 30)).all() and (out["opacity"][missed] == 0).all() \
                and (out["depth"][missed] == -1).all()
            if name == "fog" and stop == 0:
                assert not early.any()      # wgt < Tr whenever alpha < 32768: Tr never reaches 0
            if name == "mixed":
                assert early.any() and (~early & ~missed).any() and (out["depth"] == -1).any() and (out["depth"] >= 0).any()


def test_oracle_a_transparent_table_shows_the_background():
    vol = small_volume()
    n, h, w = vol.shape
    d = rotate_np.detector(h, w)
    lut = TABLES["mixed"].copy()
    lut[:, 3] = 0
    out = render_np.render(vol, table(h, w, d, d), d, d, lut, stop=0, surface=1, bg=(1, 2, 255), wc=WC, ww=WW)
    assert (out["rgb"] == (1, 2, 255)).all() and (out["opacity"] == 0).all() and (out["depth"] == -1).all()
    assert np.array_equal(out["taken"], out["counted"])      # nothing ends such a ray


@pytest.mark.parametrize("sampling", ["nearest", "bilinear"])
def test_oracle_an_opaque_grey_table_shows_the_first_counted_sample(sampling):
    vol = small_volume()
    n, h, w = vol.shape
    d = rotate_np.detector(h, w)
    coef = table(h, w, d, d)
    grey = np.empty((256, 4), dtype=np.uint16)
    grey[:, :3] = np.arange(256)[:, None]
    grey[:, 3] = ONE
    cls, ok = render_np.classes(vol, coef, d, d, sampling, WC, WW)
    out = render_np.composite(cls, ok, grey, stop=0, surface=ONE, bg=(0, 0, 0))
    seen = rotate_np.count(h, w, coef, d, d) > 0      # [A][U]
    first = np.where(seen, ok.argmax(axis=2), -1)
    assert np.array_equal(out["depth"], np.broadcast_to(first[:, None, :], out["depth"].shape))
    assert np.array_equal(out["opacity"], np.broadcast_to(np.where(seen, 255, 0)[:, None, :], out["opacity"].shape))
    want = np.take_along_axis(cls, np.broadcast_to(np.maximum(first, 0)[:, None, :, None], cls.shape[:3] + (1,)), axis=3)[..., 0]
    want = np.where(seen[:, None, :], want, 0)
    assert all(np.array_equal(out["rgb"][..., c], want) for c in range(3))
    assert np.array_equal(out["taken"], np.broadcast_to(seen[:, None, :], out["taken"].shape))      # one sample, then the ray ends


def test_oracle_reads_a_wild_table_clamped():
    col, alpha = render_np.clamped(TABLES["wild"])
    assert (col == 255).all() and (alpha == ONE).all()
    with pytest.raises(AssertionError):
        render_np.clamped(np.zeros((255, 4), dtype=np.uint16))


# ---------------------------------------------------------------------------------------------- 2. transfer_function
def test_transfer_function_reproduces_its_points_and_rounds_half_up():
    from cta_gan_amd.infer import TRANSFER_PRESETS, transfer_function
    points = [(0, 0, 10, 255, 0.0), (10, 5, 10, 0, 0.25), (11, 200, 100, 0, 1.0), (255, 255, 0, 17, 0.5)]
    lut = transfer_function(points)
    assert lut.dtype == np.uint16 and lut.shape == (256, 4)
    for lv, r, g, b, a in points:
        assert lut[lv].tolist() == [r, g, b, int(np.floor(a * 32768 + 0.5))]
    assert np.array_equal(lut, transfer_function(points, 1))
    # colours: level 5 lies halfway between the first two points: R = 2.5 -> 3 (floor(x + 0.5), not round-half-even), B = 127.5 -> 128
    assert lut[5, 0] == 3 and lut[5, 1] == 10 and lut[5, 2] == 128 and lut[5, 3] == 4096
    lut = transfer_function([(0, 0, 0, 0, 0.0), (4, 2, 0, 0, 0.0)])      # R = 0.5, 1.0, 1.5 at the levels 1 .. 3
    assert lut[:5, 0].tolist() == [0, 1, 1, 2, 2] and (lut[4:, 0] == 2).all()      # the last point extends to the end
    one = transfer_function([(7, 1, 2, 3, 0.5)])
    assert (one == (1, 2, 3, 16384)).all()
    for name in ("grey", "vessels", "bone"):
        lut = transfer_function(TRANSFER_PRESETS[name])
        assert lut[:, :3].max() <= 255 and lut[:, 3].max() <= ONE and lut[0, 3] == 0
    grey = transfer_function(TRANSFER_PRESETS["grey"])
    assert all(np.array_equal(grey[:, c], np.arange(256)) for c in range(3)) and (np.diff(grey[:, 3].astype(int)) > 0).all()
    assert sorted(TRANSFER_PRESETS) == ["bone", "grey", "vessels"]


def test_transfer_function_refuses_bad_points():
    from cta_gan_amd.infer import transfer_function
    good = [(0, 0, 0, 0, 0.0), (255, 255, 255, 255, 1.0)]
    for bad in ([], [(0, 0, 0, 0)], [(0, 0, 0, 0, 0.0), (0, 1, 1, 1, 1.0)], [(5, 0, 0, 0, 0.0), (4, 1, 1, 1, 1.0)],
                [(-1, 0, 0, 0, 0.0)], [(256, 0, 0, 0, 0.0)], [(1.5, 0, 0, 0, 0.0)], [(0, 256, 0, 0, 0.0)], [(0, 0, -1, 0, 0.0)],
                [(0, 0, 0, 0, 1.5)], [(0, 0, 0, 0, -0.1)], [(0, 0, 0, 0, float("nan"))], "grey", 7):
        with pytest.raises(ValueError):
            transfer_function(bad)
    for s in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            transfer_function(good, s)


@pytest.mark.parametrize("s", [2, 3, 4, 8])
def test_oversampled_opacity_composites_to_the_unit_step(s):
    """s steps of the corrected alpha leave the transparency one uncorrected step leaves, within 2 s units of 1 / 32768: each of the
    s floors loses less than 1 and each alpha's rounding moves a step by at most 0.5 (the worst case met is printed)."""
    from cta_gan_amd.infer import transfer_function
    worst = 0
    for a0, a1 in ((0.0, 1.0), (0.0, 0.01), (0.99, 1.0), (0.3, 0.7)):      # 256 opacities each: a fine grid, and both ends finer
        points = [(0, 0, 0, 0, a0), (255, 0, 0, 0, a1)]
        unit = transfer_function(points)[:, 3].astype(np.int64)
        step = transfer_function(points, s)[:, 3].astype(np.int64)
        assert (step <= unit).all() and step.max() <= ONE
        tr = np.full(256, ONE, dtype=np.int64)
        for _ in range(s):
            tr -= (tr * step) >> 15
        worst = max(worst, int(np.abs(tr - (ONE - unit)).max()))
    print("oversample %d: worst difference %d of 32768 (bound %d)" % (s, worst, 2 * s))
    assert worst <= 2 * s


# ---------------------------------------------------------------------------------------------- 3. host argument checks
def test_transfer_table_refuses_bad_tables_before_it_touches_a_device():
    import torch
    from cta_gan_amd import ops
    for bad in (np.zeros((255, 4), dtype=np.uint16), np.zeros((256, 3), dtype=np.uint16), np.zeros((4, 256), dtype=np.uint16),
                np.zeros((256, 4), dtype=np.float32), np.full((256, 4), -1, dtype=np.int32), np.full((256, 4), 65536, dtype=np.int64),
                torch.zeros((256, 4), dtype=torch.float32), np.zeros(1024, dtype=np.uint16)):
        with pytest.raises(RuntimeError, match="project_render"):
            ops.TransferTable(bad)
    with pytest.raises(RuntimeError, match="GPU device"):
        ops.TransferTable(np.zeros((256, 4), dtype=np.uint16), device="cpu")


def test_renderer_refuses_bad_arguments_before_it_touches_a_device():
    from cta_gan_amd.infer import SeriesRenderer
    for kw in (dict(transfer="veins"), dict(transfer=[(0, 0, 0, 0)]), dict(sampling="cubic"), dict(oversample=0), dict(background=(0, 0)),
               dict(background=(0, 0, 256)), dict(stop=-1), dict(stop=32768), dict(surface=0), dict(surface=32769), dict(stop=1.5)):
        with pytest.raises(ValueError):
            SeriesRenderer(2, 8, 8, [0.0], **kw)
    with pytest.raises(ValueError):
        SeriesRenderer(2, 8, 8, [])
    with pytest.raises(RuntimeError, match="GPU device"):
        SeriesRenderer(2, 8, 8, [0.0], device="cpu")


def test_translator_refuses_bad_render_arguments():
    import torch
    from cta_gan_amd.infer import SeriesTranslator
    g = torch.nn.Identity()
    for kw in (dict(render=[]), dict(render_options={"wc": 1.0}), dict(render=3, render_options={"mode": "max"}),
               dict(render=3, render_options={"device": "cuda"})):
        with pytest.raises(ValueError):
            SeriesTranslator(g, device="cpu", **kw)


def test_predict_parser_has_the_render_flags():
    sys.path.insert(0, ROOT)
    try:
        import predict
    finally:
        sys.path.remove(ROOT)
    base = ["--weights", "g.pth", "--input", "in.npy", "--output", "out.npy"]
    opts = predict.parse_args(base)
    assert opts.vr_dir is None and opts.vr_angles == 36 and opts.vr_span == 360.0 and opts.vr_preset == "vessels"
    assert (opts.vr_wc, opts.vr_ww, opts.vr_sampling, opts.vr_oversample, opts.vr_background) == (300.0, 1500.0, "nearest", 1, (0, 0, 0))
    opts = predict.parse_args(base + ["--vr-dir", "vr", "--vr-angles", "4", "--vr-span", "180", "--vr-preset", "bone", "--vr-wc", "400",
                                      "--vr-ww", "2000", "--vr-sampling", "bilinear", "--vr-oversample", "2", "--vr-background",
                                      "10,20,255"])
    assert (opts.vr_dir, opts.vr_angles, opts.vr_span, opts.vr_preset) == ("vr", 4, 180.0, "bone")
    assert (opts.vr_wc, opts.vr_ww, opts.vr_sampling, opts.vr_oversample, opts.vr_background) == (400.0, 2000.0, "bilinear", 2, (10, 20, 255))
    from cta_gan_amd.infer import TRANSFER_PRESETS
    assert sorted(predict.VR_PRESETS) == sorted(TRANSFER_PRESETS)
    for bad in (["--vr-preset", "veins"], ["--vr-background", "1,2"], ["--vr-background", "1,2,256"], ["--vr-background", "a,b,c"],
                ["--vr-sampling", "cubic"], ["--vr-angles", "0"], ["--vr-oversample", "0"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
