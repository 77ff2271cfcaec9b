"""CPU: bilinear sampling and oversampled rays of the rotating projections (csrc/project_rotate.hip:
ctg_project_rotate_bilinear; infer.rotation_coefficients(..., oversample); predict.py --rot-sampling / --rot-oversample) -- the
entry point is declared, bound and exported; the host's oversampled coefficient rows; the numpy restatement the GPU tests compare
against (tests/rotate_lerp_np.py) agrees with an interpolation worked out by hand, with nearest sampling where the fractions are
zero, keeps a constant slice constant at the ends of int16, and never loses a one-pixel maximum, which nearest sampling at unit
steps does."""
import ctypes
import os
import sys

import numpy as np
import pytest

import rotate_lerp_np
import rotate_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, SIG = "ctg_project_rotate_bilinear", "piiiiipiiiiiffippp"
MODES = ["max", "min", "mean"]


def test_header_and_binding_carry_the_entry():
    from cta_gan_amd import _lib, ops
    from test_abi import parse_header
    assert parse_header().get(NAME) == SIG and parse_header().get("ctg_project_rotate") == SIG
    assert _lib.SIGNATURES.get(NAME) == SIG
    assert ops.ROTATE_SAMPLINGS == {"nearest": "ctg_project_rotate", "bilinear": NAME}
    text = open(os.path.join(ROOT, "include", "ctagan_hip.h")).read()
    assert text.index("int ctg_project_rotate(") < text.index("int " + NAME + "(")      # declared after the nearest entry
    comment = text.split("int " + NAME + "(")[0][-3500:]
    assert "added under ABI 15: purely additive" in comment and "infer.py" in comment
    assert _lib.ABI_VERSION == 15 and "#define CTG_ABI_VERSION 15" in text
    src = open(os.path.join(ROOT, "cta_gan_amd", "csrc", "project_rotate.hip")).read()
    assert 'extern "C" int ' + NAME + "(" in src


def test_built_library_exports_the_entry():
    from cta_gan_amd import build
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, NAME)


# ---------------------------------------------------------------------------------------------- the coefficient rows
def test_unit_steps_are_the_rows_of_nearest_sampling():
    from cta_gan_amd.infer import rotation_coefficients
    for angle in (0, 90, 180, 270, 45, 10, 137.5, -30, 359.9, 33.3):
        for h, w, u, t in ((1, 1, None, None), (5, 7, 7, 5), (33, 31, None, None), (512, 512, None, None), (19, 515, 515, 19),
                           (37, 53, 30, 40)):
            want = rotate_np.coefficients(angle, h, w, u, t)
            assert list(rotation_coefficients(angle, h, w, u, t, oversample=1)) == want
            assert list(rotation_coefficients(angle, h, w, u, t)) == want
            assert rotate_lerp_np.coefficients(angle, h, w, u, t, 1) == want
            for s in (2, 3):
                c = rotation_coefficients(angle, h, w, u, t, oversample=s)
                assert list(c) == rotate_lerp_np.coefficients(angle, h, w, u, t, s)
                assert c[1] == want[1] and c[4] == want[4]      # the detector's step does not change
                assert max(abs(c[1]), abs(c[2]), abs(c[4]), abs(c[5])) <= 65536 and max(abs(c[0]), abs(c[3])) < 2 ** 29


OVERSAMPLED = [      # (angle, U, T in voxels) of a 5 x 7 slice at s = 2: ct = (2 T - 1) / 4
    # 0: c3 = (2 - 2.25 + 0.5) 65536, the half step 32768
    (0, 7, 5, [32768, 65536, 0, 16384, 0, 32768]),
    # 90: c0 = (3 + 3.25 + 0.5) 65536
    (90, 5, 7, [442368, 0, -32768, 32768, 65536, 0]),
    # 45, s = cos = sin = 0.70710678: c0 = (3.5 + 0.25 s) 65536 = 240961.3, c3 = (2.5 - 8.25 s) 65536 = -218472.8, s / 2 -> 23170.5
    (45, 9, 9, [240961, 46341, -23170, -218473, 46341, 23170]),
]


@pytest.mark.parametrize("angle,u,t,want", OVERSAMPLED, ids=[str(c[0]) for c in OVERSAMPLED])
def test_oversampled_coefficient_rows(angle, u, t, want):
    from cta_gan_amd.infer import rotation_coefficients
    got = rotation_coefficients(angle, 5, 7, u, t, oversample=2)
    assert isinstance(got, tuple) and len(got) == 6 and all(type(v) is int for v in got)
    assert list(got) == want and rotate_lerp_np.coefficients(angle, 5, 7, u, t, 2) == want


def test_the_step_limit_is_refused_by_name():
    from cta_gan_amd import ops
    from cta_gan_amd.infer import rotation_coefficients
    assert ops.ROTATE_MAX_DIM == 4096
    rotation_coefficients(0, 8, 8, 8, 2048, oversample=2)      # 4096 steps: the limit itself
    with pytest.raises(ValueError) as e:
        rotation_coefficients(0, 8, 8, 8, 2049, oversample=2)
    assert "2049" in str(e.value) and "4098" in str(e.value)
    with pytest.raises(ValueError):
        rotation_coefficients(0, 512, 512, oversample=6)      # 725 x 6 = 4350
    with pytest.raises(ValueError):
        rotation_coefficients(0, 8, 8, oversample=0)


# ---------------------------------------------------------------------------------------------- the interpolation, by hand
def test_a_two_by_two_slice_interpolated_by_hand():
    # one ray of four steps, X = 16384 + 36864 t, Y = 49152 + 12288 t; every sample counts (X >> 16 = 0 0 1 1, Y >> 16 = 0 0 1 1)
    #   t   Xc = X - 32768   x0   fx    Yc     y0   fy
    #   0      -16384        -1   192   16384   0    64     x0 = -1: both columns clamp onto column 0
    #   1       20480         0    80   28672   0   112
    #   2       57344         0   224   40960   0   160
    #   3       94208         1   112   53248   0   208     x0 + 1 = 2: both columns clamp onto column 1
    sl = np.array([[[-7, 1000], [10, -32768]]], dtype=np.int16)
    coef = [[16384, 0, 36864, 49152, 0, 12288]]
    assert rotate_np.count(2, 2, coef, 1, 4).tolist() == [[4]]
    # t = 0: top = 256 (-7), bot = 256 (10); (-7 192 + 10 64 + 128) >> 8 = -576 >> 8 = floor(-2.75 + 0.5) = -3: the shift floors
    # t = 1: top = -7 176 + 1000 80 = 78768, bot = 10 176 - 32768 80 = -2619680; (78768 144 - 2619680 112 + 32768) >> 16 = -4304
    # t = 2: top = -7 32 + 1000 224 = 223776, bot = 10 32 - 32768 224 = -7339712; (223776 96 - 7339712 160 + 32768) >> 16 = -17591
    # t = 3: top = 256000, bot = -8388608; 187.5 - 26624 = -26436.5, plus the half exactly -26436
    v, ok = rotate_lerp_np.samples(sl, coef[0], 1, 4)
    assert ok.all() and v.tolist() == [[[-3, -4304, -17591, -26436]]]
    got = rotate_lerp_np.rotate_modes(sl, coef, 1, 4)
    # the sum -48334 over 4 samples is -12083.5: toward zero -12083 (floor: -12084)
    assert {m: got[m].tolist() for m in MODES} == {"max": [[[-3]]], "min": [[[-26436]]], "mean": [[[-12083]]]}
    # the same ray two steps longer leaves the slice: the count stays 4 and so does every value; with no sample at all: fill
    assert rotate_np.count(2, 2, coef, 1, 6).tolist() == [[4]]
    assert rotate_lerp_np.rotate(sl, coef, 1, 6, "mean").tolist() == [[[-12083]]]
    away = [[16384 + (5 << 16), 0, 36864, 49152, 0, 12288]]
    assert rotate_lerp_np.rotate(sl, away, 1, 4, "max", fill=-77).tolist() == [[[-77]]]


# ---------------------------------------------------------------------------------------------- properties of the restatement
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 16, 24), (2, 33, 31)], ids=lambda s: "%dx%dx%d" % s)
def test_cardinal_angles_equal_nearest_sampling(shape):
    """At 0 / 180 degrees with the detector (W, H) and at 90 / 270 with (H, W) every sample sits on a pixel centre: the fractions
    are exactly 0 and bilinear is nearest."""
    n, h, w = shape
    vol = np.random.RandomState(h * w).randint(-32768, 32768, size=shape).astype(np.int16)
    for angles, u, t in (((0, 180), w, h), ((90, 270), h, w)):
        coef = [rotate_np.coefficients(a, h, w, u, t) for a in angles]
        got = rotate_lerp_np.rotate_modes(vol, coef, u, t, MODES)
        for mode in MODES:
            assert np.array_equal(got[mode], rotate_np.rotate(vol, coef, u, t, mode)), (angles, mode)


@pytest.mark.parametrize("s", [1, 2, 3])
def test_a_constant_slice_stays_constant_at_both_ends_of_int16(s):
    """The four weights sum to 65536 and the accumulator's extremes fit (rotate_lerp_np asserts the int32 range): a slice of
    -32768 or of 32767 comes back as itself on every ray that counts a sample."""
    h, w = 9, 11
    d = rotate_np.detector(h, w)
    vol = np.stack([np.full((h, w), -32768, dtype=np.int16), np.full((h, w), 32767, dtype=np.int16)])
    coef = [rotate_lerp_np.coefficients(a, h, w, oversample=s) for a in (0, 90, 45, 10, 137.5, -30, 359.9)]
    seen = rotate_np.count(h, w, coef, d, d * s) > 0
    assert seen.any(axis=1).all() and not seen.all()
    got = rotate_lerp_np.rotate_modes(vol, coef, d, d * s, MODES, fill=5)
    for mode in MODES:
        for i, const in enumerate((-32768, 32767)):
            assert np.array_equal(got[mode][:, i], np.where(seen, const, 5)), (mode, const)


def test_a_one_pixel_maximum_is_lost_by_nearest_and_kept_by_bilinear():
    """A 33 x 31 slice of 0 with one pixel at 1000, at every position in turn (slice i has pixel i), default detector.  Nearest
    sampling at unit steps steps over some positions at 45 degrees.  Bilinear cannot: the samples of all rays form a rotated
    unit lattice, which has a point within sqrt(2) / 2 of any pixel centre, so the pixel's weight in that sample is at least about
    (1 - 0.71)^2 and the maximum along that ray is > 0."""
    h, w = 33, 31
    d = rotate_np.detector(h, w)
    vol = np.zeros((h * w, h, w), dtype=np.int16)
    vol.reshape(h * w, h * w)[np.arange(h * w), np.arange(h * w)] = 1000
    lost = rotate_np.rotate(vol, [rotate_np.coefficients(45, h, w)], d, d, "max")[0].max(axis=1) == 0
    print("nearest, unit steps, 45 degrees: %d of %d positions lost" % (lost.sum(), h * w))
    assert lost.sum() > 0
    for angle in (45, 30, 10, 77):
        peak = rotate_lerp_np.rotate(vol, [rotate_lerp_np.coefficients(angle, h, w)], d, d, "max")[0].max(axis=1)
        print("bilinear, %g degrees: the smallest peak over the positions is %d of 1000" % (angle, peak.min()))
        assert (peak > 0).all(), angle


# ---------------------------------------------------------------------------------------------- the host's arguments
def test_bad_sampling_and_oversample_are_refused_at_construction():
    from cta_gan_amd.infer import SeriesRotator, SeriesTranslator
    for kw in (dict(sampling="cubic"), dict(sampling=None), dict(oversample=0), dict(oversample=1.5), dict(oversample=True)):
        with pytest.raises(ValueError):
            SeriesRotator(4, 8, 8, [0.0], **kw)
    for kw in (dict(rotate_sampling="linear"), dict(rotate_oversample=0), dict(rotate_oversample="2")):
        with pytest.raises(ValueError):
            SeriesTranslator(None, rotate=3, **kw)


def test_predict_sampling_arguments():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import predict
    p = predict.build_parser()
    base = ["--weights", "g.pth", "--input", "in.npy", "--output", "out.npy"]
    o = p.parse_args(base)
    assert (o.rot_sampling, o.rot_oversample, o.rot_dir, o.rot_angles, o.rot_span) == ("nearest", 1, None, 36, 360.0)
    o = p.parse_args(base + ["--rot-dir", "rot", "--rot-sampling", "bilinear", "--rot-oversample", "2"])
    assert (o.rot_dir, o.rot_sampling, o.rot_oversample) == ("rot", "bilinear", 2)
    for bad in (["--rot-sampling", "cubic"], ["--rot-oversample", "1.5"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)
    assert "--rot-sampling nearest|bilinear" in predict.__doc__ and "--rot-oversample S" in predict.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--rot-sampling nearest|bilinear" in readme and "--rot-oversample S" in readme
