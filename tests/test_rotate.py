"""CPU: the rotating projections (csrc/project_rotate.hip, cta_gan_amd/infer.py, predict.py --rot-dir) -- the entry point is
declared, bound and exported; the numpy restatement the GPU tests compare against agrees with the coefficient rows, the
cardinal-angle identities and a slice worked out by hand; the host side's angle and detector arithmetic; predict.py's options."""
import ctypes
import os
import sys

import numpy as np
import pytest

import project_np
import rotate_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, SIG = "ctg_project_rotate", "piiiiipiiiiiffippp"
MODES = ["max", "min", "mean"]


def test_header_and_binding_carry_the_entry():
    from cta_gan_amd import _lib
    from test_abi import parse_header
    assert parse_header().get(NAME) == SIG
    assert _lib.SIGNATURES.get(NAME) == SIG
    text = open(os.path.join(ROOT, "include", "ctagan_hip.h")).read()
    comment = text.split("int " + NAME)[0][-3500:]
    assert "infer.py" in comment and "additive" in comment
    src = open(os.path.join(ROOT, "cta_gan_amd", "csrc", "project_rotate.hip")).read()
    assert 'extern "C" int ' + NAME in src


def test_built_library_exports_the_entry():
    from cta_gan_amd import build
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, NAME)


COEFFICIENTS = [      # (angle, U, T) of a 5 x 7 slice
    (0, 7, 5, [32768, 65536, 0, 32768, 0, 65536]),
    (90, 5, 7, [425984, 0, -65536, 32768, 65536, 0]),
    (180, 7, 5, [425984, -65536, 0, 294912, 0, -65536]),
    (270, 5, 7, [32768, 0, 65536, 294912, -65536, 0]),
    (45, 9, 9, [229376, 46341, -46341, -206888, 46341, 46341]),
]


@pytest.mark.parametrize("angle,u,t,want", COEFFICIENTS, ids=[str(c[0]) for c in COEFFICIENTS])
def test_coefficient_rows(angle, u, t, want):
    from cta_gan_amd.infer import rotation_coefficients
    got = rotation_coefficients(angle, 5, 7, u, t)
    assert isinstance(got, tuple) and len(got) == 6 and all(type(v) is int for v in got)
    assert list(got) == want
    assert rotate_np.coefficients(angle, 5, 7, u, t) == want
    assert rotation_coefficients(float(angle) + 360.0, 5, 7, u, t)[1::3] == (want[1], want[4])      # cos, sin of a full turn more
    if (u, t) == (9, 9):      # the default detector of 5 x 7
        assert list(rotation_coefficients(angle, 5, 7)) == want and rotate_np.coefficients(angle, 5, 7) == want


def test_coefficients_agree_at_other_angles_and_refuse_sizes():
    from cta_gan_amd.infer import rotation_coefficients
    for angle in (10, 137.5, -30, 359.9, 33.3):
        for h, w in ((1, 1), (33, 31), (512, 512), (19, 515)):
            c = rotation_coefficients(angle, h, w)
            assert list(c) == rotate_np.coefficients(angle, h, w)
            assert max(abs(c[1]), abs(c[2]), abs(c[4]), abs(c[5])) <= 65536 and max(abs(c[0]), abs(c[3])) < 2 ** 29
    with pytest.raises(ValueError):
        rotation_coefficients(0, 4097, 8)
    with pytest.raises(ValueError):
        rotation_coefficients(0, 8, 8, 0, 8)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 16, 24), (2, 33, 31)], ids=lambda s: "%dx%dx%d" % s)
def test_cardinal_angles_are_the_coronal_and_sagittal_projections(shape, mode):
    n, h, w = shape
    vol = np.random.RandomState(h * w).randint(-32768, 32768, size=shape).astype(np.int16)
    _, coronal, sagittal = project_np.project(vol, mode)
    coef = [rotate_np.coefficients(a, h, w, w, h) for a in (0, 180)]
    got = rotate_np.rotate(vol, coef, w, h, mode)
    assert got.shape == (2, n, w) and got.dtype == np.int16
    assert np.array_equal(got[0], coronal) and np.array_equal(got[1], coronal[:, ::-1])
    assert (rotate_np.count(h, w, coef, w, h) == h).all()
    coef = [rotate_np.coefficients(a, h, w, h, w) for a in (90, 270)]
    got = rotate_np.rotate(vol, coef, h, w, mode)
    assert got.shape == (2, n, h)
    assert np.array_equal(got[0], sagittal) and np.array_equal(got[1], sagittal[:, ::-1])
    assert (rotate_np.count(h, w, coef, h, w) == w).all()


def test_a_slice_at_45_degrees_written_out_by_hand():
    # centre (1, 1), sin = cos = s = 0.7071; with p = u - 3 and q = t - 2 the sample is x = 1 + (p - q) s, y = 1 + (p + q) s,
    # rounded to nearest: a difference (or sum) of 0 -> 1, 1 or 2 -> 2, -1 or -2 -> 0, beyond -> outside.
    #   p = -3: none     p = -2: (0,0)     p = -1: (0,1) (0,0) (1,0)     p = 0: (0,2) (0,2) (1,1) (2,0) (2,0)     [(y, x)]
    #   p = 1: (1,2) (2,2) (2,1)     p = 2: (2,2)     p = 3: none
    sl = np.array([[[1, -2, 3], [4, 5, -6], [-7, 8, 9]]], dtype=np.int16)
    coef = [rotate_np.coefficients(45, 3, 3, 7, 5)]
    assert rotate_np.count(3, 3, coef, 7, 5).tolist() == [[0, 1, 3, 5, 3, 1, 0]]
    fill = -77
    want = {"max": [fill, 1, 4, 5, 9, 9, fill], "min": [fill, 1, -2, -7, -6, 9, fill],
            # sums 1, 3, 3 + 3 + 5 - 7 - 7 = -3, 11, 9 over the rays' own counts: -3 / 5 truncates to 0 (floor: -1)
            "mean": [fill, 1, 1, 0, 3, 9, fill]}
    for mode in MODES:
        assert rotate_np.rotate(sl, coef, 7, 5, mode, fill).tolist() == [[want[mode]]], mode
    assert rotate_np.rotate(sl, coef, 7, 5, "max").tolist()[0][0][::6] == [0, 0]      # the default fill
    # the default detector of 3 x 3 is 5: the two empty rays are gone, the others are the same
    assert rotate_np.detector(3, 3) == 5
    assert rotate_np.rotate(sl, [rotate_np.coefficients(45, 3, 3)], 5, 5, "max", fill).tolist() == [[want["max"][1:6]]]


def test_mean_divides_by_the_rays_own_count_toward_zero():
    # a 3 x 1 slice under rays of 5 steps: 3 samples count; -8 / 3 = -2 (floor: -3; by the 5 steps: -1)
    vol = np.array([-3, -3, -2], dtype=np.int16).reshape(1, 3, 1)
    coef = [rotate_np.coefficients(0, 3, 1, 1, 5)]
    assert rotate_np.count(3, 1, coef, 1, 5).tolist() == [[3]]
    assert rotate_np.rotate(vol, coef, 1, 5, "mean").tolist() == [[[-2]]]
    assert rotate_np.rotate(-vol, coef, 1, 5, "mean").tolist() == [[[2]]]
    big = np.full((2, 4, 6), 32767, dtype=np.int16)
    coef = [rotate_np.coefficients(a, 4, 6) for a in (0, 45, 77)]
    d = rotate_np.detector(4, 6)
    got = rotate_np.rotate(big, coef, d, d, "mean", fill=-5)
    assert set(np.unique(got).tolist()) == {-5, 32767}
    assert np.array_equal(got[:, 0] == -5, rotate_np.count(4, 6, coef, d, d) == 0)


def test_empty_rays_of_a_512_slice_under_the_default_detector():
    assert rotate_np.detector(512, 512) == 725
    for angle, empty in ((0, 213), (90, 213), (10, 132), (45, 0), (137.5, 2)):
        cnt = rotate_np.count(512, 512, [rotate_np.coefficients(angle, 512, 512)], 725, 725)
        assert int((cnt == 0).sum()) == empty, angle


def test_level_of_rotated_values_is_the_projection_level():
    v = np.array([[0, 1, 877, 1275, -1024, 32767]], dtype=np.int16)
    assert np.array_equal(rotate_np.level(v, 50.0, 400.0), project_np.level(v, 50.0, 400.0))
    assert rotate_np.level(v, 50.0, 400.0).tolist() == [[0, 0, 1, 255, 0, 255]]


def test_view_angles_and_default_detector():
    from cta_gan_amd.infer import default_detector, view_angles
    assert view_angles(4) == [0.0, 90.0, 180.0, 270.0]
    assert view_angles(36)[1] == 10.0 and len(view_angles(36)) == 36 and view_angles(36)[-1] == 350.0
    assert view_angles(3, span=180.0, start=-30.0) == [-30.0, 30.0, 90.0]
    assert view_angles(1) == [0.0]
    with pytest.raises(ValueError):
        view_angles(0)
    assert default_detector(512, 512) == 725 and default_detector(5, 7) == 9 and default_detector(3, 4) == 5
    assert default_detector(1, 1) == 2 and default_detector(19, 515) == 516
    for h, w in ((1, 1), (5, 7), (33, 31), (512, 512)):
        assert default_detector(h, w) == rotate_np.detector(h, w)


def test_predict_rotation_arguments():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import predict
    p = predict.build_parser()
    base = ["--weights", "g.pth", "--input", "in.npy", "--output", "out.npy"]
    o = p.parse_args(base)
    assert o.rot_dir is None and o.rot_angles == 36 and o.rot_span == 360.0      # nothing new happens
    # the defaults of the existing options do not move
    assert (o.mip_dir, o.mip_mode, o.slab, o.aspect, o.wc, o.ww, o.batch, o.hu, o.level_dir, o.dtype) == \
        (None, "max", None, 1.0, 50.0, 400.0, 16, False, None, None)
    o = p.parse_args(base + ["--rot-dir", "rot", "--rot-angles", "18", "--rot-span", "180", "--mip-mode", "min"])
    assert (o.rot_dir, o.rot_angles, o.rot_span, o.mip_mode, o.mip_dir) == ("rot", 18, 180.0, "min", None)
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--rot-angles", "many"])
