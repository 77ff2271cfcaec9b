"""CPU: the subtraction volume (csrc/subtract.hip, cta_gan_amd/infer.py, predict.py --sub-output) -- the entry point is declared,
bound and exported; the numpy restatement the GPU tests compare against agrees with scipy's median filter and with cases worked
out by hand; the arguments of the translator and of predict.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

import project_np
import subtract_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, SIG = "ctg_subtract_slices", "ppiiiiiiiiffppp"
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 37, 53), (4, 19, 515), (2, 9, 1032), (2, 1, 9), (2, 9, 1)]


def test_header_and_binding_carry_the_entry():
    from cta_gan_amd import _lib
    from test_abi import parse_header
    assert parse_header().get(NAME) == SIG
    assert _lib.SIGNATURES.get(NAME) == SIG
    assert _lib.ABI_VERSION == 15
    text = open(os.path.join(ROOT, "include", "ctagan_hip.h")).read()
    assert "#define CTG_ABI_VERSION 15" in text
    comment = text.split("int " + NAME)[0][-3000:]
    assert "infer.py" in comment and "additive" in comment and "must not overlap" in comment
    src = open(os.path.join(ROOT, "cta_gan_amd", "csrc", "subtract.hip")).read()
    assert 'extern "C" int ' + NAME in src


def test_built_library_exports_the_entry():
    from cta_gan_amd import build
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, NAME)
    lib.ctg_abi_version.restype = ctypes.c_int
    assert lib.ctg_abi_version() == 15


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_restatement_median_equals_scipy(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(shape[1] * shape[2])
    for d in (rng.randint(-66559, 33792, size=shape), rng.randint(0, 4, size=shape)):      # the second: ties
        want = np.stack([ndimage.median_filter(p, size=3, mode="nearest") for p in d])
        assert np.array_equal(subtract_np.median3x3(d), want)


CORNERS = [      # (ct, cta, cta_is_hu, sub)
    (-32768, 32767, 0, 32767),
    (32767, -32768, 0, -32768),
    (-1024, 0, 0, 0),
    (-1024, 0, 1, 1024),
    (0, 4095, 0, 3071),
    (0, 4095, 1, 4095),
]


@pytest.mark.parametrize("ct,cta,hu,want", CORNERS)
def test_restatement_int16_corner_cases(ct, cta, hu, want):
    c, a = np.full((1, 3, 3), ct, dtype=np.int16), np.full((1, 3, 3), cta, dtype=np.int16)
    for median in (False, True):
        got = subtract_np.subtract(a, c, bool(hu), median, None)
        assert got.dtype == np.int16 and (got == want).all(), got


def test_restatement_on_a_plane_written_out_by_hand():
    # ct = -1024 everywhere: d = cta.  The centre's neighbourhood is all nine values (median 5); a corner's is its own value four
    # times, two neighbours twice each and the diagonal one once.
    cta = np.array([[[9, 1, 8], [2, 5, 7], [3, 6, 4]]], dtype=np.int16)
    ct = np.full((1, 3, 3), -1024, dtype=np.int16)
    assert subtract_np.subtract(cta, ct, False, False, None).tolist() == cta.tolist()
    # (0, 0): 9 9 9 9 1 1 2 2 5 -> 5;  (0, 2): 8 8 8 8 1 1 7 7 5 -> 7;  (0, 1): 9 9 1 1 8 8 2 5 7 -> 7
    got = subtract_np.subtract(cta, ct, False, True, None)
    assert got[0, 1, 1] == 5 and got[0, 0, 0] == 5 and got[0, 0, 2] == 7 and got[0, 0, 1] == 7
    # floor and band test the centre pixel after the median; equality keeps it
    assert subtract_np.subtract(cta, ct, False, True, 6)[0, 0].tolist() == [0, 7, 7]
    assert subtract_np.subtract(cta, ct, False, True, 5)[0, 0].tolist() == [5, 7, 7]
    band = ct.copy()
    band[0, 0] = [-900, -901, 400]
    d = subtract_np.subtract(cta, band, False, False, None, -900, 400)
    assert d[0, 0].tolist() == [9 - 124, 0, 8 - 1424] and d[0, 1].tolist() == [0, 0, 0]      # -1024 is below the band
    # H = 1 and W = 1 planes: the median of three values, the ends replicated
    row = np.array([[[5, 1, 9, 2]]], dtype=np.int16)
    assert subtract_np.subtract(row, ct[:, :1, :1].repeat(4, axis=2), False, True, None).tolist() == [[[5, 5, 2, 2]]]
    col = row.reshape(1, 4, 1)
    assert subtract_np.subtract(col, np.full((1, 4, 1), -1024, dtype=np.int16), False, True, None).reshape(-1).tolist() == [5, 5, 2, 2]


def test_restatement_level_is_the_projection_level_of_a_hu_value():
    v = np.array([-1024, -1, 0, 1, 2, 150, 299, 300, 301, 32767], dtype=np.int16)
    assert np.array_equal(subtract_np.level(v), project_np.level(v, 150.0, 300.0, True))
    # win_min = 0.5, dFactor = 0.85: level = trunc((v - 0.5) * 0.85) clamped -- 0 and 1 are level 0, 301 HU of enhancement is 255
    assert subtract_np.level(v).tolist() == [0, 0, 0, 0, 1, 127, 253, 254, 255, 255]
    assert np.unique(subtract_np.level(np.arange(-1024, 8192), 150.0, 300.0)).size == 256


def test_translator_refuses_a_sub_source_without_subtract():
    from cta_gan_amd.infer import SeriesTranslator
    with pytest.raises(ValueError):
        SeriesTranslator(None, project_source="sub")      # raised before the generator or a device is touched
    with pytest.raises(ValueError):
        SeriesTranslator(None, subtract=True, project_source="both")


def test_ops_and_infer_carry_the_new_names():
    import inspect
    from cta_gan_amd import infer, ops
    p = inspect.signature(ops.subtract_slices).parameters
    assert [k for k in p][:2] == ["cta", "ct_hu"] and all(p[k].kind is p[k].KEYWORD_ONLY for k in list(p)[2:])
    assert (p["cta_is_hu"].default, p["median"].default, p["floor"].default, p["ct_range"].default, p["wc"].default,
            p["ww"].default, p["want_sub"].default, p["want_level"].default) == (False, True, 0, (None, None), 150.0, 300.0, True, True)
    q = inspect.signature(infer.SeriesTranslator.__init__).parameters
    assert (q["subtract"].default, q["sub_median"].default, q["sub_floor"].default, q["sub_ct_range"].default,
            q["sub_window"].default, q["project_source"].default) == (False, True, 0, (None, None), (150.0, 300.0), "cta")
    assert callable(infer.subtract_volume)


def test_predict_subtraction_arguments():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import predict
    base = ["--weights", "g.pth", "--input", "in.npy", "--output", "out.npy"]
    o = predict.parse_args(base)
    assert (o.sub_output, o.sub_level_dir, o.sub_floor, o.sub_no_median, o.sub_ct_min, o.sub_ct_max, o.sub_wc, o.sub_ww,
            o.mip_source) == (None, None, 0, False, None, None, 150.0, 300.0, "cta")      # nothing new happens
    # the defaults of the existing options do not move
    assert (o.mip_dir, o.mip_mode, o.slab, o.aspect, o.wc, o.ww, o.batch, o.hu, o.level_dir, o.dtype, o.rot_dir, o.rot_angles) == \
        (None, "max", None, 1.0, 50.0, 400.0, 16, False, None, None, None, 36)
    o = predict.parse_args(base + ["--sub-output", "sub.npy", "--sub-level-dir", "lv", "--sub-floor", "60", "--sub-no-median",
                                   "--sub-ct-min", "-900", "--sub-ct-max", "400", "--sub-wc", "100", "--sub-ww", "200",
                                   "--mip-dir", "mip", "--mip-source", "sub"])
    assert (o.sub_output, o.sub_level_dir, o.sub_floor, o.sub_no_median, o.sub_ct_min, o.sub_ct_max, o.sub_wc, o.sub_ww,
            o.mip_source) == ("sub.npy", "lv", 60, True, -900, 400, 100.0, 200.0, "sub")
    for bad in (["--mip-dir", "mip", "--mip-source", "sub"], ["--sub-level-dir", "lv"], ["--mip-source", "bone"],
                ["--sub-output", "s.npy", "--sub-ct-min", "5", "--sub-ct-max", "4"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
