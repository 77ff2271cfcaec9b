"""CPU: the depth of the maximum (csrc/project_rotate.hip: ctg_project_rotate_depth; csrc/project.hip:
ctg_project_accumulate_depth, ctg_project_finish_depth; infer.py: depth=True, ray_voxel; predict.py --depth / --depth-cue) -- the
three entries are declared, bound and exported under ABI 15; the numpy restatement the GPU tests compare against
(tests/depth_np.py) agrees with cases worked out by hand; the depth cue is the identity at 0, monotone in the depth and keeps
1 <= w <= 256; ray_voxel is the kernel's nearest rule; the host refuses a mean and a cue out of range."""
import ctypes
import os
import sys

import numpy as np
import pytest

import depth_np
import project_np
import rotate_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "ctg_project_rotate_depth": ("piiiiipiiiiiiiffippppp", "project_rotate.hip", "ctg_project_rotate_bilinear"),
    "ctg_project_accumulate_depth": ("piiiiiipppp", "project.hip", "ctg_project_accumulate"),
    "ctg_project_finish_depth": ("piliiiiffippppp", "project.hip", "ctg_project_finish"),
}


# ---------------------------------------------------------------------------------------------- the entries
def test_header_and_binding_carry_the_entries():
    from cta_gan_amd import _lib, ops
    from test_abi import parse_header
    decls = parse_header()
    text = open(os.path.join(ROOT, "include", "ctagan_hip.h")).read()
    for name, (sig, source, extends) in ENTRIES.items():
        assert decls.get(name) == sig and _lib.SIGNATURES.get(name) == sig, name
        assert text.index("int %s(" % extends) < text.index("int %s(" % name)      # declared after the entry it extends
        src = open(os.path.join(ROOT, "cta_gan_amd", "csrc", source)).read()
        assert 'extern "C" int ' + name + "(" in src
    comment = text.split("int ctg_project_rotate_depth(")[0][-6000:]
    assert "added under ABI 15: purely additive" in comment and "infer.py" in comment
    assert "key = b << 16 | (65535 - d)" in comment and "key = b << 16 | d" in comment
    assert _lib.ABI_VERSION == 15 and "#define CTG_ABI_VERSION 15" in text
    # what exists keeps its meaning
    assert ops.ROTATE_SAMPLINGS == {"nearest": "ctg_project_rotate", "bilinear": "ctg_project_rotate_bilinear"}
    assert ops.PROJECT_IDENTITY == (-32768, 32767, 0) and ops.PROJECT_DEPTH_IDENTITY == (0, -1)
    for name in ("project_rotate_depth", "project_accumulate_depth", "project_finish_depth"):
        assert callable(getattr(ops, name))


def test_built_library_exports_the_entries():
    from cta_gan_amd import build
    lib = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert hasattr(lib, name), name


# ---------------------------------------------------------------------------------------------- depth_np, by hand
def hand_slice():
    """5 x 7, zero but for a doubled maximum 9 in column 2, rows 1 and 2, and a doubled minimum -4 in column 5, rows 0 and 4."""
    sl = np.zeros((1, 5, 7), dtype=np.int16)
    sl[0, 1, 2] = sl[0, 2, 2] = 9
    sl[0, 0, 5] = sl[0, 4, 5] = -4
    return sl


def test_a_doubled_maximum_seen_from_the_front_and_from_the_back():
    sl = hand_slice()
    # 0 degrees, detector 7, rays of 5: sample (u, t) is pixel (x, y) = (u, t); 180 degrees: (6 - u, 4 - t)
    coef = [rotate_np.coefficients(0, 5, 7, 7, 5), rotate_np.coefficients(180, 5, 7, 7, 5)]
    assert coef[0] == [32768, 65536, 0, 32768, 0, 65536] and coef[1] == [425984, -65536, 0, 294912, 0, -65536]
    values, depth = depth_np.rotate_depth(sl, coef, 7, 5, "max")
    # front: column 2 is ray 2, rows 1 and 2 are steps 1 and 2: the nearer one, step 1.  Column 5: 0 first at row 1 (row 0 is -4)
    assert values[0, 0].tolist() == [0, 0, 9, 0, 0, 0, 0] and depth[0, 0].tolist() == [0, 0, 1, 0, 0, 1, 0]
    # back: column 2 is ray 4; row 2 is step 2, row 1 is step 3: the nearer one is now row 2.  Column 5 is ray 1: row 3 at step 1
    assert values[1, 0].tolist() == [0, 0, 0, 0, 9, 0, 0] and depth[1, 0].tolist() == [0, 1, 0, 0, 2, 0, 0]
    values, depth = depth_np.rotate_depth(sl, coef, 7, 5, "min")
    assert values[0, 0].tolist() == [0, 0, 0, 0, 0, -4, 0] and depth[0, 0].tolist() == [0, 0, 0, 0, 0, 0, 0]
    assert values[1, 0].tolist() == [0, -4, 0, 0, 0, 0, 0] and depth[1, 0].tolist() == [0, 0, 0, 0, 0, 0, 0]
    # the values are those of the plain restatement
    for mode in depth_np.MODES:
        assert np.array_equal(depth_np.rotate_depth(sl, coef, 7, 5, mode)[0], rotate_np.rotate(sl, coef, 7, 5, mode))


def test_a_missed_ray_has_depth_minus_one_and_the_fill():
    sl = hand_slice()
    # a detector of 9 columns: cu = 4, so ray u looks at column u - 1; rays 0 and 8 miss the slice.  Rays of 7 steps: ct = 3, so
    # step t is row t - 1: steps 0 and 6 are not counted, and the depth counts them all the same (it is the step index)
    coef = [rotate_np.coefficients(0, 5, 7, 9, 7)]
    assert coef[0] == [-32768, 65536, 0, -32768, 0, 65536]
    assert rotate_np.count(5, 7, coef, 9, 7).tolist() == [[0, 5, 5, 5, 5, 5, 5, 5, 0]]
    values, depth = depth_np.rotate_depth(sl, coef, 9, 7, "max", fill=-77)
    assert values[0, 0].tolist() == [-77, 0, 0, 9, 0, 0, 0, 0, -77]
    assert depth[0, 0].tolist() == [-1, 1, 1, 2, 1, 1, 2, 1, -1]
    values, depth = depth_np.rotate_depth(sl, coef, 9, 7, "min", fill=5)
    assert values[0, 0].tolist() == [5, 0, 0, 0, 0, 0, -4, 0, 5] and depth[0, 0].tolist() == [-1, 1, 1, 1, 1, 1, 1, 1, -1]
    # the cue leaves a missed ray alone: w = 256
    level = np.full((9,), 200, dtype=np.uint8)
    assert depth_np.cued(level, 256, depth[0, 0], 7).tolist() == [200] + [(200 * (256 - 256 // 7) + 128) >> 8] * 7 + [200]


def test_bilinear_depth_at_a_cardinal_angle_is_the_nearest_one():
    vol = np.random.RandomState(5).randint(-32768, 32768, size=(2, 5, 7)).astype(np.int16)
    vol[0, 1, 3] = vol[0, 3, 3] = 32767
    coef = [rotate_np.coefficients(a, 5, 7, 7, 5) for a in (0, 180)]
    for mode in depth_np.MODES:
        a, b = depth_np.rotate_depth(vol, coef, 7, 5, mode, "nearest"), depth_np.rotate_depth(vol, coef, 7, 5, mode, "bilinear")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert depth_np.rotate_depth(vol, coef, 7, 5, "max")[1][:, 0, 3].tolist() == [1, 1]


def test_axis_projections_by_hand():
    vol = np.zeros((5, 2, 3), dtype=np.int16)
    vol[1, 0, 0] = vol[3, 0, 0] = 7         # a doubled maximum along the slices: slice 1 whole, slices 1 | 3 in slabs of 2
    vol[:, 1, 2] = [-3, -1, -1, -3, -2]     # a maximum -1 doubled inside the middle slab; a minimum -3 in slices 0 and 3
    out = depth_np.project_depth(vol, "max")
    assert out["axial"][0].tolist() == [[[7, 0, 0], [0, 0, -1]]] and out["axial"][1].tolist() == [[[1, 0, 0], [0, 0, 1]]]
    assert out["axial"][2].tolist() == [[[0]]] and out["axial"][3].tolist() == [[[5]]]
    out = depth_np.project_depth(vol, "max", thick=2)
    assert out["axial"][1].tolist() == [[[1, 0, 0], [0, 0, 1]], [[3, 2, 2], [2, 2, 2]], [[4, 4, 4], [4, 4, 4]]]      # global slices
    assert out["axial"][2].ravel().tolist() == [0, 2, 4] and out["axial"][3].ravel().tolist() == [2, 2, 1]      # a short last slab
    assert out["coronal"][0][1].tolist() == [7, 0, 0] and out["coronal"][1][1].tolist() == [0, 0, 0]
    assert out["coronal"][1][0].tolist() == [0, 0, 0] and out["coronal"][0][0].tolist() == [0, 0, 0]      # -3 below row 0's 0
    assert out["sagittal"][0][1].tolist() == [7, 0] and out["sagittal"][1][1].tolist() == [0, 0]
    out = depth_np.project_depth(vol, "min")
    assert out["axial"][0][0, 1, 2] == -3 and out["axial"][1][0, 1, 2] == 0
    # slice 3 is [[7, 0, 0], [0, 0, -3]]: the column minima 0, 0, -3 sit in rows 1, 0, 1, the row minima 0, -3 in columns 1, 2
    assert out["coronal"][1][3].tolist() == [1, 0, 1] and out["sagittal"][1][3].tolist() == [1, 2]
    for mode in depth_np.MODES:      # the values are those of the plain restatement
        for thick in (None, 2):
            got = depth_np.project_depth(vol, mode, thick)
            for a, want in zip(("axial", "coronal", "sagittal"), project_np.project(vol, mode, thick)):
                assert np.array_equal(got[a][0], want), (mode, thick, a)


# ---------------------------------------------------------------------------------------------- the depth cue
@pytest.mark.parametrize("length", [1, 5, 37, 725, 4096])
def test_cue_properties(length):
    level = np.arange(256, dtype=np.uint8)[:, None]
    d = np.arange(length, dtype=np.int64)[None, :]
    assert np.array_equal(depth_np.cued(level, 0, d, length), np.broadcast_to(level, (256, length)))      # the identity at 0
    for cue in (0, 1, 128, 256):
        w = depth_np.cue_weight(cue, d, length)
        assert w.min() >= 1 and w.max() <= 256 and w[0, 0] == 256 and (np.diff(w, axis=1) <= 0).all()
        c = depth_np.cued(level, cue, d, length).astype(np.int64)
        assert (c <= level).all() and (np.diff(c, axis=1) <= 0).all() and (np.diff(c, axis=0) >= 0).all()      # monotone
        assert np.array_equal(depth_np.cued(level, cue, np.full((1, 1), -1), length), level)                    # a missed ray
        for dd in (0, length // 2, length - 1):      # the formula itself, in python integers
            assert w[0, dd] == 256 - (cue * dd) // length
    if length > 1:
        assert depth_np.cue_weight(256, length - 1, length) == 256 - 256 * (length - 1) // length >= 1


# ---------------------------------------------------------------------------------------------- picking
def test_ray_voxel_is_the_nearest_rule():
    from cta_gan_amd.infer import ray_voxel, rotation_coefficients
    h, w = 33, 31
    d = rotate_np.detector(h, w)
    for angle in (0, 90, 180, 45, 10, 137.5, -30, 359.9):
        for s in (1, 2):
            c = rotation_coefficients(angle, h, w, oversample=s)
            xi, yi, _ = rotate_np._samples(h, w, c, d, d * s)
            x, y = ray_voxel(c, np.arange(d)[:, None], np.arange(d * s)[None, :])
            assert np.array_equal(x, xi) and np.array_equal(y, yi)
            assert ray_voxel(c, 7, 11) == (int(xi[7, 11]), int(yi[7, 11])) and all(type(v) is int for v in ray_voxel(c, 7, 11))
    with pytest.raises(ValueError):
        ray_voxel([1, 2, 3], 0, 0)


# ---------------------------------------------------------------------------------------------- the host's arguments
def test_a_mean_and_a_cue_out_of_range_are_refused():
    from cta_gan_amd.infer import SeriesProjector, SeriesRotator, SeriesTranslator
    for kw in (dict(mode="mean", depth=True), dict(depth=True, cue=257), dict(depth=True, cue=-1), dict(depth=True, cue=1.5),
               dict(depth=True, cue=True), dict(cue=10)):
        with pytest.raises(ValueError):
            SeriesRotator(4, 8, 8, [0.0], **kw)
        with pytest.raises(ValueError):
            SeriesProjector(4, 8, 8, **kw)
    with pytest.raises(ValueError):
        SeriesProjector(32768, 8, 8, depth=True)      # a depth is an int16
    for kw in (dict(project="mean", depth=True), dict(rotate=3, rotate_mode="mean", depth=True), dict(depth=True),
               dict(project="max", depth=True, depth_cue=300), dict(project="max", depth_cue=5),
               dict(project="max", rotate=3, rotate_mode="mean", depth=True)):
        with pytest.raises(ValueError):
            SeriesTranslator(None, **kw)


def test_predict_depth_arguments():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import predict
    base = ["--weights", "g.pth", "--input", "in.npy", "--output", "out.npy"]
    o = predict.parse_args(base)
    assert (o.depth, o.depth_cue) == (False, 0)
    o = predict.parse_args(base + ["--rot-dir", "rot", "--depth", "--depth-cue", "128"])
    assert (o.depth, o.depth_cue) == (True, 128)
    for bad in (["--depth"], ["--rot-dir", "rot", "--depth-cue", "5"], ["--rot-dir", "rot", "--depth", "--depth-cue", "257"],
                ["--rot-dir", "rot", "--depth", "--mip-mode", "mean"], ["--mip-dir", "m", "--depth", "--depth-cue", "-1"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
    assert "--depth" in predict.__doc__ and "--depth-cue C" in predict.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--depth" in readme and "--depth-cue C" in readme
