"""CPU: lines in any direction (csrc/reformat.hip: ctg_reformat_lines; ops.LineTable, ops.reformat_lines; infer.view_lines,
orbit_lines, oblique_lines, curved_lines, VolumeReformatter; predict.py --mpr-dir / --tumble-dir / --cpr-dir) -- the entry point
is declared and bound; the range check of the line table; the numpy restatement the GPU tests compare against
(tests/reformat_np.py) reproduces the restatements of the rotating and the axis projections where a line table can express
them; the trilinear value; the pins of the host geometry, evaluated through the restatement; a helical vessel that the curved
reformat follows and a plane does not; the refusals that need no GPU."""
import math
import os

import numpy as np
import pytest

import project_np
import reformat_np
import rotate_lerp_np
import rotate_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, SIG = "ctg_reformat_lines", "piiipiiiiiiffippp"
MODES = ["max", "min", "mean"]
ANGLES = [0, 30, 45, 90, 200]


def planted(n, h, w, seed):
    """Random int16 with both extremes planted; the last slice is all 32767 (the largest sums a mean can meet)."""
    vol = np.random.RandomState(seed).randint(-32768, 32768, size=(n, h, w)).astype(np.int16)
    vol[0, 0, 0], vol[0, h - 1, w - 1], vol[n // 2, h // 2, w // 2] = -32768, 32767, -32768
    if n > 1:
        vol[n - 1] = 32767
    return vol


# ---------------------------------------------------------------------------------------------- the entry and the table's range
def test_header_and_binding_carry_the_entry():
    from cta_gan_amd import _lib, ops
    from test_abi import parse_header
    assert parse_header().get(NAME) == SIG and _lib.SIGNATURES.get(NAME) == SIG
    assert ops.REFORMAT_SAMPLINGS == {"nearest": 0, "trilinear": 1}
    text = open(os.path.join(ROOT, "include", "ctagan_hip.h")).read()
    comment = text.split("int " + NAME + "(")[0][-4500:]
    assert "added under ABI 15: purely additive" in comment and "infer.py" in comment
    assert _lib.ABI_VERSION == 15 and "#define CTG_ABI_VERSION 15" in text
    src = open(os.path.join(ROOT, "cta_gan_amd", "csrc", "reformat.hip")).read()
    assert 'extern "C" int ' + NAME + "(" in src and src.count('extern "C"') == 1      # no other symbol


@pytest.mark.parametrize("u,t", [(1, 1), (33, 1), (1, 70), (4096, 4096), (31, 9)])
def test_line_table_accepts_a_sum_of_2_31_minus_1_and_refuses_2_31(u, t):
    from cta_gan_amd import ops
    cu, ck = 163840, -70000      # a step of 2.5 voxels along the line is in range
    top = 2 ** 31 - 1 - cu * (u - 1) - abs(ck) * (t - 1)
    for axis in range(3):
        for sign in (1, -1):
            row = np.zeros((2, 9), dtype=np.int64)
            row[1, 3 * axis:3 * axis + 3] = sign * top, -sign * cu, ck
            host = ops.line_table_host(row, u, t)
            assert host.dtype == np.int32 and host.shape == (2, 9) and np.array_equal(host, row)
            row[1, 3 * axis] += sign
            for make in (lambda: ops.line_table_host(row, u, t), lambda: ops.LineTable(row, u, t)):
                with pytest.raises(RuntimeError, match="out of range"):
                    make()
    assert ops.line_table_host(np.zeros((2, 3, 9), dtype=np.int32), u, t).shape == (2, 3, 9)      # any leading shape
    for bad in (np.zeros((2, 8), dtype=np.int64), np.zeros((0, 9), dtype=np.int64), np.zeros((2, 9)), np.zeros(9, dtype=np.int64)[:0]):
        with pytest.raises(RuntimeError):
            ops.line_table_host(bad, u, t)
    for bu, bt in ((0, 1), (1, 0), (4097, 1), (1, 4097)):
        with pytest.raises(RuntimeError):
            ops.line_table_host(np.zeros((1, 9), dtype=np.int64), bu, bt)


# ---------------------------------------------------------------------------------------------- against the existing oracles
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 33, 31)], ids=lambda s: "%dx%dx%d" % s)
def test_an_orbit_about_z_reproduces_the_rotating_projections(shape):
    """The pin of orbit_lines first: the x and y columns are the six integers of rotation_coefficients, z0 = (r << 16) + 32768 and
    zu = zk = 0; then the restatement on that table equals rotate_np (nearest) and rotate_lerp_np (trilinear: fz = 0) bit for bit."""
    from cta_gan_amd.infer import default_detector, orbit_lines, rotation_coefficients
    n, h, w = shape
    vol = planted(n, h, w, seed=h)
    d = default_detector(h, w)
    for s in (1, 2):
        lines, steps = orbit_lines(n, h, w, ANGLES, axis="z", rows=n, cols=d, depth=d, oversample=s)
        assert lines.shape == (len(ANGLES), n, 9) and steps == d * s and lines.dtype == np.int64
        coef = np.array([rotation_coefficients(a, h, w, oversample=s) for a in ANGLES], dtype=np.int64)
        assert np.array_equal(lines[:, :, :6], np.repeat(coef[:, None, :], n, axis=1))
        assert np.array_equal(lines[:, :, 6], np.repeat(((np.arange(n) << 16) + 32768)[None, :], len(ANGLES), axis=0))
        assert (lines[:, :, 7:] == 0).all()
        for mode in MODES:
            got, cnt = reformat_np.reformat(vol, lines, d, steps, mode, "nearest", fill=-7)
            assert np.array_equal(got, rotate_np.rotate(vol, coef, d, steps, mode, fill=-7))
            assert np.array_equal(cnt, np.repeat(rotate_np.count(h, w, coef, d, steps)[:, None, :], n, axis=1))
            got, _ = reformat_np.reformat(vol, lines, d, steps, mode, "trilinear", fill=-7)
            assert np.array_equal(got, rotate_lerp_np.rotate(vol, coef, d, steps, mode, fill=-7))
    assert (cnt == 0).any() and (cnt > 0).any()


@pytest.mark.parametrize("sampling", reformat_np.SAMPLINGS)
def test_a_slab_of_the_whole_volume_along_z_is_the_axial_projection(sampling):
    from cta_gan_amd.infer import oblique_lines
    n, h, w = 6, 5, 9
    vol = planted(n, h, w, seed=2)
    made = oblique_lines(n, h, w, (0, 0, 1), thick=n)
    lines, steps = made
    assert lines.shape == (1, h, 9) and steps == n and made.cols == w
    for mode in MODES:
        got, cnt = reformat_np.reformat(vol, lines, w, steps, mode, sampling)
        assert (cnt == n).all() and np.array_equal(got[0], project_np.project(vol, mode)[0][0]), mode


# ---------------------------------------------------------------------------------------------- the trilinear value
def test_trilinear_keeps_a_constant_volume_constant_and_returns_the_voxel_at_integer_positions():
    from cta_gan_amd import ops
    assert tuple(ops.REFORMAT_SAMPLINGS) == reformat_np.SAMPLINGS      # the restatement's samplings are the binding's
    rng = np.random.RandomState(5)
    n, h, w = 4, 5, 6
    pos = [rng.randint(-70000, (s << 16) + 70000, size=4000).astype(np.int64) for s in (w, h, n)]
    for value in (-32768, 32767, 1234):
        got = reformat_np.sample(np.full((n, h, w), value, dtype=np.int16), pos[0], pos[1], pos[2], "trilinear")
        assert (got == value).all(), value
    vol = planted(n, h, w, seed=6)
    z, y, x = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
    centre = [(c.astype(np.int64) << 16) + 32768 for c in (x, y, z)]      # an integer position carries the + 0.5
    assert np.array_equal(reformat_np.sample(vol, *centre, "trilinear"), vol)
    assert np.array_equal(reformat_np.sample(vol, *centre, "nearest"), vol)
    # half way between two slices, columns or rows: the mean of the two voxels, halves rounded up
    for axis in range(3):
        moved = [c + (32768 if a == axis else 0) for a, c in enumerate(centre)]
        a, b = vol.astype(np.int64), np.roll(vol.astype(np.int64), -1, axis=2 - axis)
        keep = [slice(None)] * 3
        keep[2 - axis] = slice(0, -1)
        assert np.array_equal(reformat_np.sample(vol, *moved, "trilinear")[tuple(keep)], ((a + b + 1) >> 1)[tuple(keep)]), axis


# ---------------------------------------------------------------------------------------------- the pins of the host geometry
@pytest.mark.parametrize("sampling", reformat_np.SAMPLINGS)
def test_oblique_planes_along_the_axes_return_the_stored_volume(sampling):
    from cta_gan_amd.infer import oblique_lines
    n, h, w = 4, 5, 7
    vol = planted(n, h, w, seed=3)
    for normal, count, want in (((0, 0, 1), n, vol), ((0, 1, 0), h, vol.transpose(1, 0, 2)), ((1, 0, 0), w, vol.transpose(2, 0, 1)),
                                ("z", n, vol), ((0, 0, 2.5), n, vol)):
        made = oblique_lines(n, h, w, normal, count=count, pitch=1.0)
        lines, steps = made
        assert steps == 1 and lines.shape == want.shape[:2] + (9,) and made.cols == want.shape[2]
        got, cnt = reformat_np.reformat(vol, lines, made.cols, 1, "max", sampling)
        assert (cnt == 1).all() and np.array_equal(got, want), normal
    # in-kernel anisotropy: at aspect 2 the coronal plane has 2 n rows and every slice shows twice under nearest sampling
    lines, _ = oblique_lines(n, h, w, (0, 1, 0), count=h, aspect=2.0)
    assert lines.shape == (h, 2 * n, 9)
    got, _ = reformat_np.reformat(vol, lines, w, 1, "max", "nearest")
    assert np.array_equal(got, np.repeat(vol.transpose(1, 0, 2), 2, axis=1))


@pytest.mark.parametrize("sampling", reformat_np.SAMPLINGS)
def test_a_straight_centreline_along_z_reads_the_columns_beside_it(sampling):
    from cta_gan_amd.infer import curved_lines
    n, h, w = 6, 7, 9
    vol = planted(n, h, w, seed=4)
    y0, x0, cols = 3, 4, 5
    for pts in ([[0, y0, x0], [n - 1, y0, x0]], [[0, y0, x0], [2, y0, x0], [2.5, y0, x0], [n - 1, y0, x0]]):
        made = curved_lines(n, h, w, pts, cols=cols)
        lines, steps = made
        assert lines.shape == (1, n, 9) and steps == 1 and made.cols == cols
        got, cnt = reformat_np.reformat(vol, lines, cols, 1, "max", sampling)
        assert (cnt == 1).all() and np.array_equal(got[0], vol[:, y0, x0 - 2:x0 + 3])
    # a quarter turn about the line reads the rows beside it instead, up or down
    lines, _ = curved_lines(n, h, w, pts, angles=(0.0, 90.0), cols=cols)
    got, _ = reformat_np.reformat(vol, lines, cols, 1, "max", "nearest")
    assert np.array_equal(got[0], vol[:, y0, x0 - 2:x0 + 3])
    assert np.array_equal(got[1], vol[:, y0 - 2:y0 + 3, x0]) or np.array_equal(got[1], vol[:, y0 - 2:y0 + 3, x0][:, ::-1])


def test_a_tumble_at_a_quarter_turn_is_the_axial_view():
    """Turned by 90 degrees about x, the coronal view looks along z: a max over its rays is the axial MIP, its rows the image rows
    in one order or the other."""
    from cta_gan_amd.infer import orbit_lines
    n, h, w = 5, 6, 7
    vol = planted(n, h, w, seed=8)
    lines, steps = orbit_lines(n, h, w, [90.0], axis="x", rows=h, cols=w, depth=n)
    got, cnt = reformat_np.reformat(vol, lines, w, steps, "max", "nearest")
    axial = project_np.project(vol, "max")[0][0]
    assert (cnt == n).all() and (np.array_equal(got[0], axial) or np.array_equal(got[0], axial[::-1]))
    made = orbit_lines(n, h, w, [0.0, 45.0], axis=(1, 1, 1))
    lines, steps = made      # the defaults see the whole volume at every angle
    d = int(math.ceil(math.sqrt(n * n + h * h + w * w)))
    assert lines.shape == (2, d, 9) and steps == d and made.cols == d
    got, _ = reformat_np.reformat(vol, lines, d, steps, "max", "nearest", fill=-32768)
    assert got[0].max() == vol.max() == got[1].max()


# ---------------------------------------------------------------------------------------------- a vessel
def test_the_curved_reformat_follows_a_helical_vessel_and_a_plane_does_not():
    from cta_gan_amd.infer import curved_lines, oblique_lines
    n, h, w = 40, 48, 44
    turn = np.linspace(0.0, 3.0 * math.pi, 400)
    helix = np.stack([3.0 + 33.0 * turn / turn[-1], 24.0 + 12.0 * np.sin(turn), 22.0 + 12.0 * np.cos(turn)], axis=1)      # (z, y, x)
    z, y, x = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
    grid = np.stack([z, y, x], axis=-1).reshape(-1, 1, 3).astype(np.float32)
    near = np.concatenate([((grid[s:s + 8192] - helix[None].astype(np.float32)) ** 2).sum(axis=2).min(axis=1)
                           for s in range(0, len(grid), 8192)])
    vol = np.where(near.reshape(n, h, w) <= 2.5 ** 2, 1000, 0).astype(np.int16)      # a tube of radius 2.5 voxels, background 0
    assert 0 < (vol == 1000).mean() < 0.05
    lines, steps = curved_lines(n, h, w, helix, cols=21)
    rows = lines.shape[1]
    assert rows > 100 and steps == 1      # the helix is about 118 voxels long
    got, cnt = reformat_np.reformat(vol, lines, 21, 1, "max", "trilinear")
    assert (cnt[0, :, 10] == 1).all() and (got[0, :, 10] == 1000).all()      # the core of the vessel, on every row
    assert (got[0, :, 0] == 0).all() and (got[0, :, 20] == 0).all()           # 10 voxels to either side: background
    cut = oblique_lines(n, h, w, (0, 1, 0))      # the coronal plane through the centre of the same volume
    flat, _ = reformat_np.reformat(vol, cut[0], cut.cols, 1, "max", "trilinear")
    assert (flat[0] != 1000).mean() >= 0.5 and (flat[0][:, cut.cols // 2] != 1000).mean() >= 0.5
    assert (flat[0] == 1000).any()      # it does cut the vessel, where the helix crosses it


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_that_need_no_gpu():
    from cta_gan_amd.infer import SeriesTranslator, VolumeReformatter, curved_lines, oblique_lines, orbit_lines, view_lines
    x, y, z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    for basis in ((x, y, (0, 0, 2)), (x, x, z), (x, y, (0, 0.1, 1)), (x, y, (0, 0)), (x, y, "w")):      # not orthonormal, or not a basis
        with pytest.raises(ValueError):
            view_lines(4, 5, 6, *basis, rows=5, cols=6)
    assert view_lines(4, 5, 6, x, y, z, rows=5, cols=6)[0].shape == (5, 9)
    for kw in (dict(rows=0), dict(cols=0), dict(cols=4097), dict(depth=0), dict(depth=2049, oversample=2), dict(oversample=0),
               dict(aspect=0.0), dict(aspect=-1.0)):
        args = dict(rows=5, cols=6)
        args.update(kw)
        with pytest.raises(ValueError):
            view_lines(4, 5, 6, x, y, z, **args)
    for pts in ([[0, 1, 2]], np.zeros((0, 3)), np.zeros((3, 2)), [[0, 1, 2], [0, 1, 2]], [[0, 1, 2], [1, 1, float("nan")]]):      # M < 2 ...
        with pytest.raises(ValueError):
            curved_lines(4, 5, 6, pts)
    with pytest.raises(ValueError):
        oblique_lines(4, 5, 6, (0, 0, 0))
    with pytest.raises(ValueError):
        oblique_lines(4, 5, 6, (0, 0, 1), up=(0, 0, -1))      # up along the normal
    with pytest.raises(ValueError):
        orbit_lines(4, 5, 6, [0.0], axis="w")
    with pytest.raises(ValueError):
        orbit_lines(4, 5, 6, [])
    tables = {"planes": lambda n, h, w: oblique_lines(n, h, w, (0, 1, 1))}
    for kw in (dict(sampling="cubic"), dict(sampling="bilinear"), dict(mode="median"), dict(tables={}),
               dict(tables={"a": (np.zeros((2, 9), dtype=np.int64), 1)})):      # (a bare pair needs cols)
        args = dict(tables=tables)
        args.update(kw)
        with pytest.raises(ValueError):
            VolumeReformatter(4, 5, 6, **args)
    with pytest.raises(RuntimeError, match="out of range"):
        VolumeReformatter(4, 5, 6, {"a": (np.full((2, 9), 2 ** 30, dtype=np.int64), 3)}, cols=2)
    ref = VolumeReformatter(4, 5, 6, tables)
    assert ref.nbytes == 2 * 4 * 5 * 6 + ref.lines["planes"][0].size * 4 + 3 * ref.lines["planes"][0].size // 9 * ref.lines["planes"][1]
    with pytest.raises(RuntimeError, match="exactly once"):
        ref.result()      # before any slice has arrived
    with pytest.raises(ValueError):
        SeriesTranslator(None, reformat_options={"mode": "max"})      # options without tables
    with pytest.raises(ValueError):
        SeriesTranslator(None, reformat=tables, reformat_options={"angle": 3})
    with pytest.raises(ValueError):
        SeriesTranslator(None, reformat={})


def test_predict_options():
    import predict
    base = ["--weights", "w", "--input", "i", "--output", "o"]
    o = predict.parse_args(base)
    assert o.mpr_dir is None and o.tumble_dir is None and o.cpr_dir is None and o.reformat_sampling == "trilinear"
    o = predict.parse_args(base + ["--mpr-dir", "m", "--mpr-normal", "1,0.5,0", "--mpr-count", "3", "--mpr-pitch", "2.5", "--mpr-thick",
                                   "4", "--tumble-dir", "t", "--tumble-angles", "8", "--tumble-axis", "y", "--cpr-dir", "c",
                                   "--cpr-centreline", "p.npy", "--cpr-angles", "2", "--cpr-width", "33", "--cpr-thick", "3",
                                   "--reformat-sampling", "nearest"])
    assert o.mpr_normal == (1.0, 0.5, 0.0) and (o.mpr_count, o.mpr_pitch, o.mpr_thick) == (3, 2.5, 4)
    assert (o.tumble_angles, o.tumble_axis) == (8, "y") and (o.cpr_angles, o.cpr_width, o.cpr_thick) == (2, 33, 3)
    assert o.reformat_sampling == "nearest"
    for bad in (["--mpr-dir", "m"], ["--mpr-normal", "0,0,1"], ["--mpr-dir", "m", "--mpr-normal", "0,0"],
                ["--mpr-dir", "m", "--mpr-normal", "0,0,0"], ["--mpr-dir", "m", "--mpr-normal", "a,b,c"], ["--cpr-dir", "c"],
                ["--cpr-centreline", "p.npy"], ["--tumble-dir", "t", "--tumble-angles", "0"], ["--tumble-dir", "t", "--tumble-axis", "w"],
                ["--reformat-sampling", "bilinear"], ["--mpr-dir", "m", "--mpr-normal", "0,0,1", "--mpr-pitch", "0"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
    for flag in ("--mpr-normal X,Y,Z", "--tumble-axis x|y|z", "--cpr-centreline pts.npy", "--reformat-sampling nearest|trilinear"):
        assert flag in predict.__doc__ and flag in open(os.path.join(ROOT, "README.md")).read(), flag
