"""CPU: the host geometry of the lumen sections (infer.lumen_lines), the refusals that need no GPU, the accuracy of the rule itself
(tests/lumen_np.py, the restatement csrc/lumen.hip is compared with on the GPU) on voxelised discs of known size and centre, the
"half" edge, the host measurements (lumen_profile, lumen_stenosis) on a profile with a known narrowing, and the ABI entries."""
import functools
import math
import os

import numpy as np
import pytest

import lumen_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = "piiip" + "i" * 9 + "ppppp"
TRUE = (20.6, 19.3)      # (x, y) of every disc's centre
RADII = (2.0, 3.5, 6.0)


def test_header_binding_and_source_carry_the_entry():
    from cta_gan_amd import _lib, ops
    from test_abi import parse_header
    assert parse_header().get("ctg_lumen_sections") == SIG and _lib.SIGNATURES.get("ctg_lumen_sections") == SIG
    text = open(os.path.join(ROOT, "include", "ctagan_hip.h")).read()
    comment = text.split("int ctg_lumen_sections(")[0][-6000:]
    assert "added under ABI 15: purely additive" in comment and "infer.py" in comment and "tests/lumen_np.py" in comment
    assert _lib.ABI_VERSION == 15 and "#define CTG_ABI_VERSION 15" in text
    src = open(os.path.join(ROOT, "cta_gan_amd", "csrc", "lumen.hip")).read()
    assert src.count('extern "C"') == 1 and 'extern "C" int ctg_lumen_sections(' in src
    assert "#define LUM_MAX_STEPS %d " % ops.LUMEN_MAX_STEPS in src and "#define LUM_MAX_RECENTRE %d\n" % ops.LUMEN_MAX_RECENTRE in src
    assert ops.LUMEN_RAYS == (8, 16, 32, 64) == lumen_np.RAYS and tuple(ops.LUMEN_EDGES) == lumen_np.EDGES
    assert len(ops.LUMEN_SECTIONS) == 8 and ops.LUMEN_SECTIONS[5:7] == ("open", "outside")


# ---------------------------------------------------------------------------------------------- 1. geometry
def test_a_straight_line_along_z_gives_rays_in_the_slice_plane():
    from cta_gan_amd.infer import LumenSet, lumen_lines
    n, h, w = 9, 30, 40
    made = lumen_lines(n, h, w, [[0, 11, 17], [n - 1, 11, 17]], rays=16, reach=5.0, oversample=2)
    table, steps = made
    assert isinstance(made, LumenSet) and isinstance(made, tuple) and (made.rays, made.steps, made.oversample) == (16, 11, 2)
    assert steps == math.floor(5.0 * 2) + 1 and table.shape == (n, 16, 9) and table.dtype == np.int64
    assert np.array_equal(made.arc, np.arange(n, dtype=np.float64))
    for r in range(n):
        for j in range(16):
            x0, xu, xk, y0, yu, yk, z0, zu, zk = table[r, j]
            assert (x0, y0, z0) == ((17 << 16) + 32768, (11 << 16) + 32768, (r << 16) + 32768) and (xu, yu, zu) == (0, 0, 0)
            assert zk == 0      # in the slice plane
            assert xk == math.floor(math.cos(2 * math.pi * j / 16) / 2 * 65536 + 0.5)
            assert yk == math.floor(math.sin(2 * math.pi * j / 16) / 2 * 65536 + 0.5)
    assert tuple(table[0, 0, [2, 5, 8]]) == (32768, 0, 0)      # ray 0 runs along +x, half a pixel per step
    assert tuple(table[0, 4, [2, 5, 8]]) == (0, 32768, 0)      # a quarter turn on: +y


def test_rows_and_steps_follow_the_formulas_and_aspect_scales_z_only():
    from cta_gan_amd.infer import curved_lines, lumen_lines
    pts = [[1.0, 3.0, 4.0], [4.0, 9.5, 7.0], [9.0, 12.0, 15.0]]
    for pitch, reach, s, aspect in ((1.0, 16.0, 2, 1.0), (0.6, 3.3, 3, 2.5), (2.0, 255.0, 1, 0.7)):
        made = lumen_lines(12, 20, 24, pts, rays=8, reach=reach, pitch=pitch, oversample=s, aspect=aspect)
        p = np.asarray(pts)[:, ::-1] * np.array([1.0, 1.0, aspect])
        length = np.sqrt(((p[1:] - p[:-1]) ** 2).sum(axis=1)).sum()
        assert made[0].shape == (math.floor(length / pitch + 1e-9) + 1, 8, 9) and made.steps == math.floor(reach * s) + 1
        assert np.allclose(made.arc, np.arange(len(made.arc)) * pitch)
        # the sections sit on the rows of the curved reformat: the same resampling and the same frame
        cpr = curved_lines(12, 20, 24, pts, cols=1, pitch=pitch, aspect=aspect)[0][0]      # cols 1: the row starts on the line
        assert np.array_equal(cpr[:, 0::3], made[0][:, 0, 0::3])
        # ray 0 is e1, the reformat's `right` at angle 0, in steps of 1 / s
        right = cpr[:, 1::3] / 65536.0
        assert np.abs(made[0][:, 0, 2::3] / 65536.0 * s - right).max() < 2e-5 * s
    # aspect: z in the table is z in pixel units over the aspect, x and y are untouched
    one = lumen_lines(9, 30, 40, [[0, 11, 17], [8, 11, 17]], rays=8, reach=4.0, aspect=1.0)
    two = lumen_lines(9, 30, 40, [[0, 11, 17], [4, 11, 17]], rays=8, reach=4.0, aspect=2.0)      # the same 8 pixels of length
    assert one[0].shape == two[0].shape == (9, 8, 9)
    assert np.array_equal(one[0][:, :, :6], two[0][:, :, :6])
    assert np.array_equal(two[0][:, 0, 6], ((np.arange(9) << 15) + 32768))      # z0 = r / 2 + 0.5


def test_refusals_that_need_no_gpu():
    from cta_gan_amd import ops
    from cta_gan_amd.infer import VolumeLumen, lumen_lines
    line = [[0, 5, 5], [7, 5, 5]]
    for rays in (0, 4, 12, 33, 128, True, 32.5):
        with pytest.raises(ValueError, match="rays"):
            lumen_lines(8, 12, 12, line, rays=rays)
        with pytest.raises(RuntimeError, match="rays"):
            ops.lumen_options("t", rays, 9, 100)
    for reach, s in ((0.4, 2), (0.0, 1), (-1.0, 1), (128.0, 2), (256.0, 1), (float("inf"), 1)):      # T = 1, 1, none, 257, 257, none
        with pytest.raises(ValueError, match="steps"):
            lumen_lines(8, 12, 12, line, reach=reach, oversample=s)
    assert lumen_lines(8, 12, 12, line, reach=0.5, oversample=2).steps == 2 and lumen_lines(8, 12, 12, line, reach=255.0, oversample=1).steps == 256
    for steps in (1, 257, 0, 2.5):
        with pytest.raises(RuntimeError, match="steps"):
            ops.lumen_options("t", 32, steps, 100)
    with pytest.raises(RuntimeError, match="base"):
        ops.lumen_options("t", 32, 9, 100, edge="half", base=101)
    with pytest.raises(RuntimeError, match="base"):
        ops.lumen_options("t", 32, 9, 100, edge="half")
    with pytest.raises(RuntimeError, match="base"):
        ops.lumen_options("t", 32, 9, 100, edge="band", base=0)
    assert ops.lumen_options("t", 32, 9, 100, edge="half", base=100)[6] == 100
    for recentre in (-1, 5, 1.5, True):
        with pytest.raises(RuntimeError, match="recentre"):
            ops.lumen_options("t", 32, 9, 100, recentre=recentre)
    with pytest.raises(RuntimeError, match="edge"):
        ops.lumen_options("t", 32, 9, 100, edge="full")
    with pytest.raises(RuntimeError, match="sampling"):
        ops.lumen_options("t", 32, 9, 100, sampling="bilinear")
    with pytest.raises(RuntimeError, match="band"):
        ops.lumen_options("t", 32, 9, 100, hi=99)
    # the same through the view, which checks everything on the host before a volume exists
    for bad in ({"rays": 12}, {"reach": 200.0}, {"edge": "half", "base": 501}, {"edge": "half"}, {"recentre": 5}, {"sampling": "cubic"}):
        with pytest.raises(ValueError):
            VolumeLumen(8, 12, 12, 500, line, **bad)
    with pytest.raises(ValueError, match="centreline"):
        VolumeLumen(8, 12, 12, 500, [[0, 5, 5]])
    # the range check: |c0| + (1 + 2 recentre) (T-1) max |ck| < 2^31
    table = np.zeros((2, 8, 9), dtype=np.int64)
    table[:, :, 2] = 1 << 16
    table[1, :, 0] = (1 << 31) - 1 - 15 * (1 << 16)
    assert ops.lumen_table_host(table, 8, 16, 0).dtype == np.int32
    with pytest.raises(RuntimeError, match="out of range"):
        ops.lumen_table_host(table, 8, 16, 1)      # the recentred walks reach three times as far
    with pytest.raises(RuntimeError, match="out of range"):
        ops.lumen_table_host(table, 8, 17, 0)
    table[1, 3, 0] += 1                            # any ray's start counts, and a negative one as much
    with pytest.raises(RuntimeError, match="out of range"):
        ops.lumen_table_host(table, 8, 16, 0)
    table[1, 3, 0] = -table[1, 3, 0]
    with pytest.raises(RuntimeError, match="out of range"):
        ops.lumen_table_host(table, 8, 16, 0)
    with pytest.raises(RuntimeError, match=r"\[R, 8, 9\]"):
        ops.lumen_table_host(np.zeros((2, 16, 9), dtype=np.int64), 8, 16, 0)
    with pytest.raises(ValueError, match="out of range"):
        VolumeLumen(8, 12, 12, 500, [[0, 5, 32000.0], [7, 5, 32000.0]], reach=127.5, recentre=4)


# ---------------------------------------------------------------------------------------------- 2. accuracy of the rule on discs
def disc(radius, fg=1000, bg=0, n=3, h=40, w=40):
    y, x = np.mgrid[0:h, 0:w]
    plane = np.where((x - TRUE[0]) ** 2 + (y - TRUE[1]) ** 2 <= radius * radius, fg, bg).astype(np.int16)
    return np.repeat(plane[None], n, axis=0)


def starts(radius):
    """Three starts per disc: the voxel nearest the truth, and two 1.8 and 2.7 px off it (0.9 and 1.0 px in the smallest disc, whose
    radius is 2)."""
    a, b = (0.9, 0.7) if radius < 3 else (1.8, 1.9)
    return ((21.0, 19.0), (TRUE[0] + a, TRUE[1]), (TRUE[0] - b, TRUE[1] + b))


@functools.lru_cache(maxsize=None)
def measured(radius, start, recentre, fg=1000, lo=500, edge="band", base=None):
    from cta_gan_amd.infer import lumen_lines
    vol = disc(radius, fg=fg)
    lines = lumen_lines(*vol.shape, [[0, start[1], start[0]], [2, start[1], start[0]]], rays=32, reach=16.0, oversample=2)
    radii, cross, sections, centres = lumen_np.sections(vol, lines[0], lines.steps, lo, 32767, "trilinear", edge, base, recentre)
    assert sections[1, 5] == 0 and sections[1, 6] == 0
    eq = float(lumen_np.equivalent_diameter(cross, 32)[1]) / (256 * 2)
    centre = centres[1, :2] / 65536.0 - 0.5
    return eq, float(np.hypot(centre[0] - TRUE[0], centre[1] - TRUE[1])), sections[1, 1] / 512.0


@pytest.mark.parametrize("radius", RADII)
def test_equivalent_diameter_and_recentred_centre_on_a_disc(radius):
    """K = 32, oversample 2, trilinear.  Measured (LAB_NOTES.md): |equivalent - 2R| <= 0.124 px and the recentred centre within
    0.133 px of the truth over the nine cases; the bounds are the issue's 0.25 px."""
    for start in starts(radius):
        for recentre in (0, 2):
            eq, off, _ = measured(radius, start, recentre)
            print("R %.1f start %s recentre %d: equivalent %.3f (2R %+.3f), centre off by %.3f" % (radius, start, recentre, eq, eq - 2 * radius, off))
            assert abs(eq - 2 * radius) <= 0.25
            if recentre == 2:
                assert off <= 0.25
        far = measured(radius, starts(radius)[2], 0)
        assert far[1] > 0.9      # (the start really was off centre)


def test_without_recentring_the_least_chord_measures_the_click():
    off, on = measured(6.0, starts(6.0)[2], 0), measured(6.0, starts(6.0)[2], 2)
    assert off[2] < 10.8 and abs(on[2] - 12.0) < 0.75 and on[2] > off[2] + 0.5


def test_eight_rays_lose_a_tenth_of_the_area():
    from cta_gan_amd.infer import lumen_lines
    vol = disc(6.0)
    areas = {}
    for rays in (8, 32):
        lines = lumen_lines(*vol.shape, [[0, 19.0, 21.0], [2, 19.0, 21.0]], rays=rays, oversample=2)
        _, cross, _, _ = lumen_np.sections(vol, lines[0], lines.steps, 500, recentre=2)
        areas[rays] = float(lumen_np.area(cross, rays)[1]) / 512.0 ** 2
    assert 0.85 < areas[8] / areas[32] < 0.95 and abs(areas[32] / (math.pi * 36.0) - 1.0) < 0.02


def test_edge_half_follows_the_lumens_own_density():
    """A disc of 400 over 0 with lo = 100: "half" with base 0 puts the wall at 200, half-way, and measures what the 1000 / 500 disc
    measures; the plain band puts it at 100, further out."""
    for radius in RADII:
        for start in starts(radius)[:2]:
            ref = measured(radius, start, 2)
            half = measured(radius, start, 2, fg=400, lo=100, edge="half", base=0)
            band = measured(radius, start, 2, fg=400, lo=100)
            assert abs(half[0] - ref[0]) <= 0.02 and abs(half[0] - 2 * radius) <= 0.25 and half[1] <= 0.25
            assert band[0] > half[0] + 0.2
    vol = disc(3.5, fg=400)
    from cta_gan_amd.infer import lumen_lines
    lines = lumen_lines(*vol.shape, [[0, 19.0, 21.0], [2, 19.0, 21.0]])
    sections = lumen_np.sections(vol, lines[0], lines.steps, 100, edge="half", base=0)[2]
    assert (sections[:, 7] == 200).all()
    assert (lumen_np.sections(vol, lines[0], lines.steps, 250, edge="half", base=0)[2][:, 7] == 250).all()      # never below lo


# ---------------------------------------------------------------------------------------------- 3. the host measurements
def synthetic(diameters, rays=32, oversample=2, bad=()):
    """The result tree of sections that are perfect polygons of the given diameters (pixels); `bad`: sections with an open ray."""
    rho = np.round(np.asarray(diameters, dtype=np.float64) * 0.5 * 256 * oversample).astype(np.int64)
    radii = np.repeat(rho[:, None], rays, axis=1)
    sections = np.zeros((len(rho), 8), dtype=np.int32)
    sections[:, 0], sections[:, 1], sections[:, 2] = rho * rays, 2 * rho, 2 * rho
    for i in bad:
        sections[i, 5] = 1
    return {"radii": radii.astype(np.int32), "cross": (radii * np.roll(radii, -1, axis=1)).sum(axis=1), "sections": sections,
            "centres": np.zeros((len(rho), 3), dtype=np.int32), "arc": np.arange(len(rho)) * 0.5, "oversample": np.array([oversample], dtype=np.int32)}


def test_profile_and_stenosis_of_a_known_narrowing():
    from cta_gan_amd.infer import lumen_profile, lumen_stenosis
    d = np.full(60, 4.0)
    d[28:33] = (3.0, 2.5, 2.0, 2.5, 3.0)      # 50 % by diameter at section 30
    d[2] = 1.0                                # inside the margin: not a candidate
    d[31] = 0.5                               # narrower still, but invalid
    tree = synthetic(d, bad=(31, 20))
    prof = lumen_profile(tree, pixel_mm=0.5)
    assert set(prof) == {"area", "equivalent", "dmin", "dmax", "mean", "arc", "valid"}
    assert prof["valid"].sum() == 58 and not prof["valid"][31] and not prof["valid"][20]
    poly = math.sqrt(0.5 * 32 * math.sin(2 * math.pi / 32) / math.pi)      # equivalent / true diameter of a 32-gon: 0.9968
    assert np.allclose(prof["equivalent"], d * 0.5 * poly, rtol=0, atol=2e-3)
    assert np.allclose(prof["dmin"], d * 0.5, atol=1e-3) and np.allclose(prof["dmax"], prof["dmin"]) and np.allclose(prof["mean"], prof["dmin"])
    assert np.allclose(prof["area"], math.pi * (prof["equivalent"] / 2) ** 2) and np.allclose(prof["arc"], np.arange(60) * 0.25)
    got = lumen_stenosis(prof, margin=5, reference=10, gap=5)
    assert got["index"] == 30 and abs(got["percent_diameter"] - 50.0) < 0.1 and abs(got["percent_area"] - 75.0) < 0.1
    assert abs(got["reference_diameter"] - 2.0 * poly) < 2e-3 and abs(got["diameter"] - 1.0 * poly) < 2e-3
    assert list(got["proximal"]) == [i for i in range(15, 25) if i != 20] and list(got["distal"]) == list(range(36, 46))
    # a tree off the device: tensors, and oversample / arc given by hand
    import torch
    bare = {k: torch.from_numpy(np.ascontiguousarray(tree[k])) for k in ("radii", "cross", "sections", "centres")}
    again = lumen_profile(bare, pixel_mm=0.5, oversample=2, arc=tree["arc"])
    assert all(np.array_equal(again[k], prof[k]) for k in prof)
    with pytest.raises(ValueError, match="oversample"):
        lumen_profile(bare)


def test_stenosis_refuses_an_empty_window():
    from cta_gan_amd.infer import lumen_profile, lumen_stenosis
    d = np.full(40, 4.0)
    d[20] = 2.0
    with pytest.raises(ValueError, match="proximal"):
        lumen_stenosis(lumen_profile(synthetic(d, bad=range(5, 15))), margin=5, reference=10, gap=5)
    with pytest.raises(ValueError, match="distal"):
        lumen_stenosis(lumen_profile(synthetic(d, bad=range(26, 40))), margin=5, reference=10, gap=5)
    with pytest.raises(ValueError, match="no valid section"):
        lumen_stenosis(lumen_profile(synthetic(d, bad=range(40))))
    d[:] = 4.0
    d[3] = 2.0      # the narrowest valid section inside the margin 3 has no proximal window beyond the gap
    with pytest.raises(ValueError, match="proximal"):
        lumen_stenosis(lumen_profile(synthetic(d)), margin=3, reference=10, gap=5)
    for bad in ({"margin": -1}, {"reference": 0}, {"gap": 1.5}):
        with pytest.raises(ValueError):
            lumen_stenosis(lumen_profile(synthetic(d)), **bad)


# ---------------------------------------------------------------------------------------------- 4. the command line
def test_predict_options():
    import predict
    base = ["--weights", "w", "--input", "i", "--output", "o"]
    line = ["--cl-start", "3,24,34", "--cl-end", "36,24,10", "--cl-threshold", "300"]
    assert "lumen" not in predict.parse_args(base + line).cl
    o = predict.parse_args(base + line + ["--lumen-output", "lumen.npz"])
    assert o.cl["lumen"] == {"rays": 32, "reach": 16.0, "oversample": 2, "edge": "band", "base": None, "recentre": 2} and o.pixel_mm == 1.0
    o = predict.parse_args(base + line + ["--lumen-output", "l.npz", "--lumen-rays", "64", "--lumen-reach", "10.5", "--lumen-oversample", "4",
                                          "--lumen-edge", "half", "--lumen-base=-100", "--lumen-recentre", "0", "--pixel-mm", "0.4"])
    assert o.cl["lumen"] == {"rays": 64, "reach": 10.5, "oversample": 4, "edge": "half", "base": -100, "recentre": 0} and o.pixel_mm == 0.4
    from cta_gan_amd.infer import CENTRELINE_OPTIONS, LUMEN_OPTIONS
    assert "lumen" in CENTRELINE_OPTIONS and set(o.cl["lumen"]) <= set(LUMEN_OPTIONS)
    for bad in (["--lumen-output", "l.npz"], line + ["--lumen-output", "l.npz", "--lumen-rays", "12"],
                line + ["--lumen-output", "l.npz", "--lumen-reach", "200"], line + ["--lumen-output", "l.npz", "--lumen-reach", "0"],
                line + ["--lumen-output", "l.npz", "--lumen-edge", "half"], line + ["--lumen-output", "l.npz", "--lumen-base", "0"],
                line + ["--lumen-output", "l.npz", "--lumen-edge", "half", "--lumen-base", "301"],
                line + ["--lumen-output", "l.npz", "--lumen-recentre", "5"], line + ["--lumen-output", "l.npz", "--pixel-mm", "0"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
    for flag in ("--lumen-output lumen.npz", "--lumen-rays", "--lumen-reach", "--lumen-oversample", "--lumen-edge", "--lumen-base",
                 "--lumen-recentre", "--pixel-mm"):
        assert flag in predict.__doc__ and flag in open(os.path.join(ROOT, "README.md")).read(), flag
