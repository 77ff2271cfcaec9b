"""GPU: the lumen sections of the resident volume (csrc/lumen.hip through ops.lumen_sections, cta_gan_amd/infer.py: VolumeLumen,
lumen_volume, VolumeCentreline(lumen=...), SeriesTranslator(centreline={..., "lumen": ...})) against the numpy restatement
tests/lumen_np.py.  Exact integer arithmetic: every comparison is np.array_equal, never a tolerance."""
import functools
import math

import numpy as np
import pytest
import torch

import components_np as cnp
import lumen_np

SHAPE = (12, 24, 40)      # (n, h, w): nothing larger is needed

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


def same(got, want):
    assert len(got) == len(want) == 4
    for g, w, dtype in zip(got, want, (np.int32, np.int64, np.int32, np.int32)):
        g = cpu(g) if torch.is_tensor(g) else g
        assert g.dtype == dtype and g.shape == w.shape and np.array_equal(g, w)


# ---------------------------------------------------------------------------------------------- 1. noise and blobs, oblique frames
BLOBS = ((5.5, 7.0, 27.0), (6.0, 17.0, 33.0), (4.5, 12.0, 22.5))      # (z, y, x) of the cores


@functools.lru_cache(maxsize=None)
def mixed_volume():
    """int16 noise in -1100 .. 3000 on the low-x half; on the other half smooth blobs (1400 at the core, falling 600 per voxel,
    small enough to close inside the 12 slices at any angle) over -1000, so that walks of many steps, closed sections and recentring
    all happen."""
    n, h, w = SHAPE
    rs = np.random.RandomState(11)
    vol = rs.randint(-1100, 3001, size=SHAPE).astype(np.int64)
    z, y, x = np.mgrid[0:n, 0:h, 0:w]
    smooth = np.full(SHAPE, -1000, dtype=np.int64)
    for (cz, cy, cx), rad in zip(BLOBS, (1.5, 2.0, 1.0)):
        d = np.sqrt((z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2)
        smooth = np.maximum(smooth, np.clip(1400 - 600 * (d - rad), -1000, 1400).astype(np.int64))
    vol = np.where(x >= 18, smooth, vol).astype(np.int16)
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def oblique_table(sections, rays, steps, seed):
    """Random oblique frames: centres all over the volume and a little beyond it (negative coordinates included), every third one
    within a voxel or two of a blob's core; steps sized so that the longest ray is about 12 voxels whatever T is."""
    from cta_gan_amd.infer import _table
    n, h, w = SHAPE
    rs = np.random.RandomState(seed)
    centre = np.stack([rs.uniform(-3.0, w + 2.0, sections), rs.uniform(-3.0, h + 2.0, sections), rs.uniform(-2.0, n + 1.0, sections)], axis=1)
    for r in range(0, sections, 3):
        bz, by, bx = BLOBS[(r // 3) % len(BLOBS)]
        centre[r] = np.array([bx, by, bz]) + rs.uniform(-1.2, 1.2, 3)
    a = rs.normal(size=(sections, 3))
    a /= np.sqrt((a ** 2).sum(axis=1))[:, None]
    b = np.cross(a, rs.normal(size=(sections, 3)))
    b /= np.sqrt((b ** 2).sum(axis=1))[:, None]
    e2 = np.cross(a, b)      # (b, e2): an orthonormal frame across the random direction a
    per = max(1.0, (steps - 1) / 12.0)
    table = np.empty((sections, rays, 9), dtype=np.int64)
    for j in range(rays):
        phi = 2.0 * math.pi * j / rays
        table[:, j] = _table(centre, np.zeros_like(centre), math.cos(phi) * b + math.sin(phi) * e2, per, 1.0)
    table.setflags(write=False)
    return table


CASES = [  # R, K, T, sampling, edge, recentre, (lo, hi)
    (1, 8, 2, "nearest", "band", 0, (200, 2500)),
    (5, 16, 3, "trilinear", "half", 1, (200, 2500)),
    (67, 32, 37, "trilinear", "band", 4, (200, 32767)),
    (67, 64, 37, "nearest", "half", 1, (200, 2500)),
    (5, 64, 256, "trilinear", "band", 4, (-500, 1399)),
    (67, 8, 256, "nearest", "band", 0, (-32768, 32767)),
    (5, 32, 37, "nearest", "half", 4, (0, 32767)),
    (1, 16, 37, "trilinear", "half", 0, (200, 32767)),
    (67, 16, 3, "nearest", "band", 1, (-1100, 3000)),
    (5, 8, 37, "trilinear", "half", 4, (200, 32767)),
    (67, 32, 2, "trilinear", "band", 1, (200, 2500)),
    (1, 64, 256, "nearest", "half", 1, (200, 32767)),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "R%d-K%d-T%d-%s-%s-rc%d" % c[:6])
def test_sections_equal_the_restatement(ops, case):
    sections, rays, steps, sampling, edge, recentre, (lo, hi) = case
    vol = mixed_volume()
    table = oblique_table(sections, rays, steps, seed=sections + rays + steps)
    base = -1000 if edge == "half" else None
    want = lumen_np.sections(vol, table, steps, lo, hi, sampling, edge, base, recentre)
    got = ops.lumen_sections(torch.from_numpy(np.array(vol)).cuda(), np.array(table), rays, steps, lo, hi, sampling=sampling, edge=edge,
                             base=base, recentre=recentre)
    same(got, want)
    if sections == 67:      # the random frames do meet what they were made for
        sec = want[2]
        assert (sec[:, 6] == 1).any() and (sec[:, 6] == 0).any() and (table[:, 0, 0::3] < 0).any()
        if steps >= 37:
            assert (sec[:, 5] > 0).any() and (want[0] > 512).any()
    if case[:3] == (67, 32, 37):
        assert ((sec[:, 5] == 0) & (sec[:, 6] == 0)).any() and (want[3] != table[:, 0, 0::3]).any()      # closed sections: centres moved


def test_a_line_table_made_once_serves_many_calls(ops):
    vol = torch.from_numpy(np.array(mixed_volume())).cuda()
    host = oblique_table(5, 16, 37, seed=1)
    table = ops.LineTable(np.array(host), 16, 37)
    for sampling in ("nearest", "trilinear"):
        same(ops.lumen_sections(vol, table, 16, 37, 200, sampling=sampling, recentre=2),
             lumen_np.sections(mixed_volume(), host, 37, 200, 32767, sampling, "band", None, 2))
    with pytest.raises(RuntimeError, match="checked for"):
        ops.lumen_sections(vol, table, 16, 36, 200)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.lumen_sections(vol.cpu(), table, 16, 37, 200)
    with pytest.raises(RuntimeError, match=r"\[R, 8, 9\]"):
        ops.lumen_sections(vol, np.array(host).reshape(10, 8, 9)[:, None], 8, 37, 200)


# ---------------------------------------------------------------------------------------------- 2. every branch, by construction
LO, HI, T_BR = 500, 2000, 9


@functools.lru_cache(maxsize=None)
def branch_volume():
    n, h, w = SHAPE
    vol = np.zeros(SHAPE, dtype=np.int16)
    vol[:, :, 20:] = 1000            # a wide region in the band, up to the faces x = w-1, y = 0, y = h-1, z = 0, z = n-1
    vol[:, :, 0:4] = 1000            # and one up to the face x = 0
    vol[2:10, 6:15, 6:15] = 1000     # a closed box: walls 4 voxels from (10, 10)
    vol[5, 12, 30] = LO              # prev == lo_r ...
    vol[5, 12, 31] = LO - 1          # ... and v == lo_r - 1 next to it: fraction 0
    vol[5, 16, 27] = LO - 1          # v == lo_r - 1 after prev = 1000: fraction 255
    vol[5, 4, 26] = HI               # prev == hi ...
    vol[5, 4, 27] = HI + 500         # ... and a crossing of hi next to it: fraction 0
    vol[5, 20, 33] = HI + 1          # a crossing of hi after prev = 1000
    vol[6, 8, 8] = LO - 400          # a centre outside the band
    vol.setflags(write=False)
    return vol


# (x, y, z) of the centre, frame: "xy" (ray 0 = +x, ray K/4 = +y) or "zx" (ray 0 = +z, ray K/4 = +x)
BRANCH_SECTIONS = [((30.0, 12.0, 5.0), "xy"),      # 0: prev == lo_r along +x
                   ((26.0, 16.0, 5.0), "xy"),      # 1: v == lo_r - 1 along +x
                   ((26.0, 4.0, 5.0), "xy"),       # 2: prev == hi along +x
                   ((31.0, 20.0, 5.0), "xy"),      # 3: a crossing of hi two steps out along +x
                   ((8.0, 8.0, 6.0), "xy"),        # 4: the centre outside the band
                   ((-3.0, 5.0, 5.0), "xy"),       # 5: the centre outside the volume, at a negative coordinate
                   ((45.0, 30.0, 14.0), "xy"),     # 6: outside beyond the far corner
                   ((37.0, 12.0, 8.0), "xy"),      # 7: leaves through x = w-1
                   ((1.0, 12.0, 8.0), "xy"),       # 8: leaves through x = 0 (negative coordinates along the ray)
                   ((29.0, 2.0, 8.0), "xy"),       # 9: leaves through y = 0
                   ((29.0, 21.0, 8.0), "xy"),      # 10: leaves through y = h-1
                   ((30.0, 10.0, 1.0), "zx"),      # 11: leaves through z = 0
                   ((30.0, 10.0, 10.0), "zx"),     # 12: leaves through z = n-1
                   ((29.0, 11.0, 9.0), "xy"),      # 13: never stops: every ray open at 256 (T-1)
                   ((10.0, 10.0, 5.0), "xy"),      # 14: the closed box from its middle
                   ((11.0, 9.0, 5.0), "xy"),       # 15: the closed box from off its middle: recentring moves it
                   ((12.0, 10.0, 5.0), "zx")]      # 16: the closed box in a plane that holds z


def branch_table(rays):
    from cta_gan_amd.infer import _table
    frames = {"xy": (np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])), "zx": (np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))}
    centre = np.array([c for c, _ in BRANCH_SECTIONS])
    e1 = np.array([frames[f][0] for _, f in BRANCH_SECTIONS])
    e2 = np.array([frames[f][1] for _, f in BRANCH_SECTIONS])
    table = np.empty((len(centre), rays, 9), dtype=np.int64)
    for j in range(rays):
        phi = 2.0 * math.pi * j / rays
        table[:, j] = _table(centre, np.zeros_like(centre), math.cos(phi) * e1 + math.sin(phi) * e2, 1, 1.0)
    return table


def test_the_restatement_takes_every_branch():
    """(CPU work, kept here beside the table it reads: what the GPU is compared with below does go through each branch.)"""
    table = branch_table(8)
    radii, cross, sec, centres = lumen_np.sections(branch_volume(), table, T_BR, LO, HI, "nearest", "band", None, 0)
    assert radii[0, 0] == 0 and radii[1, 0] == 256 * 0 + (500 * 256) // 501 + 0 and radii[1, 0] == 255
    assert radii[2, 0] == 0 and radii[3, 0] == 256 + (1000 * 256) // 1001
    assert sec[4].tolist() == [0, 0, 0, 0, 0, 0, 1, LO] and sec[5, 6] == 1 and sec[6, 6] == 1 and not radii[4:7].any() and not cross[4:7].any()
    assert table[5, 0, 0] < 0
    assert radii[7, 0] == 2 * 256 and radii[8, 4] == 256 and radii[9, 6] == 2 * 256 and radii[10, 2] == 2 * 256      # (k-1) 256 at the face
    assert radii[11, 4] == 256 and radii[12, 0] == 256 and (sec[7:13, 5] >= 1).all() and (sec[7:13, 6] == 0).all()
    assert (radii[13] == 256 * (T_BR - 1)).all() and sec[13, 5] == 8 and sec[13, 0] == 8 * 256 * (T_BR - 1)
    assert sec[14, 5] == 0 and radii[14, 0] == 4 * 256 + 128 and sec[14, 1] == 9 * 256 and sec[14, 3:5].tolist() == [0, 1]
    moved = lumen_np.sections(branch_volume(), table, T_BR, LO, HI, "nearest", "band", None, 2)[3]
    assert np.array_equal(moved[:14], table[:14, 0, 0::3])      # outside or open: the centre stays where it was put
    assert np.abs(moved[15, :2] - table[14, 0, 0:6:3]).max() < 6554 and moved[15, 2] == table[15, 0, 6]      # in its plane, to within 0.1 px of the middle
    assert np.abs(table[15, 0, 0:6:3] - table[14, 0, 0:6:3]).min() == 65536
    assert moved[16, 1] == table[16, 0, 3] and moved[16, 0] != table[16, 0, 0]


@pytest.mark.parametrize("rays", (8, 32))
@pytest.mark.parametrize("sampling", ("nearest", "trilinear"))
def test_every_branch_equals_the_restatement(ops, rays, sampling):
    vol, table = branch_volume(), branch_table(rays)
    dev = torch.from_numpy(np.array(vol)).cuda()
    line = ops.LineTable(table, rays, T_BR)
    for edge, base in (("band", None), ("half", 0), ("half", LO)):
        for recentre in (0, 2):
            same(ops.lumen_sections(dev, line, rays, T_BR, LO, HI, sampling=sampling, edge=edge, base=base, recentre=recentre),
                 lumen_np.sections(vol, table, T_BR, LO, HI, sampling, edge, base, recentre))


# ---------------------------------------------------------------------------------------------- 3. ABI refusals
def test_abi_refusals_launch_nothing(ops):
    from cta_gan_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, h, w = SHAPE
    vol = torch.from_numpy(np.array(mixed_volume())).cuda()
    host = oblique_table(5, 8, 3, seed=2)
    lines = torch.from_numpy(host.astype(np.int32).reshape(-1, 9)).cuda()
    i32 = lambda count: torch.full((count,), 777, dtype=torch.int32, device="cuda")
    radii, cross, sections, centres = i32(5 * 8 + 2), torch.full((5 + 1,), 777, dtype=torch.int64, device="cuda"), i32(5 * 8 + 2), i32(5 * 3 + 2)
    P = dict(vol=vol.data_ptr(), lines=lines.data_ptr(), radii=radii.data_ptr(), cross=cross.data_ptr(), sections=sections.data_ptr(),
             centres=centres.data_ptr())

    def go(vol=P["vol"], N=n, H=h, W=w, lines=P["lines"], R=5, K=8, T=3, lo=200, hi=2500, sampling=1, edge=0, base=0, recentre=0,
           radii=P["radii"], cross=P["cross"], sections=P["sections"], centres=P["centres"]):
        return lib.ctg_lumen_sections(vol, N, H, W, lines, R, K, T, lo, hi, sampling, edge, base, recentre, radii, cross, sections, centres, st)

    bad = [go(vol=None), go(lines=None), go(radii=None), go(cross=None), go(sections=None), go(centres=None), go(N=0), go(H=4097), go(W=0),
           go(R=0), go(R=2 ** 28, K=8), go(K=0), go(K=4), go(K=12), go(K=128), go(T=1), go(T=257), go(lo=5, hi=4), go(lo=-32769), go(hi=32768),
           go(sampling=2), go(sampling=-1), go(edge=2), go(edge=-1), go(edge=1, base=201), go(edge=1, base=-32769), go(recentre=-1),
           go(recentre=5), go(vol=P["vol"] + 1), go(lines=P["lines"] + 2), go(radii=P["radii"] + 2), go(cross=P["cross"] + 4),
           go(sections=P["sections"] + 1), go(centres=P["centres"] + 2)]
    assert bad == [1] * len(bad), bad      # CTG_EINVAL
    torch.cuda.synchronize()
    for t in (radii, cross, sections, centres):
        assert int((t != 777).sum()) == 0      # nothing was launched
    # the same call with everything in order succeeds, and writes only what is its own
    assert go() == 0
    torch.cuda.synchronize()
    want = lumen_np.sections(mixed_volume(), host, 3, 200, 2500, "trilinear", "band", None, 0)
    same((radii[:40].reshape(5, 8), cross[:5], sections[:40].reshape(5, 8), centres[:15].reshape(5, 3)), want)
    assert cpu(radii[40:]).tolist() == [777, 777] and int(cross[5]) == 777 and cpu(sections[40:]).tolist() == [777, 777]
    assert cpu(centres[15:]).tolist() == [777, 777]
    radii.fill_(777), centres.fill_(777)
    assert go(edge=1, base=200, radii=P["radii"] + 4, centres=P["centres"] + 4) == 0      # (any 4-byte boundary will do)
    torch.cuda.synchronize()
    half = lumen_np.sections(mixed_volume(), host, 3, 200, 2500, "trilinear", "half", 200, 0)
    same((radii[1:41].reshape(5, 8), cross[:5], sections[:40].reshape(5, 8), centres[1:16].reshape(5, 3)), half)
    assert int(radii[0]) == 777 and int(radii[41]) == 777 and int(centres[0]) == 777 and int(centres[16]) == 777 and int(cross[5]) == 777


# ---------------------------------------------------------------------------------------------- 4. through the layers
TRUE = (20.6, 11.3)      # (x, y) of the tube's axis


@functools.lru_cache(maxsize=None)
def tube():
    n, h, w = SHAPE
    y, x = np.mgrid[0:h, 0:w]
    plane = np.where((x - TRUE[0]) ** 2 + (y - TRUE[1]) ** 2 <= 3.5 ** 2, 1000, 0).astype(np.int16)
    vol = np.repeat(plane[None], n, axis=0)
    vol.setflags(write=False)
    return vol


def tree_equals(tree, lines, want):
    same([tree[k] for k in ("radii", "cross", "sections", "centres")], want)
    arc, s = tree["arc"], tree["oversample"]
    arc, s = (cpu(arc), cpu(s)) if torch.is_tensor(arc) else (arc, s)
    assert arc.dtype == np.float64 and np.array_equal(arc, lines.arc) and s.tolist() == [lines.oversample]
    assert sorted(tree) == ["arc", "centres", "cross", "oversample", "radii", "sections"]


def test_volume_lumen_chunks_source_and_twin(ops):
    from cta_gan_amd.infer import ResidentVolume, VolumeLumen, lumen_lines, lumen_profile, lumen_volume
    vol = tube()
    n, h, w = SHAPE
    pts = [[0.0, 12.0, 22.0], [n - 1.0, 11.0, 20.0]]      # a click-like line: off the axis, and a little oblique
    opts = dict(rays=32, reach=8.0, oversample=2, recentre=2)
    lines = lumen_lines(n, h, w, pts, rays=32, reach=8.0, oversample=2)
    want = lumen_np.sections(vol, lines[0], lines.steps, 500, 32767, "trilinear", "band", None, 2)
    view = VolumeLumen(n, h, w, 500, pts, **opts)
    assert view.nbytes == 2 * n * h * w + 4 * lines[0].size + len(lines.arc) * (4 * 32 + 60) + 4
    dev = torch.from_numpy(np.array(vol)).cuda()
    order = np.random.RandomState(5).permutation(n)
    for z in order[:-1]:
        view.update(dev[z:z + 1], int(z))
    with pytest.raises(RuntimeError, match="exactly once"):
        view.result()
    view.update(dev[order[-1]:order[-1] + 1], int(order[-1]))
    for _ in range(2):
        out = view.result()
        assert all(t.is_cuda for t in out.values())
        tree_equals(out, lines, want)
    # what it measures: the tube's 7 px, from a line that is up to 1.6 px off its axis; the tilted sections at the two ends reach
    # out of the volume, which leaves rays open: not valid
    prof = lumen_profile(out)
    assert prof["valid"].tolist() == [False] + [True] * (n - 2) + [False] and np.abs(prof["equivalent"][1:-1] - 7.0).max() <= 0.25
    c = cpu(out["centres"])[1:-1, :2] / 65536.0 - 0.5
    assert np.hypot(c[:, 0] - TRUE[0], c[:, 1] - TRUE[1]).max() <= 0.25
    # source=: the view reads a shared resident volume and holds none of its own
    shared = ResidentVolume(n, h, w)
    half = VolumeLumen(n, h, w, (100, 32767), pts, edge="half", base=0, sampling="nearest", source=shared, **opts)
    assert half.nbytes == view.nbytes - 2 * n * h * w and half.volume is None
    with pytest.raises(RuntimeError, match="through its source"):
        half.update(dev, 0)
    shared.update(dev, 0)
    assert half.volume is shared.volume
    tree_equals(half.result(), lines, lumen_np.sections(vol, lines[0], lines.steps, 100, 32767, "nearest", "half", 0, 2))
    # the twin: a host volume in chunks comes back as numpy, a device volume stays where it is
    host = lumen_volume(np.array(vol), 500, pts, batch=5, **opts)
    assert all(isinstance(v, np.ndarray) for v in host.values())
    tree_equals(host, lines, want)
    there = lumen_volume(dev, 500, pts, **opts)
    assert there["radii"].is_cuda
    tree_equals(there, lines, want)


def test_centreline_volume_with_and_without_lumen(ops):
    from cta_gan_amd.infer import centreline_volume, lumen_lines, lumen_profile
    vol = np.array(tube())
    n, h, w = SHAPE
    start, ends = (0, 11, 21), [(n - 1, 11, 21), (6, 12, 20)]
    plain = centreline_volume(vol, 500, start, ends, radius=4)
    assert "lumen" not in plain and sorted(plain) == ["clearance", "counts", "paths", "points", "stats"]
    lumen = dict(rays=16, reach=8.0, recentre=1, edge="half", base=0, threshold=(100, 32767))
    out = centreline_volume(vol, 500, start, ends, radius=4, lumen=lumen)
    assert sorted(out) == sorted(list(plain) + ["lumen"]) and len(out["lumen"]) == 2
    for k in ("paths", "counts", "stats"):
        assert np.array_equal(out[k], plain[k])
    for e in range(2):
        assert np.array_equal(out["points"][e], plain["points"][e])
        lines = lumen_lines(n, h, w, out["points"][e], rays=16, reach=8.0)
        tree_equals(out["lumen"][e], lines, lumen_np.sections(vol, lines[0], lines.steps, 100, 32767, "trilinear", "half", 0, 1))
    assert lumen_profile(out["lumen"][0])["valid"][2:-2].all()      # (away from the two faces the line ends on, every wall is found)
    # without a threshold of its own the lumen takes the centreline's band; beside cpr both are there
    both = centreline_volume(torch.from_numpy(vol).cuda(), (500, 1200), start, ends[:1], radius=4, cpr=dict(cols=9), lumen=dict(rays=8, reach=6.0))
    lines = lumen_lines(n, h, w, cpu(both["points"][0]), rays=8, reach=6.0)
    assert both["lumen"][0]["radii"].is_cuda and len(both["cpr"]) == 1
    tree_equals(both["lumen"][0], lines, lumen_np.sections(vol, lines[0], lines.steps, 500, 1200, "trilinear", "band", None, 0))
    for bad in (dict(rays=12), dict(cols=9), dict(edge="half"), dict(recentre=9), 32):
        with pytest.raises(ValueError):
            centreline_volume(vol, 500, start, ends, lumen=bad)


def make_generator(seed=0):
    from cta_gan_amd import synth
    from cta_gan_amd.Model.HdGan import Generator
    return synth.fill_module(Generator(1, 1), seed=seed).cuda()


def test_series_translator_returns_the_tree_of_the_view_alone(ops):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator, centreline_volume
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        g = make_generator()
        vol = np.random.RandomState(7).randint(-1100, 3200, size=(7, 64, 64)).astype(np.int16)
        base = SeriesTranslator(g, batch=2)(vol)
        pix = base["pix"]
        n, h, w = pix.shape
        lo, r = int(np.percentile(pix, 50)), 3
        lab = cnp.label(np.where(pix >= lo, 1500, 0).astype(np.int16), cnp.LO, cnp.HI, 26).reshape(-1)
        roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
        members = np.flatnonzero(lab == roots[np.argmax(sizes)])
        assert members.size > 100
        zyx = lambda i: (int(i // (h * w)), int((i // w) % h), int(i % w))
        options = dict(threshold=lo, start=zyx(members[0]), ends=[zyx(members[-1]), zyx(members[members.size // 2])], radius=r,
                       lumen=dict(rays=16, reach=6.0, recentre=2))
        off = SeriesTranslator(g, batch=2, centreline={k: v for k, v in options.items() if k != "lumen"})(vol)
        assert "lumen" not in off["centreline"]
        alone = centreline_volume(pix, **{k: v for k, v in options.items() if k not in ("threshold", "start", "ends")},
                                  threshold=lo, start=options["start"], ends=options["ends"])
        tr = SeriesTranslator(g, batch=2, centreline=options)
        for _ in range(2):      # (a second call on the same object)
            o = tr(vol)
            assert np.array_equal(o["pix"], pix)
            cl = o["centreline"]
            assert sorted(cl) == sorted(alone) and len(cl["lumen"]) == 2
            for k in ("paths", "counts", "stats"):
                assert np.array_equal(cl[k], alone[k]) and np.array_equal(cl[k], off["centreline"][k])
            for e in range(2):
                assert np.array_equal(cl["points"][e], alone["points"][e])
                assert sorted(cl["lumen"][e]) == sorted(alone["lumen"][e])
                for k, v in alone["lumen"][e].items():
                    assert cl["lumen"][e][k].dtype == v.dtype and np.array_equal(cl["lumen"][e][k], v), k
    finally:
        nets.set_default_compute_dtype(torch.float32)
