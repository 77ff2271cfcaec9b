"""GPU: the depth of the maximum (ctg_project_rotate_depth, ctg_project_accumulate_depth, ctg_project_finish_depth through
ops.project_rotate_depth / project_accumulate_depth / project_finish_depth; cta_gan_amd/infer.py: SeriesRotator / SeriesProjector /
rotate_volume / project_volume / SeriesTranslator with depth=True, ray_voxel; predict.py --depth) against the numpy restatement
tests/depth_np.py, which uses no packed key.  Exact integer arithmetic: every comparison is np.array_equal, never a tolerance."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_np
import project_np
import rotate_lerp_np
import rotate_np
from test_rotate_gpu import ANGLES, SHAPES, make_generator, planted, synthetic_hu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["max", "min"]
CUES = [0, 97, 256]
PLANES = ("values", "level", "depth", "cued")
DTYPES = {"values": torch.int16, "level": torch.uint8, "depth": torch.int16, "cued": torch.uint8}
SENTINEL = {"values": 12345, "level": 77, "depth": -321, "cued": 99}
WC, WW = 300.0, 40000.0      # a window wide enough that the levels of random int16 values differ

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


def table(h, w, u, t, s=1, angles=ANGLES):
    return np.array([rotate_lerp_np.coefficients(a, h, w, u, t, s) for a in angles], dtype=np.int64)


def sentinels(a, n, u, which=PLANES):
    return {p: torch.full((a, n, u), SENTINEL[p], dtype=DTYPES[p], device="cuda") if p in which else None for p in PLANES}


def run(ops, dev, n0, coef, n, u, steps, mode, cue=0, out=None, which=PLANES, **kw):
    """One ops.project_rotate_depth call into fresh (or the given) planes -> {plane: numpy or None}."""
    if out is None:
        out = sentinels(len(coef.host) if hasattr(coef, "host") else len(coef), n, u, which)
    ops.project_rotate_depth(dev, n0, coef, steps, mode, cue=cue, wc=WC, ww=WW, **out, **kw)
    return {p: None if t is None else cpu(t) for p, t in out.items()}


# ---------------------------------------------------------------------------------------------- 1. one call equals numpy
@pytest.mark.parametrize("oversample", [1, 2])
@pytest.mark.parametrize("sampling", ["nearest", "bilinear"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_project_rotate_depth_equals_numpy(ops, shape, sampling, oversample):
    n, h, w = shape
    vol = planted(n, h, w, seed=n * 1000 + w)
    dev = torch.from_numpy(vol).cuda()
    d = rotate_np.detector(h, w)
    for u, t in ((d, d), (w, h)):      # the default detector, and the slice's own width and height
        steps = t * oversample
        coef = table(h, w, u, t, oversample)
        tab = ops.RotateTable(coef)
        ref = depth_np.rotate_depth_modes(vol, coef, u, steps, MODES, sampling, fill=0)
        for mode in MODES:
            values, depth = ref[mode]
            level = rotate_np.level(values, WC, WW)
            assert (depth == -1).any() == (rotate_np.count(h, w, coef, u, steps) == 0).any()
            plain = (torch.empty((len(coef), n, u), dtype=torch.int16, device="cuda"),
                     torch.empty((len(coef), n, u), dtype=torch.uint8, device="cuda"))
            ops.project_rotate(dev, 0, tab, steps, mode, values=plain[0], level=plain[1], wc=WC, ww=WW, sampling=sampling)
            for cue in CUES:
                got = run(ops, dev, 0, tab, n, u, steps, mode, cue=cue, sampling=sampling)
                assert np.array_equal(got["values"], values), (u, t, mode, cue)
                assert np.array_equal(got["depth"], depth), (u, t, mode, cue)
                assert np.array_equal(got["level"], level), (u, t, mode, cue)
                assert np.array_equal(got["cued"], depth_np.cued(level, cue, depth, steps)), (u, t, mode, cue)
                assert np.array_equal(got["values"], cpu(plain[0])) and np.array_equal(got["level"], cpu(plain[1]))
                if cue == 0:
                    assert np.array_equal(got["cued"], got["level"])


# ---------------------------------------------------------------------------------------------- 2. ties
PAIRS = [((3, 4), 5), ((3, 11), 20), ((3, 36), 40)]      # (rows, column): other lanes of the ray; the lane's next in-flight slot; the next trip


@pytest.mark.parametrize("sampling", ["nearest", "bilinear"])
def test_equal_extremes_the_nearer_one_wins(ops, sampling):
    """U = W, T = H: at 0 degrees sample (u, t) is pixel (u, t), at 180 degrees pixel (W-1-u, H-1-t): the far one becomes the near
    one.  Slice 0 carries doubled maxima, slice 1 doubled minima."""
    n, h, w = 2, 37, 53
    vol = np.random.RandomState(11).randint(-1000, 1000, size=(n, h, w)).astype(np.int16)
    for (r0, r1), c in PAIRS:
        vol[0, r0, c] = vol[0, r1, c] = 30000
        vol[1, r0, c] = vol[1, r1, c] = -30000
    coef = table(h, w, w, h, angles=[0, 180])
    assert coef[0].tolist() == [32768, 65536, 0, 32768, 0, 65536] and coef[1, 1] == -65536 and coef[1, 5] == -65536
    dev = torch.from_numpy(vol).cuda()
    for i, mode in enumerate(MODES):
        got = run(ops, dev, 0, coef, n, w, h, mode, cue=256, sampling=sampling)
        values, depth = depth_np.rotate_depth(vol, coef, w, h, mode, sampling)
        assert np.array_equal(got["values"], values) and np.array_equal(got["depth"], depth)
        for (r0, r1), c in PAIRS:
            assert got["values"][0, i, c] == got["values"][1, i, w - 1 - c] == (30000 if mode == "max" else -30000)
            assert got["depth"][0, i, c] == r0 and got["depth"][1, i, w - 1 - c] == h - 1 - r1, (mode, r0, r1)


def test_a_constant_volume_has_the_first_counted_step(ops):
    n, h, w = 2, 33, 31
    d = rotate_np.detector(h, w)
    vol = np.full((n, h, w), -5, dtype=np.int16)
    dev = torch.from_numpy(vol).cuda()
    for s in (1, 2):
        coef = table(h, w, d, d, s)
        ok = np.stack([rotate_np._samples(h, w, c, d, d * s)[2] for c in coef])      # [A][U][T]
        first = np.where(ok.any(axis=2), ok.argmax(axis=2), -1)
        assert (first == -1).any() and (first > 0).any()
        for mode, sampling in itertools.product(MODES, ("nearest", "bilinear")):
            got = run(ops, dev, 0, coef, n, d, d * s, mode, sampling=sampling, fill=9)
            assert np.array_equal(got["depth"], np.broadcast_to(first[:, None, :], got["depth"].shape)), (s, mode, sampling)
            assert np.array_equal(got["values"], np.where(got["depth"] < 0, 9, -5))


# ---------------------------------------------------------------------------------------------- 3. picking
def test_a_pixel_and_its_depth_lead_back_to_the_voxel(ops):
    from cta_gan_amd.infer import ray_voxel
    n, h, w = 3, 33, 31
    rng = np.random.RandomState(4)
    vol = np.stack([rng.permutation(h * w).reshape(h, w) - 500 for _ in range(n)]).astype(np.int16)
    d = rotate_np.detector(h, w)
    coef = table(h, w, d, d)
    dev = torch.from_numpy(vol).cuda()
    for mode in MODES:
        got = run(ops, dev, 0, coef, n, d, d, mode)
        for a in range(len(coef)):
            hit = got["depth"][a] >= 0      # [n][U]
            assert hit.any() and np.array_equal(hit, np.broadcast_to(rotate_np.count(h, w, coef[a:a + 1], d, d)[0] > 0, hit.shape))
            x, y = ray_voxel(coef[a], np.arange(d)[None, :], got["depth"][a])
            rows = np.broadcast_to(np.arange(n)[:, None], hit.shape)
            assert np.array_equal(vol[rows[hit], y[hit], x[hit]], got["values"][a][hit]), (mode, a)


# ---------------------------------------------------------------------------------------------- 4. chunks, views, rows, outputs
@pytest.fixture(scope="module")
def volume7():
    return planted(7, 33, 31, seed=77)


@pytest.mark.parametrize("mode", MODES)
def test_chunks_in_any_order_a_two_byte_aligned_view_and_the_rows_written(ops, volume7, mode):
    n, h, w = volume7.shape
    d = rotate_np.detector(h, w)
    coef = table(h, w, d, d)
    tab = ops.RotateTable(coef)
    dev = torch.from_numpy(volume7).cuda()
    whole = run(ops, dev, 0, tab, n, d, d, mode, cue=97, sampling="bilinear")
    values, depth = depth_np.rotate_depth(volume7, coef, d, d, mode, "bilinear")
    assert np.array_equal(whole["values"], values) and np.array_equal(whole["depth"], depth)
    out = sentinels(len(coef), n, d)
    for s in (4, 0, 6, 2):      # chunks of 2 (the last of 1) in shuffled order: every call writes its own rows
        got = run(ops, dev[s:s + 2], s, tab, n, d, d, mode, cue=97, sampling="bilinear", out=out)
    assert all(np.array_equal(got[p], whole[p]) for p in PLANES)
    buf = torch.empty(n * h * w + 1, dtype=torch.int16, device="cuda")      # one element into a buffer: only 2-byte aligned
    shifted = buf[1:].view(n, h, w)
    shifted.copy_(dev)
    assert shifted.is_contiguous() and shifted.data_ptr() % 4 == 2
    got = run(ops, shifted, 0, tab, n, d, d, mode, cue=97, sampling="bilinear")
    assert all(np.array_equal(got[p], whole[p]) for p in PLANES)
    got = run(ops, dev[2:4], 2, tab, n, d, d, mode, cue=97, sampling="bilinear")      # rows outside n0 .. n0+K-1 keep the sentinel
    for p in PLANES:
        assert np.array_equal(got[p][:, 2:4], whole[p][:, 2:4]) and (got[p][:, :2] == SENTINEL[p]).all() \
            and (got[p][:, 4:] == SENTINEL[p]).all(), p


def test_any_subset_of_the_outputs_and_the_refusals(ops, volume7):
    from cta_gan_amd import _lib
    n, h, w = volume7.shape
    d = rotate_np.detector(h, w)
    tab = ops.RotateTable(table(h, w, d, d, angles=[0, 30]))
    dev = torch.from_numpy(volume7).cuda()
    whole = run(ops, dev, 0, tab, n, d, d, "min", cue=200)
    for r in range(1, 4):
        for which in itertools.combinations(PLANES, r):
            got = run(ops, dev, 0, tab, n, d, d, "min", cue=200, which=which)
            for p in PLANES:
                assert (got[p] is None) if p not in which else np.array_equal(got[p], whole[p]), (which, p)
    out = sentinels(2, n, d)
    for kw in (dict(mode="mean"), dict(mode=2), dict(cue=257), dict(cue=-1), dict(cue=1.5), dict(sampling="cubic"),
               dict(values=None, level=None, depth=None, cued=None), dict(depth=out["depth"].int()), dict(cued=out["cued"][:1]),
               dict(n0=1), dict(pix=dev.cpu())):
        args = dict(pix=dev, n0=0, coef=tab, t=d, mode="max", cue=0, **out)
        args.update(kw)
        with pytest.raises(RuntimeError):
            ops.project_rotate_depth(**args)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    P, C = dev.data_ptr(), tab.dev.data_ptr()
    V, L, D, Q = (out[p].data_ptr() for p in PLANES)

    def call(K=n, T=d, mode=0, sampling=0, cue=0, values=V, level=L, depth=D, cued=Q):
        return lib.ctg_project_rotate_depth(P, K, h, w, 0, n, C, 2, d, T, mode, sampling, 0, cue, 50.0, 400.0, 0, values, level, depth,
                                            cued, st)

    for kw in (dict(values=None, level=None, depth=None, cued=None), dict(mode=2), dict(mode=-1), dict(sampling=2), dict(sampling=-1),
               dict(cue=257), dict(cue=-1), dict(T=4097), dict(K=n + 1), dict(depth=D + 1), dict(values=V + 1)):
        assert call(**kw) == 1, kw      # CTG_EINVAL
    torch.cuda.synchronize()
    assert all((out[p] == SENTINEL[p]).all() for p in PLANES)      # nothing was launched
    assert call() == 0 and call(values=None, level=None, cued=None) == 0
    torch.cuda.synchronize()
    assert not (out["depth"] == SENTINEL["depth"]).any()


# ---------------------------------------------------------------------------------------------- 5. the projector
PROJECTOR_SHAPES = [(3, 5, 7), (7, 33, 31), (4, 19, 515), (2, 9, 1032), (5, 17, 520)]


def check_projection(got, vol, mode, thick, cue, wc=WC, ww=WW, hu=False):
    want = depth_np.project_depth(vol, mode, thick)
    assert sorted(got) == sorted(want)
    for a, (values, depth, start, length) in want.items():
        level = project_np.level(values, wc, ww, hu)
        assert sorted(got[a]) == ["cued", "depth", "level", "values"]
        g = {k: np.asarray(t.cpu() if torch.is_tensor(t) else t) for k, t in got[a].items()}
        assert g["depth"].dtype == np.int16 and g["cued"].dtype == np.uint8
        assert np.array_equal(g["values"], values), (a, mode, thick)
        assert np.array_equal(g["depth"], depth), (a, mode, thick)
        assert np.array_equal(g["level"], level), (a, mode, thick)
        assert np.array_equal(g["cued"], depth_np.cued(level, cue, depth - start, length)), (a, mode, thick, cue)


@pytest.mark.parametrize("shape", PROJECTOR_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_series_projector_depth_equals_numpy(ops, shape):
    from cta_gan_amd.infer import SeriesProjector
    n, h, w = shape
    vol = planted(n, h, w, seed=n * 100 + h)
    vol[:, h // 2, : (w + 1) // 2] = vol[0, h // 2, : (w + 1) // 2]      # ties along the slices
    vol[:, :, w // 3] = vol[:, :1, w // 3]                              # ties along the rows
    vol[:, h - 1, :] = vol[:, h - 1, :1]                                # ties along the columns
    dev = torch.from_numpy(vol).cuda()
    buf = torch.empty(n * h * w + 1, dtype=torch.int16, device="cuda")      # the same slices, only 2-byte aligned
    shifted = buf[1:].view(n, h, w)
    shifted.copy_(dev)
    chunk = 1 if n <= 4 else 3           # more than one chunk for every shape; chunks of 3 straddle the slabs of 2
    starts = list(range(0, n, chunk))
    order = starts[1::2] + starts[0::2]  # never the order of the slices: (1, 0), (1, 0, 2), (1, 3, 0, 2), (3, 0), (3, 0, 6)
    assert len(order) > 1 and order != starts
    for mode in MODES:
        for slab in (None, 2):
            plain = SeriesProjector(n, h, w, mode=mode, slab=slab)
            proj = SeriesProjector(n, h, w, mode=mode, slab=slab, depth=True, cue=CUES[1])
            for src in (dev, shifted):
                proj.reset()
                for s in order:
                    proj.update(src[s:s + chunk], s)
                for cue in CUES:
                    proj.cue = cue
                    check_projection(proj.result(WC, WW), vol, mode, slab, cue)
            out = proj.result(WC, WW, level=False)
            assert all(sorted(d) == ["depth", "level", "values"] and d["level"] is None for d in out.values())
            plain.update(dev, 0)
            base, got = plain.result(WC, WW), proj.result(WC, WW)
            for a in base:
                assert sorted(base[a]) == ["level", "values"]
                assert torch.equal(base[a]["values"], got[a]["values"]) and torch.equal(base[a]["level"], got[a]["level"])


def test_equal_slices_give_the_first_slice_of_every_slab(ops):
    from cta_gan_amd.infer import SeriesProjector, project_volume
    n, h, w = 7, 17, 520
    vol = np.repeat(planted(1, h, w, seed=1), n, axis=0)
    for mode in MODES:
        out = project_volume(vol, mode=mode, slab=3, depth=True, cue=256, batch=2, wc=WC, ww=WW)
        assert isinstance(out["axial"]["depth"], np.ndarray)
        assert np.array_equal(out["axial"]["depth"], np.broadcast_to(np.array([0, 3, 6], dtype=np.int16)[:, None, None], (3, h, w)))
        assert np.array_equal(out["axial"]["cued"], out["axial"]["level"])      # depth 0 inside every slab: w = 256
        check_projection(out, vol, mode, 3, 256)
    assert sorted(project_volume(vol, slab=3, batch=4)["axial"]) == ["level", "values"]
    with pytest.raises(RuntimeError):
        ops.project_accumulate_depth(torch.from_numpy(vol).cuda(), 0, 3, "mean",
                                     axial=torch.zeros((3, h, w), dtype=torch.int32, device="cuda"))
    acc = torch.zeros((3, h, w), dtype=torch.int32, device="cuda")
    for kw in (dict(mode="mean"), dict(cue=300), dict(thick=4, extent=7), dict(extent=40000),
               dict(want_values=False, want_level=False, want_depth=False, want_cued=False)):
        args = dict(acc=acc, mode="max", thick=3, extent=7)
        args.update(kw)
        with pytest.raises(RuntimeError):
            ops.project_finish_depth(**args)
    from cta_gan_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    pix = torch.from_numpy(vol).cuda()
    assert lib.ctg_project_accumulate_depth(pix.data_ptr(), n, h, w, 0, 3, 2, acc.data_ptr(), None, None, st) == 1      # a mean
    assert lib.ctg_project_accumulate_depth(pix.data_ptr(), n, h, w, 32767, 3, 0, acc.data_ptr(), None, None, st) == 1  # past int16
    out = torch.full((3, h, w), -321, dtype=torch.int16, device="cuda")
    assert lib.ctg_project_finish_depth(acc.data_ptr(), 3, h * w, 2, 3, 7, 0, 50.0, 400.0, 0, None, None, out.data_ptr(), None, st) == 1
    assert lib.ctg_project_finish_depth(acc.data_ptr(), 3, h * w, 0, 3, 7, 0, 50.0, 400.0, 0, None, None, None, None, st) == 1
    torch.cuda.synchronize()
    assert (acc == 0).all() and (out == -321).all()      # nothing was launched


# ---------------------------------------------------------------------------------------------- 6. rotator, volumes, translator
def check_rotation(rot, pix, angles, mode, cue, wc, ww, hu, sampling="nearest"):
    n, h, w = pix.shape
    d = rotate_np.detector(h, w)
    values, depth = depth_np.rotate_depth(pix, table(h, w, d, d, 1, angles), d, d, mode, sampling, fill=-1024 if hu else 0)
    level = rotate_np.level(values, wc, ww, hu)
    assert sorted(rot) == ["angles", "cued", "depth", "level", "values"]
    got = {k: np.asarray(t.cpu() if torch.is_tensor(t) else t) for k, t in rot.items()}
    assert got["depth"].dtype == np.int16 and got["cued"].dtype == np.uint8
    assert np.array_equal(got["values"], values) and np.array_equal(got["depth"], depth)
    assert np.array_equal(got["level"], level) and np.array_equal(got["cued"], depth_np.cued(level, cue, depth, d))


def test_series_rotator_and_rotate_volume_with_depth(ops, monkeypatch):
    from cta_gan_amd.infer import SeriesRotator, rotate_volume, view_angles
    vol = planted(5, 19, 23, seed=3)
    n, h, w = vol.shape
    dev = torch.from_numpy(vol).cuda()
    angles = view_angles(4, span=180.0, start=15.0)
    calls = []
    for name in ("project_rotate", "project_rotate_depth"):
        monkeypatch.setattr(ops, name, (lambda f, name: lambda *a, **k: (calls.append(name), f(*a, **k))[1])(getattr(ops, name), name))
    r = SeriesRotator(n, h, w, angles, mode="min", hu=True, wc=WC, ww=WW, depth=True, cue=128, sampling="bilinear")
    r.update(dev[3:], 3)
    r.update(dev[:3], 0)
    assert calls == ["project_rotate_depth"] * 2      # one launch per chunk, the plain entry is not run as well
    check_rotation(r.result(), vol, angles, "min", 128, WC, WW, True, "bilinear")
    out = SeriesRotator(n, h, w, angles, depth=True, level=False).result()
    assert sorted(out) == ["angles", "depth", "level", "values"] and out["level"] is None
    del calls[:]
    plain = SeriesRotator(n, h, w, angles, mode="min", hu=True, wc=WC, ww=WW, sampling="bilinear")
    plain.update(dev, 0)
    assert calls == ["project_rotate"] and sorted(plain.result()) == ["angles", "level", "values"]
    assert plain.depth_plane is None and plain.cued is None
    assert torch.equal(plain.result()["values"], r.result()["values"]) and torch.equal(plain.result()["level"], r.result()["level"])
    got = rotate_volume(vol, angles, mode="max", depth=True, cue=256, batch=2, wc=WC, ww=WW)
    assert isinstance(got["depth"], np.ndarray)
    check_rotation(got, vol, angles, "max", 256, WC, WW, False)
    assert sorted(rotate_volume(dev, angles)) == ["angles", "level", "values"]


def test_series_translator_depth(ops):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator, view_angles
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        g = make_generator()
        vol = synthetic_hu(5, 64, 64, seed=7)
        plain = SeriesTranslator(g, batch=2, rotate=3, project="max", slab=2)(vol)
        assert sorted(plain["rotation"]) == ["angles", "level", "values"]
        assert all(sorted(d) == ["level", "values"] for d in plain["projections"].values())
        tr = SeriesTranslator(g, batch=2, rotate=3, project="max", slab=2, depth=True, depth_cue=128)
        for out in (tr(vol), tr(vol)):      # the second call reuses the rotator, the projector and the page-locked planes
            assert np.array_equal(out["pix"], plain["pix"]) and np.array_equal(out["level"], plain["level"])
            check_rotation(out["rotation"], out["pix"], view_angles(3), "max", 128, 50.0, 400.0, False)
            check_projection(out["projections"], out["pix"], "max", 2, 128, 50.0, 400.0)
            assert np.array_equal(out["rotation"]["values"], plain["rotation"]["values"])
            assert np.array_equal(out["rotation"]["level"], plain["rotation"]["level"])
            for a, d in plain["projections"].items():
                assert np.array_equal(out["projections"][a]["values"], d["values"])
                assert np.array_equal(out["projections"][a]["level"], d["level"])
        out = SeriesTranslator(g, batch=2, rotate=[0.0, 33.5], rotate_mode="min", hu=True, depth=True)(torch.from_numpy(vol))
        assert "projections" not in out and all(torch.is_tensor(t) for t in out["rotation"].values())
        check_rotation(out["rotation"], out["pix"].numpy(), [0.0, 33.5], "min", 0, 50.0, 400.0, True)
        assert torch.equal(out["rotation"]["cued"], out["rotation"]["level"])
    finally:
        nets.set_default_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------- 7. predict.py --depth
def test_predict_command_line_depth(ops, tmp_path):
    from PIL import Image
    vol = synthetic_hu(5, 48, 40, seed=9)
    np.save(tmp_path / "series.npy", vol)
    (tmp_path / "cfg.yaml").write_text("name: HdGan\nsize: 64\ninput_nc: 1\noutput_nc: 1\n")
    torch.save(make_generator(seed=3).state_dict(), tmp_path / "g.pth")
    cmd = [sys.executable, os.path.join(ROOT, "predict.py"), "--config", str(tmp_path / "cfg.yaml"), "--weights",
           str(tmp_path / "g.pth"), "--input", str(tmp_path / "series.npy"), "--wc", "40", "--ww", "350", "--batch", "2",
           "--output", str(tmp_path / "out.npy"), "--rot-dir", str(tmp_path / "rot"), "--rot-angles", "4", "--rot-span", "180",
           "--mip-dir", str(tmp_path / "mip"), "--depth", "--depth-cue", "128"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    pix = np.load(tmp_path / "out.npy")
    angles = [0.0, 45.0, 90.0, 135.0]
    d = rotate_np.detector(48, 40)
    assert sorted(os.listdir(tmp_path / "rot")) == ["rot_%03d.png" % i for i in range(4)] + ["rotation.npz"]
    npz = np.load(tmp_path / "rot" / "rotation.npz")
    assert sorted(npz.files) == ["angles", "cued", "depth", "level", "values"]
    check_rotation({k: npz[k] for k in npz.files}, pix, angles, "max", 128, 40.0, 350.0, False)
    img = Image.open(tmp_path / "rot" / "rot_000.png")
    assert img.mode == "L" and np.array_equal(np.asarray(img), npz["cued"][0])      # the PNG of view 0 is the cued plane
    assert (npz["cued"] < npz["level"]).any()
    assert sorted(os.listdir(tmp_path / "mip")) == ["axial_000.png", "coronal.png", "projections.npz", "sagittal.png"]
    npz = np.load(tmp_path / "mip" / "projections.npz")
    axes = ["axial", "coronal", "sagittal"]
    assert sorted(npz.files) == sorted(axes + [a + "_depth" for a in axes] + [a + "_cued" for a in axes])
    want = depth_np.project_depth(pix, "max")
    for a in axes:
        assert np.array_equal(npz[a], want[a][0]) and np.array_equal(npz[a + "_depth"], want[a][1])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "mip" / "coronal.png")), npz["coronal_cued"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cfg.yaml", "g.pth", "mip", "out.npy", "rot", "series.npy"]
