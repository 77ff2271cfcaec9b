"""GPU: lines in any direction (ctg_reformat_lines through ops.reformat_lines / ops.LineTable; cta_gan_amd/infer.py:
VolumeReformatter, reformat_volume, SeriesTranslator(reformat=...); predict.py --mpr-dir / --tumble-dir / --cpr-dir) against the
numpy restatement tests/reformat_np.py, which is a plain loop over the steps of a ray with a counted mask, and against the
rotation kernels of project_rotate.hip where a line table can express their view.  Exact integer arithmetic: every comparison is
np.array_equal, never a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import reformat_np
from test_rotate_gpu import make_generator, synthetic_hu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("max", "min", "mean")
SAMPLINGS = reformat_np.SAMPLINGS
ANGLES = [0, 30, 45, 90, 200]
VOLUMES = [(5, 7, 9), (13, 33, 31), (1, 6, 5), (4, 1, 1)]
US = (1, 31, 32, 33, 70)
TS = (1, 2, 7, 8, 9, 33, 70)      # across the 8 lanes of a ray and the trip of 32 steps
WC, WW = 300.0, 30000.0           # a window wide enough that the levels of random int16 values differ

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib, ops
    _lib.load()
    return ops


def cpu(t):
    return None if t is None else t.cpu().numpy()


def planted(n, h, w, seed):
    """Random int16 with both extremes planted; the last slice is all 32767 (the largest sums a mean can meet) when there are
    several."""
    vol = np.random.RandomState(seed).randint(-32768, 32768, size=(n, h, w)).astype(np.int16)
    vol[0, 0, 0], vol[0, h - 1, w - 1], vol[n // 2, h // 2, w // 2] = -32768, 32767, -32768
    if n > 2:
        vol[n - 1] = 32767
    return vol


def raw_table(shape, lines, u, t, a=(1.4, 0.3, 0.2), b=(0.2, 1.3, 0.4), c=(0.1, 0.2, 0.8)):
    """int64 [lines, 9]: an oblique sheaf of lines through the volume's centre, given in units of the volume's extent (x of w, y
    of h, z of n): a line spans `a`, its rays span `b`, the lines are spread over `c`.  a and b reach past the faces, so that the
    ends of a line, and of a ray, are outside and some rays miss the volume altogether.  Not a view of infer.py: the kernel takes
    any table."""
    n, h, w = shape
    size = np.array([w, h, n], dtype=np.float64)
    a, b, c = (np.array(v, dtype=np.float64) * size for v in (a, b, c))
    l = np.arange(lines, dtype=np.float64)[:, None]
    start = size / 2 - (u - 1) / 2.0 * a / u - (t - 1) / 2.0 * b / t + (l - (lines - 1) / 2.0) * c / lines      # edge-based: floor = voxel
    out = np.empty((lines, 9), dtype=np.int64)
    out[:, 0::3] = np.floor(start * 65536.0 + 0.5)
    out[:, 1::3] = np.floor(a / u * 65536.0 + 0.5)
    out[:, 2::3] = np.floor(b / t * 65536.0 + 0.5)
    return out


def check_case(ops, vol, dev, lines, u, t, expect_fill, modes=MODES, samplings=SAMPLINGS, hu=False, fill=None, what=()):
    """Every mode and sampling of one table: the conditions on the numpy side first, then values and level bit for bit."""
    table = ops.LineTable(lines, u, t)
    for sampling in samplings:
        for mode in modes:
            kw = {} if fill is None else {"fill": fill}
            want, cnt = reformat_np.reformat(vol, lines, u, t, mode, sampling, fill=(-1024 if hu else 0) if fill is None else fill)
            assert (cnt > 0).mean() >= 0.25, what      # a case that is nearly all fill proves nothing
            if expect_fill:
                assert (cnt == 0).any(), what
            values, level = ops.reformat_lines(dev, table, u, t, mode, wc=WC, ww=WW, hu=hu, sampling=sampling, **kw)
            assert values.dtype == torch.int16 and level.dtype == torch.uint8 and tuple(values.shape) == want.shape == tuple(level.shape)
            assert np.array_equal(cpu(values), want), what + (sampling, mode)
            assert np.array_equal(cpu(level), reformat_np.level(want, WC, WW, hu)), what + (sampling, mode)


@pytest.fixture(scope="module")
def volumes():
    host = {shape: planted(*shape, seed=sum(shape)) for shape in VOLUMES}
    return host, {shape: torch.from_numpy(v).cuda() for shape, v in host.items()}


# ---------------------------------------------------------------------------------------------- 1. one call equals numpy
@pytest.mark.parametrize("shape", VOLUMES, ids=lambda s: "%dx%dx%d" % s)
def test_every_line_length_and_ray_length(ops, volumes, shape):
    """U x T over an oblique sheaf of 3 lines (10 where T = 1: more than one patch of 8 lines): all modes, both samplings."""
    host, dev = volumes
    for u in US:
        for t in TS:
            lines = raw_table(shape, 10 if t == 1 else 3, u, t)
            check_case(ops, host[shape], dev[shape], lines, u, t, expect_fill=u >= 31, what=(shape, u, t))


@pytest.mark.parametrize("axis", ["x", "z", (1, 1, 1)], ids=str)
@pytest.mark.parametrize("aspect", [1.0, 2.5])
def test_orbits_about_three_axes(ops, volumes, axis, aspect):
    """The tables of infer.orbit_lines at 0, 30, 45, 90 and 200 degrees; detectors two voxels wider than the volume (not its
    diagonal), so that most rays cross it while the rim and the corners of the turned views miss it."""
    from cta_gan_amd.infer import orbit_lines
    host, dev = volumes
    for shape in ((13, 33, 31), (5, 7, 9)):
        n, h, w = shape
        rows, cols, depth = int(np.ceil(n * aspect)) + 2, w + 2, h + 1
        made = orbit_lines(*shape, ANGLES, axis=axis, rows=rows, cols=cols, depth=depth, aspect=aspect)
        lines, steps = made
        assert lines.shape == (len(ANGLES), rows, 9) and steps == depth and made.cols == cols
        check_case(ops, host[shape], dev[shape], lines, cols, steps, expect_fill=True, hu=True, what=(shape, axis, aspect))
    made = orbit_lines(13, 33, 31, [30.0], axis=axis, rows=7, cols=33, depth=17, oversample=2, aspect=aspect)      # steps of half a voxel
    check_case(ops, host[(13, 33, 31)], dev[(13, 33, 31)], made[0], 33, 34, expect_fill=False, modes=("mean",), what=(axis, aspect, 2))


def test_a_step_of_two_and_a_half_voxels_planes_and_a_table_wholly_outside(ops, volumes):
    from cta_gan_amd.infer import curved_lines, oblique_lines
    host, dev = volumes
    shape = (13, 33, 31)
    vol, d = host[shape], dev[shape]
    lines = raw_table(shape, 5, 16, 8)
    lines[:, 1] = 163840      # 2.5 voxels per sample along x: 16 samples span 40 columns of 31
    lines[:, 0] = -(4 << 16) - 1234
    check_case(ops, vol, d, lines, 16, 8, expect_fill=True, what=("step 2.5",))
    made = oblique_lines(*shape, (1, 2, 3), count=3, pitch=2.5, thick=2, aspect=2.5)      # double-oblique slabs of an anisotropic volume
    assert made[0].ndim == 3 and made[1] == 2
    check_case(ops, vol, d, made[0], made.cols, 2, expect_fill=True, what=("oblique",))
    made = oblique_lines(*shape, (1, 2, 3), up=(0, 1, 0), rows=20, cols=20)      # T = 1 planes, an `up` of the caller's
    check_case(ops, vol, d, made[0], 20, 1, expect_fill=False, fill=-555, what=("plane",))
    pts = [[0, 5, 4], [4, 12, 16], [9, 22, 20], [12, 29, 27]]
    made = curved_lines(*shape, pts, angles=(0.0, 60.0), cols=21, depth=3, pitch=0.75, aspect=1.0)
    check_case(ops, vol, d, made[0], 21, 3, expect_fill=False, what=("curved",))
    outside = raw_table(shape, 4, 33, 9)
    outside[:, 0] += 200 << 16      # 200 columns to the right of the volume
    table = ops.LineTable(outside, 33, 9)
    for sampling in SAMPLINGS:
        for mode in MODES:
            want, cnt = reformat_np.reformat(vol, outside, 33, 9, mode, sampling, fill=-321)
            assert (cnt == 0).all() and (want == -321).all()
            values, level = ops.reformat_lines(d, table, 33, 9, mode, fill=-321, wc=WC, ww=WW, sampling=sampling)
            assert np.array_equal(cpu(values), want) and np.array_equal(cpu(level), reformat_np.level(want, WC, WW))


def test_values_only_level_only_a_two_byte_aligned_view_and_a_host_table(ops, volumes):
    host, dev = volumes
    shape = (13, 33, 31)
    vol, d = host[shape], dev[shape]
    for u, t in ((33, 9), (33, 1)):
        lines = raw_table(shape, 9, u, t).reshape(3, 3, 9)      # any leading shape
        want, _ = reformat_np.reformat(vol, lines, u, t, "mean", "trilinear")
        want_level = reformat_np.level(want, WC, WW)
        assert want.shape == (3, 3, u)
        kw = dict(wc=WC, ww=WW, sampling="trilinear")
        values, level = ops.reformat_lines(d, lines, u, t, "mean", want_level=False, **kw)      # a host table, checked by the call
        assert level is None and np.array_equal(cpu(values), want)
        values, level = ops.reformat_lines(d, torch.from_numpy(lines), u, t, 2, want_values=False, **kw)
        assert values is None and np.array_equal(cpu(level), want_level)
        buf = torch.empty(vol.size + 1, dtype=torch.int16, device="cuda")      # one element into a buffer: only 2-byte aligned
        shifted = buf[1:].view(*shape)
        shifted.copy_(d)
        assert shifted.is_contiguous() and shifted.data_ptr() % 4 == 2
        values, level = ops.reformat_lines(shifted, lines, u, t, "mean", **kw)
        assert np.array_equal(cpu(values), want) and np.array_equal(cpu(level), want_level)


# ---------------------------------------------------------------------------------------------- 2. the rotation kernels as the yardstick
@pytest.mark.parametrize("sampling,rotating", [("nearest", "nearest"), ("trilinear", "bilinear")])
def test_an_orbit_about_z_equals_project_rotate(ops, volumes, sampling, rotating):
    """fz = 0 on every sample of an orbit about z, so trilinear is the bilinear rotation; the kernels of project_rotate.hip are
    the parent commit's."""
    from cta_gan_amd.infer import default_detector, orbit_lines, rotation_coefficients
    host, dev = volumes
    for shape in ((13, 33, 31), (5, 7, 9)):
        n, h, w = shape
        d = default_detector(h, w)
        for s in (1, 2):
            lines, steps = orbit_lines(n, h, w, ANGLES, axis="z", rows=n, cols=d, depth=d, oversample=s)
            coef = ops.RotateTable([rotation_coefficients(a, h, w, oversample=s) for a in ANGLES])
            for mode in MODES:
                values = torch.empty((len(ANGLES), n, d), dtype=torch.int16, device="cuda")
                level = torch.empty((len(ANGLES), n, d), dtype=torch.uint8, device="cuda")
                ops.project_rotate(dev[shape], 0, coef, steps, mode, values=values, level=level, wc=WC, ww=WW, sampling=rotating)
                got = ops.reformat_lines(dev[shape], lines, d, steps, mode, wc=WC, ww=WW, sampling=sampling)
                assert torch.equal(got[0], values) and torch.equal(got[1], level), (shape, s, mode)
                assert len(torch.unique(values)) > 10


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_launch_nothing(ops, volumes):
    from cta_gan_amd import _lib
    host, dev = volumes
    shape = (5, 7, 9)
    n, h, w = shape
    d = dev[shape]
    lines = raw_table(shape, 4, 33, 9)
    table = ops.LineTable(lines, 33, 9)
    for kw in (dict(want_values=False, want_level=False), dict(sampling="bilinear"), dict(sampling=1), dict(mode="median"), dict(mode=3),
               dict(fill=40000), dict(vol=d.cpu()), dict(vol=d.int()), dict(vol=d[0]), dict(lines=table.dev), dict(u=32), dict(t=8),
               dict(lines=lines[:, :8]), dict(u=0, lines=lines), dict(t=4097, lines=lines),
               dict(lines=np.full((1, 9), 2 ** 27, dtype=np.int64))):
        args = dict(vol=d, lines=table, u=33, t=9, mode="max")
        args.update(kw)
        with pytest.raises(RuntimeError):
            ops.reformat_lines(**args)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    values = torch.full((4, 33), 12345, dtype=torch.int16, device="cuda")
    level = torch.full((4, 33), 77, dtype=torch.uint8, device="cuda")
    P, C, V, L = d.data_ptr(), table.dev.data_ptr(), values.data_ptr(), level.data_ptr()

    def call(vol=P, N=n, H=h, W=w, lines=C, Ln=4, U=33, T=9, mode=0, sampling=0, fill=0, values=V, level=L):
        return lib.ctg_reformat_lines(vol, N, H, W, lines, Ln, U, T, mode, sampling, fill, 50.0, 400.0, 0, values, level, st)

    for kw in (dict(vol=None), dict(lines=None), dict(values=None, level=None), dict(N=0), dict(N=4097), dict(H=0), dict(H=4097), dict(W=0),
               dict(W=4097), dict(U=0), dict(U=4097), dict(T=0), dict(T=4097), dict(Ln=0), dict(Ln=-1), dict(mode=-1), dict(mode=3),
               dict(sampling=-1), dict(sampling=2), dict(fill=-32769), dict(fill=32768), dict(vol=P + 1), dict(lines=C + 2),
               dict(values=V + 1), dict(Ln=2 ** 31 - 1, U=33)):
        assert call(**kw) == 1, kw      # CTG_EINVAL
    torch.cuda.synchronize()
    assert (values == 12345).all() and (level == 77).all()      # nothing was launched
    assert call() == 0 and call(values=None, sampling=1, mode=2) == 0 and call(level=None, T=1, Ln=4) == 0
    torch.cuda.synchronize()
    assert not (level == 77).all()


# ---------------------------------------------------------------------------------------------- 4. the host layer
def tables_for(aspect=1.0):
    from cta_gan_amd.infer import curved_lines, oblique_lines, orbit_lines
    return {"planes": lambda n, h, w: oblique_lines(n, h, w, (1, 1, 2), count=3, pitch=2.0, thick=2, aspect=aspect),
            "tumble": lambda n, h, w: orbit_lines(n, h, w, [0.0, 40.0], axis="x", aspect=aspect),
            "curved": lambda n, h, w: curved_lines(n, h, w, [[0, 3, 4], [n // 2, h // 2, w // 2], [n - 1, h - 4, w - 5]], cols=9, aspect=aspect)}


def check_reformats(got, pix, tables, mode, sampling, wc, ww, hu, level=True):
    n, h, w = pix.shape
    assert sorted(got) == sorted(tables)
    hit = False
    for name, make in tables.items():
        made = make(n, h, w)
        want, cnt = reformat_np.reformat(pix, made[0], made.cols, made[1], mode, sampling, fill=-1024 if hu else 0)
        hit = hit or ((cnt > 0).any() and (cnt == 0).any())
        d = {k: None if t is None else np.asarray(t.cpu() if torch.is_tensor(t) else t) for k, t in got[name].items()}
        assert sorted(d) == ["level", "values"]
        assert d["values"].dtype == np.int16 and np.array_equal(d["values"], want), name
        if level:
            assert d["level"].dtype == np.uint8 and np.array_equal(d["level"], reformat_np.level(want, wc, ww, hu)), name
        else:
            assert d["level"] is None
    assert hit


def test_volume_reformatter_in_shuffled_chunks_and_reformat_volume(ops, monkeypatch):
    from cta_gan_amd.infer import VolumeReformatter, reformat_volume
    vol = planted(7, 19, 23, seed=3)
    n, h, w = vol.shape
    dev = torch.from_numpy(vol).cuda()
    tables = tables_for(aspect=1.5)
    calls = []
    monkeypatch.setattr(ops, "reformat_lines", (lambda f: lambda *a, **k: (calls.append("reformat_lines"), f(*a, **k))[1])(ops.reformat_lines))
    ref = VolumeReformatter(n, h, w, tables, mode="mean", sampling="trilinear", wc=WC, ww=WW, hu=True)
    nbytes = ref.nbytes
    assert ref.volume is None and nbytes > 2 * vol.size      # known before the first chunk
    for s in (4, 0, 6, 2):      # chunks of 2 (the last of 1) in shuffled order
        ref.update(dev[s:s + 2], s)
        if s != 2:
            with pytest.raises(RuntimeError, match="exactly once"):
                ref.result()
    ref.update(dev[:0], 0)      # an empty chunk changes nothing
    assert not calls
    got = ref.result()
    assert calls == ["reformat_lines"] * 3 and ref.nbytes == nbytes      # one launch per table
    assert all(t.is_cuda for d in got.values() for t in d.values())
    check_reformats(got, vol, tables, "mean", "trilinear", WC, WW, True)
    whole = reformat_volume(dev, tables, mode="mean", sampling="trilinear", wc=WC, ww=WW, hu=True)
    for name in tables:
        assert torch.equal(whole[name]["values"], got[name]["values"]) and torch.equal(whole[name]["level"], got[name]["level"])
    ref.update(dev[:2], 0)      # a slice twice
    with pytest.raises(RuntimeError, match="exactly once"):
        ref.result()
    ref.reset()
    ref.update(dev, 0)
    assert torch.equal(ref.result()["planes"]["values"], got["planes"]["values"])
    with pytest.raises(RuntimeError):
        ref.update(dev, 1)
    got = reformat_volume(vol, tables, mode="min", sampling="nearest", batch=3, level=False)      # a host array returns arrays
    assert all(isinstance(d["values"], np.ndarray) for d in got.values())
    check_reformats(got, vol, tables, "min", "nearest", 50.0, 400.0, False, level=False)
    got = reformat_volume(torch.from_numpy(vol), {"a": (tables["planes"](n, h, w)[0], 2)}, cols=tables["planes"](n, h, w).cols)
    assert torch.is_tensor(got["a"]["values"]) and not got["a"]["values"].is_cuda      # a bare pair with cols; a CPU tensor returns tensors
    check_reformats(got, vol, {"a": tables["planes"]}, "max", "trilinear", 50.0, 400.0, False)
    with pytest.raises(RuntimeError):
        reformat_volume(vol.astype(np.int32), tables)


def test_series_translator_reformat(ops, monkeypatch):
    from cta_gan_amd import _lib, nets
    from cta_gan_amd.infer import SeriesTranslator
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        g = make_generator()
        vol = synthetic_hu(5, 64, 64, seed=7)
        launched = set()
        monkeypatch.setattr(_lib, "check", (lambda f: lambda status, what: (launched.add(what), f(status, what))[1])(_lib.check))
        plain_tr = SeriesTranslator(g, batch=2, rotate=3)
        plain_tr(vol)      # (the generator's first forward also packs its weights)
        launched.clear()
        plain = plain_tr(vol)
        before = set(launched)
        launched.clear()
        none_tr = SeriesTranslator(g, batch=2, rotate=3, reformat=None)
        none = none_tr(vol)
        # with reformat=None the result and the launches are what they were, and nothing is kept
        assert sorted(none) == sorted(plain) == ["level", "pix", "rotation"] and launched == before and "ctg_reformat_lines" not in before
        assert "reformat" not in none_tr._views and "reformat" not in none_tr._view_host and "reformat" not in plain_tr._views
        tables = tables_for()
        tr = SeriesTranslator(g, batch=2, rotate=3, reformat=tables, reformat_options={"mode": "mean", "sampling": "nearest"})
        launched.clear()
        for out in (tr(vol), tr(vol)):      # the second call reuses the reformatter and the page-locked planes
            assert np.array_equal(out["pix"], plain["pix"]) and np.array_equal(out["level"], plain["level"])
            assert np.array_equal(out["rotation"]["values"], plain["rotation"]["values"])
            check_reformats(out["reformat"], out["pix"], tables, "mean", "nearest", 50.0, 400.0, False)
        assert launched == before | {"ctg_reformat_lines"}
        whole = SeriesTranslator(g, batch=2, hu=True, subtract=True, project_source="sub", reformat=tables)(torch.from_numpy(vol))
        assert all(torch.is_tensor(t) for d in whole["reformat"].values() for t in d.values())
        check_reformats(whole["reformat"], whole["sub"].numpy(), tables, "max", "trilinear", 150.0, 300.0, True)      # in sub_window
    finally:
        nets.set_default_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------- 5. predict.py
def test_predict_command_line_reformats(ops, tmp_path):
    from PIL import Image
    from cta_gan_amd.infer import curved_lines, oblique_lines, orbit_lines, view_angles
    vol = synthetic_hu(6, 48, 40, seed=9)
    np.save(tmp_path / "series.npy", vol)
    pts = np.array([[0.0, 10.0, 8.0], [2.5, 24.0, 20.0], [5.0, 40.0, 30.0]])
    np.save(tmp_path / "line.npy", pts)
    (tmp_path / "cfg.yaml").write_text("name: HdGan\nsize: 64\ninput_nc: 1\noutput_nc: 1\n")
    torch.save(make_generator(seed=3).state_dict(), tmp_path / "g.pth")
    cmd = [sys.executable, os.path.join(ROOT, "predict.py"), "--config", str(tmp_path / "cfg.yaml"), "--weights",
           str(tmp_path / "g.pth"), "--input", str(tmp_path / "series.npy"), "--batch", "4", "--output", str(tmp_path / "out.npy"),
           "--wc", "1000", "--ww", "4200", "--aspect", "2.5", "--mip-mode", "mean",
           "--mpr-dir", str(tmp_path / "mpr"), "--mpr-normal", "1,2,1", "--mpr-count", "3", "--mpr-pitch", "4", "--mpr-thick", "2",
           "--tumble-dir", str(tmp_path / "tumble"), "--tumble-angles", "4",
           "--cpr-dir", str(tmp_path / "cpr"), "--cpr-centreline", str(tmp_path / "line.npy"), "--cpr-angles", "2", "--cpr-width", "17",
           "--cpr-thick", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    pix = np.load(tmp_path / "out.npy")
    n, h, w = pix.shape
    made = {"mpr": oblique_lines(n, h, w, (1.0, 2.0, 1.0), count=3, pitch=4.0, thick=2, aspect=2.5),
            "tumble": orbit_lines(n, h, w, view_angles(4), axis="x", aspect=2.5),
            "cpr": curved_lines(n, h, w, pts, angles=view_angles(2, 180.0), cols=17, depth=3, aspect=2.5)}
    angles = {"tumble": view_angles(4), "cpr": view_angles(2, 180.0)}
    for kind, lines in made.items():
        count = lines[0].shape[0]
        assert sorted(os.listdir(tmp_path / kind)) == sorted(["%s_%03d.png" % (kind, i) for i in range(count)] + ["reformat.npz"])
        npz = np.load(tmp_path / kind / "reformat.npz")
        assert sorted(npz.files) == (["angles"] if kind in angles else []) + ["level", "values"]
        want, cnt = reformat_np.reformat(pix, lines[0], lines.cols, lines[1], "mean", "trilinear")
        assert (cnt > 0).any()
        assert npz["values"].dtype == np.int16 and np.array_equal(npz["values"], want), kind
        assert npz["level"].dtype == np.uint8 and np.array_equal(npz["level"], reformat_np.level(want, 1000.0, 4200.0)), kind
        if kind in angles:
            assert npz["angles"].tolist() == angles[kind]
        for i in range(count):
            img = Image.open(tmp_path / kind / ("%s_%03d.png" % (kind, i)))
            assert img.mode == "L" and np.array_equal(np.asarray(img), npz["level"][i])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cfg.yaml", "cpr", "g.pth", "line.npy", "mpr", "out.npy", "series.npy", "tumble"]
