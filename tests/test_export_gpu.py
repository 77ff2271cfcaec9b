"""GPU: the series export (csrc/export.hip, cta_gan_amd/infer.py, predict.py, the opt-in export of test()) against the
reference-made fixtures tests/golden/export_*.npz and against its own composition from the public ops."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["87x87", "64x48", "5x7"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib, ops
    _lib.load()
    return ops


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return {name: dict(np.load(os.path.join(golden_dir, "export_%s.npz" % name))) for name in CASES}


def cpu(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. export_slices, fixtures
@pytest.mark.parametrize("name", CASES)
def test_export_slices_equals_the_reference_fixtures(ops, fixtures, name):
    g = fixtures[name]
    x = torch.from_numpy(g["x"]).cuda()
    pix, level = ops.export_slices(x, torch.from_numpy(g["wc"]), torch.from_numpy(g["ww"]))
    assert pix.dtype == torch.int16 and level.dtype == torch.uint8 and pix.shape == x.shape == level.shape
    assert np.array_equal(cpu(pix), g["pix"])
    assert np.array_equal(cpu(level), g["level"])
    # a (B, 1, H, W) generator output is the same planes
    pix4, level4 = ops.export_slices(x.unsqueeze(1), g["wc"].tolist(), g["ww"].tolist())
    assert torch.equal(pix4, pix) and torch.equal(level4, level)
    # every plane alone with a scalar window: planes of odd H W then start at the allocation, not in the middle of it
    for i in range(x.shape[0]):
        p1, l1 = ops.export_slices(x[i:i + 1].clone(), float(g["wc"][i]), float(g["ww"][i]))
        assert np.array_equal(cpu(p1)[0], g["pix"][i]) and np.array_equal(cpu(l1)[0], g["level"][i]), i


def test_export_slices_four_windows_as_one_per_slice_vector(ops, fixtures):
    g = fixtures["64x48"]
    assert g["x"].shape[0] == 4 and len(set(zip(g["wc"].tolist(), g["ww"].tolist()))) == 4
    x = torch.from_numpy(g["x"]).cuda()
    _, level = ops.export_slices(x, torch.from_numpy(g["wc"]).cuda(), torch.from_numpy(g["ww"]).cuda())
    assert np.array_equal(cpu(level), g["level"])
    # the windows in another order give other levels: the vector really is read per slice
    _, other = ops.export_slices(x, torch.from_numpy(g["wc"][::-1].copy()), torch.from_numpy(g["ww"][::-1].copy()))
    assert not np.array_equal(cpu(other), g["level"])


@pytest.mark.parametrize("name", CASES)
def test_export_slices_hu_and_skipped_outputs(ops, fixtures, name):
    g = fixtures[name]
    x = torch.from_numpy(g["x"]).cuda()
    wc, ww = g["wc"].tolist(), g["ww"].tolist()
    pix_hu, level_hu = ops.export_slices(x, wc, ww, hu=True)
    assert np.array_equal(cpu(pix_hu).astype(np.int32), g["pix"].astype(np.int32) - 1024)
    assert np.array_equal(cpu(level_hu), g["level"])
    pix_only, none = ops.export_slices(x, wc, ww, want_level=False)
    assert none is None and np.array_equal(cpu(pix_only), g["pix"])
    # a null pix pointer leaves level unchanged (the op always returns pix, so this goes to the entry point itself)
    from cta_gan_amd import _lib
    lib = _lib.load()
    b, h, w = x.shape
    level = torch.full((b, h, w), 77, dtype=torch.uint8, device="cuda")
    wcv, wwv = torch.tensor(wc, device="cuda"), torch.tensor(ww, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.ctg_export_slices(x.data_ptr(), wcv.data_ptr(), wwv.data_ptr(), b, h, w, None, level.data_ptr(), h, w, 0, st),
               "ctg_export_slices")
    assert np.array_equal(cpu(level), g["level"])
    assert lib.ctg_export_slices(x.data_ptr(), wcv.data_ptr(), wwv.data_ptr(), b, h, w, None, None, h, w, 0, st) == 1      # CTG_EINVAL


@pytest.mark.parametrize("name", CASES)
def test_export_level_is_to_windowdata_before_its_rescale(ops, fixtures, name):
    g = fixtures[name]
    x = torch.from_numpy(g["x"]).cuda()
    wc, ww = g["wc"].tolist(), g["ww"].tolist()
    win = ops.to_windowdata(x, wc, ww)
    assert np.array_equal(cpu(win), g["win"])      # (the same shared arithmetic: ctg_to_windowdata on the boundary values)
    _, level = ops.export_slices(x, wc, ww)
    want = torch.round((win.double() + 1) / 2 * 255).to(torch.uint8)
    assert torch.equal(level, want)


def test_export_slices_outside_the_reference_domain_saturates(ops):
    x = torch.tensor([[[40.0, -40.0, float("nan"), float("inf"), -float("inf"), 1.0, -1.0, 0.0, 15.1]]], device="cuda")
    pix, level = ops.export_slices(x, 50.0, 400.0)
    assert cpu(pix)[0, 0].tolist() == [32767, -32768, 0, 32767, -32768, 4095, 0, 2047, 32767]
    assert cpu(level)[0, 0].tolist()[:5] == [255, 0, 0, 255, 0]
    pix_hu, _ = ops.export_slices(x, 50.0, 400.0, hu=True)
    assert cpu(pix_hu)[0, 0].tolist() == [32767 - 1024, -32768, -1024, 32767 - 1024, -32768, 3071, -1024, 1023, 32767 - 1024]


def test_export_slices_refuses_cpu_tensors(ops):
    with pytest.raises(RuntimeError):
        ops.export_slices(torch.zeros(1, 8, 8), 50.0, 400.0)
    with pytest.raises(RuntimeError):
        ops.series_inputs(torch.zeros(1, 8, 8, dtype=torch.int16), (8, 8))


# ---------------------------------------------------------------------------------------------- 2. export_slices with resize
def test_export_slices_with_resize_equals_resize_then_export(ops, fixtures):
    vals = torch.from_numpy(fixtures["87x87"]["x"].reshape(-1)[:2 * 64 * 64].reshape(2, 64, 64)).cuda()
    wc, ww = [50.0, 60.0], [400.0, 300.0]
    for size in [(48, 40), (81, 67), (64, 64)]:
        pix, level = ops.export_slices(vals, wc, ww, size=size)
        want_pix, want_level = ops.export_slices(ops.resize_nearest(vals, size), wc, ww)
        assert tuple(pix.shape) == (2,) + size
        assert torch.equal(pix, want_pix) and torch.equal(level, want_level), size
    pix_hu, _ = ops.export_slices(vals, wc, ww, size=(48, 40), hu=True, want_level=False)
    assert torch.equal(pix_hu, ops.export_slices(ops.resize_nearest(vals, (48, 40)), wc, ww, hu=True)[0])


# ---------------------------------------------------------------------------------------------- 3. series_inputs
def synthetic_hu(n, h, w, seed):
    rng = np.random.RandomState(seed)
    hu = rng.randint(-1100, 3200, size=(n, h, w)).astype(np.int16)
    hu.reshape(-1)[:8] = [-32768, -2048, -1025, -1024, -1023, 3071, 3072, 32767]      # below -1024 and above 3071 included
    return hu


@pytest.mark.parametrize("shape,size", [((3, 64, 64), (64, 64)), ((3, 48, 40), (64, 64)), ((2, 37, 53), (37, 53)),
                                        ((2, 64, 64), (48, 40))])
def test_series_inputs_equals_its_composition(ops, shape, size):
    hu = torch.from_numpy(synthetic_hu(*shape, seed=5)).cuda()
    assert int(hu.min()) < -1024 and int(hu.max()) > 3071
    got = ops.series_inputs(hu, size)
    want = ops.resize_nearest(ops.hu_to_inputs(hu)[1], size)
    assert got.dtype == torch.float32 and tuple(got.shape) == (shape[0],) + size
    assert torch.equal(got, want)
    assert torch.equal(ops.series_inputs(hu, size[0]) if size[0] == size[1] else got, got)


# ---------------------------------------------------------------------------------------------- 4. SeriesTranslator
def make_generator(seed=0):
    from cta_gan_amd import synth
    from cta_gan_amd.Model.HdGan import Generator
    return synth.fill_module(Generator(1, 1), seed=seed).cuda()


def composed(ops, g, vol, batch, size, wc, ww, hu=False):
    """The same chunks through the public ops, one after another on the current stream."""
    pix, level = [], []
    n, h, w = vol.shape
    with torch.no_grad():
        for s in range(0, n, batch):
            x = ops.series_inputs(torch.from_numpy(vol[s:s + batch]).cuda(), size or (h, w)).unsqueeze(1)
            p, l = ops.export_slices(g(x), wc, ww, size=(h, w), hu=hu)
            pix.append(p)
            level.append(l)
    return cpu(torch.cat(pix)), cpu(torch.cat(level))


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_series_translator_equals_the_chunks_through_the_public_ops(ops, mode):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator, plan_chunks
    nets.set_default_compute_dtype(torch.bfloat16 if mode == "bf16" else mode)
    try:
        g = make_generator()
        # N = 7, batch = 2: four chunks over two slots -- a slot reused before its copy had finished would show
        vol = synthetic_hu(7, 64, 64, seed=7)
        assert len(plan_chunks(7, 2)) == 4
        want_pix, want_level = composed(ops, g, vol, 2, None, 50.0, 400.0)
        assert len(np.unique(want_pix)) > 100      # a real image, not a constant
        tr = SeriesTranslator(g, batch=2)
        out = tr(vol)
        assert isinstance(out["pix"], np.ndarray) and out["pix"].dtype == np.int16 and out["level"].dtype == np.uint8
        assert np.array_equal(out["pix"], want_pix) and np.array_equal(out["level"], want_level)
        again = tr(torch.from_numpy(vol))      # the same object again; a CPU tensor returns tensors
        assert torch.is_tensor(again["pix"]) and not again["pix"].is_cuda
        assert np.array_equal(again["pix"].numpy(), want_pix) and np.array_equal(again["level"].numpy(), want_level)
        # a 48 x 40 series through a generator that runs at 64 x 64 comes back at 48 x 40
        small = synthetic_hu(7, 48, 40, seed=8)
        want_pix, want_level = composed(ops, g, small, 2, (64, 64), 40.0, 350.0, hu=True)
        out = SeriesTranslator(g, batch=2, size=64, wc=40.0, ww=350.0, hu=True)(small)
        assert out["pix"].shape == (7, 48, 40)
        assert np.array_equal(out["pix"], want_pix) and np.array_equal(out["level"], want_level)
        # batch > N, and no level plane
        out = SeriesTranslator(g, batch=16, size=64, hu=True, level=False)(small[:3])
        assert out["level"] is None and np.array_equal(out["pix"][:2], want_pix[:2])
    finally:
        nets.set_default_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------- 5. test() export
def test_trainer_test_exports_only_when_asked(ops, tmp_path, monkeypatch):
    from PIL import Image
    from cta_gan_amd import synth
    from cta_gan_amd.trainer import Hd_Trainer_x2
    cfg = dict(input_nc=1, output_nc=1, size=64, batchSize=2, WC=40.0, WW=400.0)
    tr = Hd_Trainer_x2.__new__(Hd_Trainer_x2)      # test() needs the generator only (Reg needs >= 256)
    tr.config, tr.device = cfg, torch.device("cuda:0")
    tr.netG_A2B = make_generator()
    batches = [{"A2": synth.synth_smooth_images("ex_a%d" % i, 2, 64), "B2": synth.synth_smooth_images("ex_b%d" % i, 2, 64)}
               for i in range(2)]
    batches[0]["A_path"] = ["/data/SE0/IM0007.dcm", "/data/SE0/IM0008.dcm"]
    batches[1]["WC"], batches[1]["WW"] = torch.tensor([60.0, 300.0]), torch.tensor([300.0, 1500.0])
    monkeypatch.chdir(tmp_path)
    plain = tr.test(batches)
    assert not any(tmp_path.iterdir())      # no key: nothing is written
    stems = ["IM0007", "IM0008", "000002", "000003"]
    root = tmp_path / "npy"
    cfg["export_root"] = str(root)
    with_npy = tr.test(batches)
    assert sorted(p.name for p in root.iterdir()) == sorted(s + ".npy" for s in stems)
    root2 = tmp_path / "both"
    cfg["export_root"], cfg["export_png"] = str(root2), True
    with_png = tr.test(batches)
    assert sorted(p.name for p in root2.iterdir()) == sorted([s + ".npy" for s in stems] + [s + ".png" for s in stems])
    for out in (with_npy, with_png):
        assert set(out) == set(plain) and all(np.array_equal(out[k], plain[k]) for k in plain)
    want_pix, want_level = [], []
    with torch.no_grad():
        for bt in batches:
            p, l = ops.export_slices(tr.netG_A2B(bt["A2"].cuda()), bt.get("WC", 40.0), bt.get("WW", 400.0))
            want_pix += list(cpu(p))
            want_level += list(cpu(l))
    for i, s in enumerate(stems):
        for r in (root, root2):
            got = np.load(r / (s + ".npy"))
            assert got.dtype == np.int16 and np.array_equal(got, want_pix[i]), s
        img = Image.open(root2 / (s + ".png"))
        assert img.mode == "L" and np.array_equal(np.asarray(img), want_level[i]), s


# ---------------------------------------------------------------------------------------------- 6. predict.py
def test_predict_command_line(ops, tmp_path):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator
    vol = synthetic_hu(5, 48, 40, seed=9)
    np.save(tmp_path / "series.npy", vol)
    (tmp_path / "cfg.yaml").write_text("name: HdGan\nsize: 64\ninput_nc: 1\noutput_nc: 1\n")
    nets.set_default_compute_dtype("bf16x3")      # predict.py's default
    try:
        g = make_generator(seed=3)
        torch.save(g.state_dict(), tmp_path / "g.pth")
        want = SeriesTranslator(g, batch=2, size=64, wc=40.0, ww=350.0)(vol)
    finally:
        nets.set_default_compute_dtype(torch.float32)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "predict.py"), "--config", str(tmp_path / "cfg.yaml"), "--weights",
                        str(tmp_path / "g.pth"), "--input", str(tmp_path / "series.npy"), "--output", str(tmp_path / "out.npy"),
                        "--level-dir", str(tmp_path / "png"), "--wc", "40", "--ww", "350", "--batch", "2"],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "compute mode: bf16x3" in r.stdout
    got = np.load(tmp_path / "out.npy")
    assert got.dtype == np.int16 and np.array_equal(got, want["pix"])
    from PIL import Image
    names = sorted(os.listdir(tmp_path / "png"))
    assert names == ["%06d.png" % i for i in range(5)]
    for i, nm in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "png" / nm)), want["level"][i])
