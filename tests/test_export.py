"""CPU: the arithmetic of the series export restated in numpy equals the reference-made fixtures bit for bit; the chunk / slot
plan of SeriesTranslator; predict.py's command line."""
import os
import sys

import numpy as np
import pytest

import export_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["87x87", "64x48", "5x7"]


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, "export_%s.npz" % name))


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_equals_the_fixtures(golden_dir, name):
    g = load(golden_dir, name)
    x = g["x"]
    assert x.dtype == np.float32 and x.min() >= -1 and x.max() <= 1
    assert np.array_equal(export_np.pix_np(x), g["pix"])
    assert np.array_equal(export_np.pix_np(x, hu=True), g["pix"].astype(np.int32) - 1024)
    for i in range(x.shape[0]):
        level = export_np.level_np(x[i], g["wc"][i], g["ww"][i])
        assert np.array_equal(level, g["level"][i]), i
        assert np.array_equal(export_np.window_np(level), g["win"][i]), i


def test_fixtures_cover_what_they_are_for(golden_dir):
    g = load(golden_dir, "87x87")
    assert g["x"].shape[0] >= 2 and (g["x"].shape[1] * g["x"].shape[2]) % 2 == 1      # later planes start misaligned
    assert set(np.unique(g["pix"])) == set(range(4096))
    assert np.unique(g["level"]).size == 256
    for v in (-1.0, np.nextafter(np.float32(-1), np.float32(0)), 1.0):
        assert (g["x"] == np.float32(v)).any()
    g = load(golden_dir, "64x48")
    assert g["x"].shape == (4, 64, 48)
    assert sorted(zip(g["wc"].tolist(), g["ww"].tolist())) == sorted([(50., 400.), (40., 400.), (60., 300.), (300., 1500.)])
    for i in range(4):
        assert np.unique(g["level"][i]).size == 256
    assert load(golden_dir, "5x7")["x"].shape[1:] == (5, 7)


def test_fixture_values_tell_wrong_arithmetic_apart(golden_dir):
    """The boundary values are what pins the operation order: a float64 evaluation and rounding instead of truncation each
    miss thousands of the pix values."""
    g = load(golden_dir, "87x87")
    x64 = g["x"].astype(np.float64)
    assert (np.trunc((x64 + 1) * 0.5 * 4095).astype(np.int16) != g["pix"]).sum() >= 2048
    assert (np.rint(export_np.stored_np(g["x"])).astype(np.int16) != g["pix"]).sum() >= 8000


@pytest.mark.parametrize("n,want", [
    (1, [(0, 1, 0)]),
    (2, [(0, 2, 0)]),
    (5, [(0, 2, 0), (2, 4, 1), (4, 5, 0)]),
    (7, [(0, 2, 0), (2, 4, 1), (4, 6, 0), (6, 7, 1)]),
])
def test_plan_chunks(n, want):
    from cta_gan_amd.infer import plan_chunks
    assert plan_chunks(n, 2) == want


def test_plan_chunks_edges():
    from cta_gan_amd.infer import plan_chunks
    assert plan_chunks(3, 16) == [(0, 3, 0)]      # batch > n: one short chunk
    assert plan_chunks(0, 4) == []
    plan = plan_chunks(37, 5)
    assert [s for s, _, _ in plan] == list(range(0, 37, 5)) and plan[-1][1] == 37
    assert all(e - s <= 5 for s, e, _ in plan) and [q for _, _, q in plan] == [i % 2 for i in range(len(plan))]
    with pytest.raises(ValueError):
        plan_chunks(3, 0)
    with pytest.raises(ValueError):
        plan_chunks(-1, 2)


def predict_module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import predict
    return predict


def test_predict_arguments():
    predict = predict_module()
    p = predict.build_parser()
    o = p.parse_args(["--weights", "g.pth", "--input", "in.npy", "--output", "out.npy"])
    assert (o.config, o.weights, o.input, o.output) == ("Yaml/HdGan.yaml", "g.pth", "in.npy", "out.npy")
    assert o.level_dir is None and o.hu is False and (o.wc, o.ww, o.batch) == (50.0, 400.0, 16) and o.dtype is None
    assert predict.DEFAULT_DTYPE == "bf16x3"
    o = p.parse_args(["--config", "c.yaml", "--weights", "g.pth", "--input", "i.npy", "--output", "o.npy", "--level-dir", "png",
                      "--hu", "--wc", "40", "--ww", "350", "--batch", "4", "--dtype", "bf16"])
    assert (o.config, o.level_dir, o.hu, o.wc, o.ww, o.batch, o.dtype) == ("c.yaml", "png", True, 40.0, 350.0, 4, "bf16")
    for bad in (["--input", "i.npy", "--output", "o.npy"], ["--weights", "g.pth", "--input", "i.npy", "--output", "o.npy",
                                                          "--dtype", "fp16"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_predict_default_dtype_is_train_py_default():
    text = open(os.path.join(ROOT, "train.py")).read()
    assert 'else "%s")' % predict_module().DEFAULT_DTYPE in text
