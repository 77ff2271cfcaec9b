"""CPU: host side of the `noise_level` augmentation (cta_gan_amd/trainer/augment.py) -- inverse matrix, PIL's fixed-point
coefficients, the parameter draws -- and the numpy restatement of PIL's fixed-point gather (tests/affine_np.py), all against
PIL's own output in tests/golden/affine_*.npz (scripts/make_golden_affine.py)."""
import glob
import os
import random

import numpy as np
import pytest

from affine_np import pil_affine_fixed

FILL = -1.0


def _fixtures(golden_dir):
    files = sorted(f for f in glob.glob(os.path.join(golden_dir, "affine_*.npz")) if "affine_hu_" not in f)
    assert len(files) >= 8
    return [np.load(f) for f in files]


def _hu_fixture(golden_dir):
    (f,) = glob.glob(os.path.join(golden_dir, "affine_hu_*.npz"))
    return np.load(f)


def _params_sets(golden_dir):
    """(h, w, (angle, tx, ty, scale), matrix, coef) of every stored draw, the two of the HU case included."""
    out = []
    for z in _fixtures(golden_dir):
        out.append((*z["img"].shape, z["params"], z["matrix"], z["coef"]))
    z = _hu_fixture(golden_dir)
    for q in range(2):
        out.append((*z["hu"].shape, z["params"][q], z["matrix"][q], z["coef"][q]))
    return out


def test_inverse_matrix_and_fixed_coefficients_reproduce_the_fixtures(golden_dir):
    from cta_gan_amd.trainer.augment import fixed_coefficients, inverse_matrix
    for h, w, (angle, tx, ty, scale), matrix, coef in _params_sets(golden_dir):
        m = inverse_matrix((w * 0.5, h * 0.5), angle, (tx, ty), scale)
        assert np.array(m, dtype=np.float64).tobytes() == matrix.tobytes()      # to the last bit
        a = fixed_coefficients(m, (h, w))
        assert all(isinstance(v, int) for v in a) and a == [int(v) for v in coef]


def test_identity_matrix_gives_the_identity_coefficients():
    from cta_gan_amd.trainer.augment import fixed_coefficients, inverse_matrix
    a = fixed_coefficients(inverse_matrix((3.5, 2.5), 0.0, (0, 0), 1.0), (5, 7))
    assert a == [65536, 0, 32768, 0, 65536, 32768]
    img = np.arange(35, dtype=np.float32).reshape(5, 7)
    assert np.array_equal(pil_affine_fixed(img, a, FILL), img)


def test_fixed_coefficients_refuse_what_leaves_32_bits():
    from cta_gan_amd.trainer.augment import fixed_coefficients
    m = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert fixed_coefficients(m, (32768, 32767))      # 32768 + 65536 * 32766 < 2^31
    with pytest.raises(OverflowError):
        fixed_coefficients(m, (32768, 32769))
    with pytest.raises(OverflowError):
        fixed_coefficients([1.0, 0.0, 40000.0, 0.0, 1.0, 0.0])


def test_numpy_restatement_reproduces_pil_fixtures(golden_dir):
    for z in _fixtures(golden_dir):
        assert np.array_equal(pil_affine_fixed(z["img"], z["coef"], FILL), z["out"])
    shares = [float((z["out"] == FILL).mean()) for z in _fixtures(golden_dir)]
    assert max(shares) > 0.05 and min(shares) == 0.0


def test_hu_fixture_is_the_oracle_arithmetic_then_the_gather(golden_dir):
    from oracle.ref_inputs import read_ori_w_arith
    z = _hu_fixture(golden_dir)
    i1, i2 = read_ori_w_arith(z["hu"].copy())
    assert np.array_equal(pil_affine_fixed(i1.astype(np.float32), z["coef"][0], FILL), z["win"])
    assert np.array_equal(pil_affine_fixed(i2.astype(np.float32), z["coef"][1], FILL), z["full"])


def test_numpy_restatement_matches_pil_on_fresh_cases():
    Image = pytest.importorskip("PIL.Image")
    from cta_gan_amd.trainer.augment import RandomAffine, fixed_coefficients, inverse_matrix
    rng = np.random.RandomState(7)
    for i, ((h, w), level) in enumerate([((37, 53), 1), ((64, 48), 2), ((5, 7), 5), ((64, 48), 5), ((37, 53), 5), ((33, 9), 2)]):
        ra = RandomAffine(level, translate=[0.02 * level] * 2, scale=[1 - 0.02 * level, 1 + 0.02 * level], fillcolor=-1, seed=i)
        for _ in range(5):
            angle, t, s = ra.get_params(w, h)
            m = inverse_matrix((w * 0.5, h * 0.5), angle, t, s)
            img = rng.rand(h, w).astype(np.float32)
            ref = Image.fromarray(img, "F").transform((w, h), Image.Transform.AFFINE, m, Image.Resampling.NEAREST, fillcolor=FILL)
            assert np.array_equal(pil_affine_fixed(img, fixed_coefficients(m, (h, w)), FILL), np.asarray(ref)), (h, w, level)


# tx = round(uniform(-t W, t W)) can exceed t W by the rounding when frac(t W) >= 0.5 (torchvision's formula does the same):
# the sizes here have frac(0.02 level W) < 0.5, where |tx| <= 0.02 level W holds for every draw
@pytest.mark.parametrize("level,w,h", [(1, 512, 512), (2, 53, 37), (5, 64, 44)])
def test_get_params_ranges_and_replay(level, w, h):
    from cta_gan_amd.trainer.augment import RandomAffine
    ra = RandomAffine(level, translate=[0.02 * level, 0.02 * level], scale=[1 - 0.02 * level, 1 + 0.02 * level], fillcolor=-1,
                      seed=123)
    rep = random.Random(123)
    for _ in range(200):
        angle, (tx, ty), scale = ra.get_params(w, h)
        assert abs(angle) <= level
        assert tx == int(tx) and ty == int(ty) and abs(tx) <= 0.02 * level * w and abs(ty) <= 0.02 * level * h
        assert 1 - 0.02 * level <= scale <= 1 + 0.02 * level
        # this project's contract: angle, tx, ty, scale, in this order, from the instance's own generator
        e_angle = rep.uniform(-level, level)
        e_tx = round(rep.uniform(-0.02 * level * w, 0.02 * level * w))
        e_ty = round(rep.uniform(-0.02 * level * h, 0.02 * level * h))
        e_scale = rep.uniform(1 - 0.02 * level, 1 + 0.02 * level)
        assert (angle, tx, ty, scale) == (e_angle, e_tx, e_ty, e_scale)


def test_sampling_leaves_the_global_generator_alone_and_follows_the_key_order():
    from cta_gan_amd.trainer.augment import NoiseAugmenter, RandomAffine
    random.seed(99)
    state = random.getstate()
    aug = NoiseAugmenter(2, 256, seed=5)
    shapes = {"B2": (3, 64, 48), "A2": (3, 64, 48), "B1": (3, 37, 53)}
    coef = aug.sample(shapes)
    assert random.getstate() == state
    # per sample, keys in the order A1, A2, B1, B2, A, B, one independent draw each
    ra = RandomAffine(2, translate=[0.04, 0.04], scale=[0.96, 1.04], fillcolor=-1, seed=5)
    for i in range(3):
        for k in ("A2", "B1", "B2"):
            _, h, w = shapes[k]
            assert coef[k][i] == ra.coefficients(w, h), (i, k)
    assert coef["B1"] != coef["B2"]
    # shared_per_series: B2 reuses B1's parameters (same size here, so the same coefficients), A2 has no A1 and draws
    shared = NoiseAugmenter(2, 256, seed=5, shared_per_series=True).sample({"A2": (2, 64, 48), "B1": (2, 64, 48), "B2": (2, 64, 48)})
    assert shared["B1"] == shared["B2"] and shared["A2"] != shared["B1"]
    assert random.getstate() == state


def test_level_zero_draws_nothing():
    from cta_gan_amd.trainer.augment import NoiseAugmenter
    aug = NoiseAugmenter(0, 64)
    assert aug.affine is None and aug.level == 0
    batch = {"meta": 1}
    assert aug(batch) is batch


def test_unsupported_modes_raise():
    from cta_gan_amd.trainer.augment import RandomAffine
    with pytest.raises(NotImplementedError):
        RandomAffine(1, shear=5)
    with pytest.raises(NotImplementedError):
        RandomAffine(1, resample=2)
    RandomAffine(1, shear=None, resample=False)
    import trainer.augment as shim
    assert shim.RandomAffine is RandomAffine
