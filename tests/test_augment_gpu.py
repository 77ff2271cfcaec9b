"""GPU: the `noise_level` augmentation -- csrc/augment.hip (`ops.affine_nearest`, `ops.hu_affine_inputs`) against PIL's output
(tests/golden/affine_*.npz) and the numpy restatement (tests/affine_np.py), `NoiseAugmenter`, the prefetcher's `transform`
and the trainers' wiring.  Every comparison is bitwise over every element."""
import glob
import os

import numpy as np
import pytest
import torch

import affine_np as anp

pytestmark = pytest.mark.gpu

FILL = -1.0
SIZES = [(5, 7), (37, 53), (64, 48)]
OUT_SIZES = [None, (64, 64), (24, 40), (77, 131)]      # None: the input's own size; up, down, odd width
_LEVEL5 = {(5, 7): "5x7_l5", (37, 53): "37x53_l5", (64, 48): "64x48_l5"}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _coef_of(h, w, angle, tx, ty, scale):
    from cta_gan_amd.trainer.augment import fixed_coefficients, inverse_matrix
    return fixed_coefficients(inverse_matrix((w * 0.5, h * 0.5), angle, (tx, ty), scale), (h, w))


def _planes(golden_dir, h, w):
    """kind -> (image, coefficients) for an h x w source.  'fixture': PIL's own case at level 5; 'allfill': translated by the
    whole width, every pixel is fill; 'tiny': angle 0.3, scale 1, no translation (nearly every pixel reads itself); 'rand1/2':
    strong random parameters with a translation of at least one pixel; 'zoom': magnified, no pixel leaves the source."""
    z = np.load(os.path.join(golden_dir, "affine_%s.npz" % _LEVEL5[(h, w)]))
    rng = np.random.RandomState(1000 * h + w)
    img = lambda: rng.rand(h, w).astype(np.float32) * 1.9 - 0.9      # noqa: E731  (never equal to the fill)
    planes = {"fixture": (z["img"], [int(v) for v in z["coef"]]),
              "allfill": (img(), _coef_of(h, w, 0.3, -w if (h + w) % 2 else w, 0, 1.0)),
              "tiny": (img(), _coef_of(h, w, 0.3, 0, 0, 1.0)),
              "zoom": (img(), _coef_of(h, w, 2.0, 1, -1, 1.5))}
    for name in ("rand1", "rand2"):
        sx, sy = rng.choice([-1, 1], 2)
        planes[name] = (img(), _coef_of(h, w, rng.uniform(-15, 15), int(sx * rng.randint(1, 4)), int(sy * rng.randint(1, 4)),
                                        rng.uniform(0.85, 1.15)))
    return planes


def _run(imgs, coefs, size):
    from cta_gan_amd import ops
    x = torch.from_numpy(np.stack(imgs)).cuda()
    c = torch.tensor(coefs, dtype=torch.int32).cuda()
    return ops.affine_nearest(x, c, size, FILL)


def _expected(imgs, coefs, size):
    return torch.from_numpy(np.stack([anp.affine_resize(i, c, FILL, size) for i, c in zip(imgs, coefs)]))


@pytest.mark.parametrize("h,w", SIZES)
def test_affine_nearest_single_planes_match_pil_and_numpy(golden_dir, h, w):
    """N = 1, every plane kind, every output size.  Input conditions asserted from the numpy side: the all-fill plane is all
    fill, the zoom plane has none, the strong planes move more than half of their pixels and one of them leaves > 5 % fill."""
    planes = _planes(golden_dir, h, w)
    fill_share = {k: float((anp.pil_affine_fixed(i, c, FILL) == FILL).mean()) for k, (i, c) in planes.items()}
    assert fill_share["allfill"] == 1.0 and fill_share["zoom"] == 0.0
    assert max(fill_share["rand1"], fill_share["rand2"]) > 0.05
    for k in ("rand1", "rand2", "zoom"):
        assert anp.moved_share(planes[k][1], h, w) > 0.5, k
    for kind, (img, coef) in planes.items():
        for size in OUT_SIZES:
            size = size or (h, w)
            got = _run([img], [coef], size)
            assert got.shape == (1,) + tuple(size)
            assert torch.equal(got.cpu(), _expected([img], [coef], size)), (kind, size)
    # PIL's own pixels, every fixture of this size (all levels)
    for f in sorted(glob.glob(os.path.join(golden_dir, "affine_%dx%d_*.npz" % (h, w)))):
        z = np.load(f)
        assert torch.equal(_run([z["img"]], [z["coef"].tolist()], (h, w)).cpu(), torch.from_numpy(z["out"])[None]), f


def test_affine_nearest_matches_the_128x96_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "affine_128x96_l5.npz"))
    assert torch.equal(_run([z["img"]], [z["coef"].tolist()], (128, 96)).cpu(), torch.from_numpy(z["out"])[None])


@pytest.mark.parametrize("h,w", SIZES)
def test_affine_nearest_five_planes_with_distinct_coefficients(golden_dir, h, w):
    """N = 5 (more than one workgroup per launch, per-plane coefficients): fixture, all-fill, tiny-angle, strong and zoom plane in
    one launch; the fused resize equals `resize_nearest` of the same-size warp bit for bit."""
    from cta_gan_amd import ops
    planes = _planes(golden_dir, h, w)
    kinds = ["fixture", "allfill", "tiny", "rand1", "zoom"]
    imgs, coefs = [planes[k][0] for k in kinds], [planes[k][1] for k in kinds]
    assert len({tuple(c) for c in coefs}) == 5
    exp_same = _expected(imgs, coefs, (h, w))
    assert float((exp_same == FILL).float().mean()) > 0.05
    assert np.mean([anp.moved_share(c, h, w) for c in coefs]) > 0.5
    same = _run(imgs, coefs, (h, w))
    assert torch.equal(same.cpu(), exp_same)
    for size in OUT_SIZES[1:]:
        got = _run(imgs, coefs, size)
        assert torch.equal(got.cpu(), _expected(imgs, coefs, size)), size
        assert torch.equal(got, ops.resize_nearest(same, size)), size          # composition
    # a (B, 1, H, W) view keeps its leading axes, and an unaligned destination row start takes the scalar head (odd width above)
    x4 = torch.from_numpy(np.stack(imgs)).cuda()[:, None]
    out4 = ops.affine_nearest(x4, torch.tensor(coefs, dtype=torch.int32).cuda(), (h, w), FILL)
    assert out4.shape == (5, 1, h, w) and torch.equal(out4[:, 0], same)


def test_hu_affine_inputs_matches_the_fixture_and_the_three_kernel_composition(golden_dir):
    from cta_gan_amd import ops
    (f,) = glob.glob(os.path.join(golden_dir, "affine_hu_*.npz"))
    z = np.load(f)
    hu = torch.from_numpy(z["hu"]).cuda()
    coef = torch.from_numpy(z["coef"].astype(np.int32)).cuda()             # (2, 6): windowed, full-range
    win, full = ops.hu_affine_inputs(hu[None], coef[None], hu.shape, 50.0, 400.0, FILL)
    assert torch.equal(win[0].cpu(), torch.from_numpy(z["win"])) and torch.equal(full[0].cpu(), torch.from_numpy(z["full"]))
    # random HU, B = 3, 64x48 -> 40x40: hu_to_inputs -> affine_nearest -> resize_nearest of the existing kernels
    rng = np.random.RandomState(3)
    h, w, b = 64, 48, 3
    hu = torch.from_numpy(rng.randint(-1100, 1500, size=(b, h, w)).astype(np.int16)).cuda()
    table = [[_coef_of(h, w, rng.uniform(-8, 8), int(rng.randint(-3, 4)), int(rng.randint(-3, 4)), rng.uniform(0.9, 1.1))
              for _ in range(2)] for _ in range(b)]
    coef = torch.tensor(table, dtype=torch.int32).cuda()
    win, full = ops.hu_affine_inputs(hu, coef, (40, 40), 50.0, 400.0, FILL)
    w0, f0 = ops.hu_to_inputs(hu, 50.0, 400.0)
    for got, plain, q in ((win, w0, 0), (full, f0, 1)):
        ref = ops.resize_nearest(ops.affine_nearest(plain, coef[:, q].contiguous(), (h, w), FILL), (40, 40))
        assert got.shape == (b, 40, 40) and torch.equal(got, ref), q
        assert 0.0 < float((got == FILL).float().mean()) < 0.9
    # another window reaches the kernel
    win2, full2 = ops.hu_affine_inputs(hu, coef, (40, 40), 300.0, 1500.0, FILL)
    assert not torch.equal(win2, win) and torch.equal(full2, full)


def test_bad_input_raises():
    from cta_gan_amd import ops
    x = torch.zeros(2, 5, 7)
    coef = torch.zeros(2, 6, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.affine_nearest(x, coef.cuda(), (5, 7), FILL)
    with pytest.raises(RuntimeError):
        ops.affine_nearest(x.cuda(), coef, (5, 7), FILL)
    with pytest.raises(RuntimeError):
        ops.hu_affine_inputs(torch.zeros(2, 5, 7, dtype=torch.int16), torch.zeros(2, 2, 6, dtype=torch.int32).cuda(), (5, 7), 50.0, 400.0, FILL)
    for size in ((0, 7), (5, -1), (32769, 7)):
        with pytest.raises(RuntimeError, match="CTG_EINVAL"):
            ops.affine_nearest(x.cuda(), coef.cuda(), size, FILL)
        with pytest.raises(RuntimeError, match="CTG_EINVAL"):
            ops.hu_affine_inputs(x.cuda().short(), torch.zeros(2, 2, 6, dtype=torch.int32).cuda(), size, 50.0, 400.0, FILL)
    with pytest.raises(RuntimeError, match="CTG_EINVAL"):
        ops.hu_affine_inputs(x.cuda().short(), torch.zeros(2, 2, 6, dtype=torch.int32).cuda(), (5, 7), 50.0, 0.0, FILL)
    with pytest.raises(RuntimeError):          # one row of coefficients too few
        ops.affine_nearest(x.cuda(), coef[:1].cuda(), (5, 7), FILL)


def _host_batch(seed, b=2, keys=(("A2", 64, 48), ("B1", 37, 53), ("B2", 64, 48))):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.rand(b, 1, h, w, generator=g) * 1.9 - 0.9 for k, h, w in keys}


def test_noise_augmenter_level_zero_seeds_and_series():
    from cta_gan_amd.trainer.augment import NoiseAugmenter
    dev = {k: v.cuda() for k, v in _host_batch(1, keys=(("A2", 40, 40), ("B1", 40, 40), ("B2", 40, 40))).items()}
    out = NoiseAugmenter(0, 40)(dev)
    assert all(out[k] is dev[k] for k in dev)                                # the very tensors
    out = NoiseAugmenter(0, 24)(dev)
    assert out["A2"].shape == (2, 1, 24, 24) and out["A2"].is_cuda
    batch = {k: v.cuda() for k, v in _host_batch(2).items()}
    a, b = NoiseAugmenter(2, 40, seed=5)(batch), NoiseAugmenter(2, 40, seed=5)(batch)
    c = NoiseAugmenter(2, 40, seed=6)(batch)
    for k in batch:
        assert a[k].shape == (2, 1, 40, 40) and a[k].dtype == torch.float32
        assert torch.equal(a[k], b[k]) and not torch.equal(a[k], c[k]), k
    # grouping by source size, stacking and splitting keep every plane with its own draw: against numpy, plane by plane
    coef = NoiseAugmenter(2, 40, seed=5).sample({k: (v.shape[0], v.shape[2], v.shape[3]) for k, v in batch.items()})
    for k, v in batch.items():
        exp = _expected(list(v[:, 0].cpu().numpy()), coef[k], (40, 40))
        assert torch.equal(a[k][:, 0].cpu(), exp), k
    # the two images of one series: independent draws by default (the reference's loaders), one draw with shared_per_series
    x = batch["B2"]
    two = {"B1": x, "B2": x}
    out = NoiseAugmenter(5, 64, seed=1)(two)
    assert all(not torch.equal(out["B1"][i], out["B2"][i]) for i in range(2))
    out = NoiseAugmenter(5, 64, seed=1, shared_per_series=True)(two)
    assert torch.equal(out["B1"], out["B2"]) and not torch.equal(out["B1"][0], out["B1"][1])


def test_noise_augmenter_raw_hu_batches():
    from cta_gan_amd import ops
    from cta_gan_amd.trainer.augment import NoiseAugmenter
    rng = np.random.RandomState(9)
    hu_a = torch.from_numpy(rng.randint(-1100, 1500, size=(2, 1, 64, 48)).astype(np.int16)).cuda()
    hu_b = torch.from_numpy(rng.randint(-1100, 1500, size=(2, 1, 64, 48)).astype(np.int16)).cuda()
    out = NoiseAugmenter(2, 40, seed=3)({"hu_A": hu_a, "hu_B": hu_b, "meta": 7})
    assert sorted(out) == ["A1", "A2", "B1", "B2", "meta"] and out["meta"] == 7
    a1, a2 = ops.hu_to_inputs(hu_a)
    b1, b2 = ops.hu_to_inputs(hu_b)
    ref = NoiseAugmenter(2, 40, seed=3)({"A1": a1, "A2": a2, "B1": b1, "B2": b2})
    for k in ("A1", "A2", "B1", "B2"):
        assert out[k].shape == (2, 1, 40, 40) and torch.equal(out[k], ref[k]), k
    plain = NoiseAugmenter(0, 64)({"hu_A": hu_a})
    assert torch.equal(plain["A1"], ops.resize_nearest(a1, (64, 64))) and torch.equal(plain["A2"], ops.resize_nearest(a2, (64, 64)))


def test_prefetcher_runs_the_transform_on_the_copy_stream_between_its_events():
    from cta_gan_amd.Model.HdGan import DataPrefetcher
    from cta_gan_amd.trainer.augment import NoiseAugmenter
    src = [_host_batch(10 + i) for i in range(3)]
    aug = NoiseAugmenter(2, 40, seed=5)
    seen = []

    def transform(batch):
        out = aug(batch)
        mid = torch.cuda.Event(enable_timing=True)
        mid.record()                                  # on the stream the transform's launches went to
        seen.append((torch.cuda.current_stream(), mid))
        return out

    pf = DataPrefetcher([dict(b) for b in src], transform=transform)
    got, events = [], []
    while True:
        events.append(pf.copy_events)                # of the batch that next() is about to hand out
        batch = pf.next()
        if batch is None:
            break
        got.append(batch)
    torch.cuda.synchronize()
    assert len(got) == 3 and len(seen) == 3
    by_hand = NoiseAugmenter(2, 40, seed=5)
    for i, batch in enumerate(got):
        exp = by_hand({k: v.cuda() for k, v in src[i].items()})
        assert all(torch.equal(batch[k], exp[k]) for k in exp), i
        stream, mid = seen[i]
        start, end = events[i]
        assert stream == pf.stream and stream != torch.cuda.current_stream()
        # one stream executes in order: start, copies, gather launches, mid, end
        assert start.elapsed_time(mid) >= 0.0 and mid.elapsed_time(end) >= 0.0
    # default: no transform, batches as before
    plain = DataPrefetcher([dict(src[0])]).next()
    assert all(torch.equal(plain[k].cpu(), src[0][k]) for k in src[0])


def test_trainer_applies_noise_level_to_host_batches_only():
    """`Hd_Trainer_x2.train(loader)` with noise_level 2 == a trainer without augmentation fed the pre-augmented batches, bit for
    bit in the generator's weights; != the raw batches; a config without the key == noise_level 0."""
    from cta_gan_amd import nets, ops, synth
    from cta_gan_amd.trainer import Hd_Trainer_x2
    from cta_gan_amd.trainer.augment import NoiseAugmenter
    from oracle.golden_cases import REG_GAINS
    saved = ops.DETERMINISTIC
    ops.DETERMINISTIC = True
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        raw = [{k: synth.synth_smooth_images("aug%d_%s" % (i, k), 2, 256) for k in ("A2", "B1", "B2")} for i in range(2)]
        pre_aug = NoiseAugmenter(2, 256, seed=5)
        pre = [{k: v.cpu() for k, v in pre_aug({k: v.cuda() for k, v in b.items()}).items()} for b in raw]
        assert not torch.equal(pre[0]["A2"], raw[0]["A2"])

        def run(loader, **over):
            cfg = dict(input_nc=1, output_nc=1, size=256, batchSize=2, lr=1e-4, lrd=1e-4, Adv_lamda1=1, Corr_lamda1=20,
                       Corr_lamda2=2, Smooth_lamda=10, epoch=0, n_epochs=1, decay_epoch=0, **over)
            tr = Hd_Trainer_x2(cfg)
            synth.fill_module(tr.netG_A2B, seed=0)
            synth.fill_module(tr.netD_B, seed=1)
            synth.fill_module(tr.R_A, seed=4, gains=REG_GAINS)
            tr.train([dict(b) for b in loader])
            torch.cuda.synchronize()
            return torch.cat([p.detach().reshape(-1) for p in tr.netG_A2B.parameters()]).clone()

        w_aug = run(raw, noise_level=2, seed=5)
        w_pre = run(pre, noise_level=0)
        w_raw = run(raw, noise_level=0)
        w_nokey = run(raw)
        assert torch.isfinite(w_aug).all()
        assert torch.equal(w_aug, w_pre)
        assert not torch.equal(w_aug, w_raw)
        assert torch.equal(w_nokey, w_raw)
    finally:
        ops.DETERMINISTIC = saved
        nets.set_default_compute_dtype(torch.float32)
