"""What the `noise_level` augmentation costs (LAB_NOTES: "Device-side RandomAffine").

    python scripts/affine_bench.py kernels      # one ctg_hu_affine_inputs launch vs ctg_hu_to_inputs + ctg_resize_nearest x 2
    python scripts/affine_bench.py train        # ms/step of Hd_Trainer_x2.train(loader) at noise_level 0 and 1, alternated

`kernels`: B = 16 raw 512 x 512 HU planes -> 512 x 512 images; device events around back-to-back launches (so the figure holds
the launch gap where the kernel is shorter than it) -- under `rocprofv3 --kernel-trace --stats` the trace gives the kernel
times themselves.  `train`: B = 16, 512 x 512, bf16, host batches through the prefetcher; noise_level 0 takes the code path
of a config without the key (no transform).  Both print the build digest."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _digest():
    from cta_gan_amd import build
    return build._digest()[:16]


def kernels(reps=200):
    from cta_gan_amd import ops
    from cta_gan_amd.trainer.augment import NoiseAugmenter, _upload
    b, s = 16, 512
    g = torch.Generator().manual_seed(0)
    hu = torch.randint(-1100, 1500, (b, 1, s, s), generator=g, dtype=torch.int16).cuda()
    coef = NoiseAugmenter(1, s, seed=0).sample({"A1": (b, s, s), "A2": (b, s, s)})
    table = _upload([row for i in range(b) for row in (coef["A1"][i], coef["A2"][i])], hu.device)

    def fused():
        return ops.hu_affine_inputs(hu, table, (s, s))

    def plain():
        win, full = ops.hu_to_inputs(hu)
        return ops.resize_nearest(win, (s, s)), ops.resize_nearest(full, (s, s))

    def convert_only():
        return ops.hu_to_inputs(hu)

    out = {}
    for name, fn in (("hu_affine_inputs (1 launch)", fused), ("hu_to_inputs + 2 x resize_nearest (3 launches)", plain),
                     ("hu_to_inputs (1 launch)", convert_only)):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        best = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            best.append(e0.elapsed_time(e1) * 1e3 / reps)
        out[name] = best
        print("%-50s us per call, 5 windows of %d: %s" % (name, reps, " ".join("%.1f" % v for v in best)), flush=True)
    print("bytes: fused reads %.1f MB HU, writes %.1f MB" % (hu.numel() * 2 / 1e6, 2 * hu.numel() * 4 / 1e6))
    return out


def train(steps=20, rounds=3):
    from cta_gan_amd import nets, synth
    from cta_gan_amd.trainer import Hd_Trainer_x2
    nets.set_default_compute_dtype(torch.bfloat16)
    b, s = 16, 512
    host = [{k: synth.synth_smooth_images("ab%d_%s" % (i, k), b, s) for k in ("A2", "B1", "B2")} for i in range(4)]

    def make(level):
        cfg = dict(input_nc=1, output_nc=1, size=s, batchSize=b, lr=1e-4, lrd=1e-4, Adv_lamda1=1, Corr_lamda1=20, Corr_lamda2=2,
                   Smooth_lamda=10, epoch=0, n_epochs=1, decay_epoch=0, noise_level=level, seed=0)
        tr = Hd_Trainer_x2(cfg)
        tr.train([dict(x) for x in host])          # warm-up epoch
        torch.cuda.synchronize()
        return tr

    trainers = {0: make(0), 1: make(1)}
    for r in range(rounds):
        for level, tr in trainers.items():
            loader = [dict(host[i % 4]) for i in range(steps)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train(loader)
            torch.cuda.synchronize()
            print("round %d noise_level %d: %.2f ms/step over %d steps" % (r, level, (time.perf_counter() - t0) * 1e3 / steps, steps),
                  flush=True)


if __name__ == "__main__":
    print("build digest", _digest(), flush=True)
    {"kernels": kernels, "train": train}[sys.argv[1]]()
