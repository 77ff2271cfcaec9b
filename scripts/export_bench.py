"""What the series export costs (LAB_NOTES: "Series inference").

    python scripts/export_bench.py kernels      # one ctg_export_slices launch vs the stock-torch composition, same tensors
    python scripts/export_bench.py series       # SeriesTranslator on a 256-slice 512 x 512 volume vs the generator forward alone

`kernels`: B = 16 generator-range 512 x 512 planes, equal sizes, both outputs (4 B read + 3 B written per pixel); the composition
is `((x + 1) * 0.5 * 4095).to(torch.int16)` plus `ops.to_windowdata` and a uint8 cast.  Device events around back-to-back
launches, alternating the two; both results are compared first.  `series`: batch = 16, bf16 and bf16x3, host volume in pageable
memory; the forward alone runs no-grad on a resident batch of the same size in the same mode.  Both print the build digest."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _digest():
    from cta_gan_amd import build
    return build._digest()[:16]


def kernels(reps=200, rounds=5):
    from cta_gan_amd import ops
    b, s = 16, 512
    x = (torch.rand((b, 1, s, s), generator=torch.Generator().manual_seed(0)) * 2 - 1).cuda()
    wc = torch.full((b,), 50.0, device="cuda")
    ww = torch.full((b,), 400.0, device="cuda")

    def fused():
        return ops.export_slices(x, wc, ww)

    def composed():
        pix = ((x + 1) * 0.5 * 4095).to(torch.int16)
        level = ((ops.to_windowdata(x, wc, ww) + 1) * 127.5).round().to(torch.uint8)
        return pix, level

    def series_in():
        return ops.series_inputs(hu, (s, s))

    hu = torch.randint(-1100, 3000, (b, s, s), generator=torch.Generator().manual_seed(1), dtype=torch.int16).cuda()
    (p0, l0), (p1, l1) = fused(), composed()
    print("same results: pix %s level %s" % (torch.equal(p0, p1.reshape(p0.shape)), torch.equal(l0, l1.reshape(l0.shape))), flush=True)
    fns = (("export_slices (1 launch)", fused), ("torch composition", composed), ("series_inputs (1 launch)", series_in))
    for _, fn in fns:
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in fns}
    for _ in range(rounds):
        for name, fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    npix = b * s * s
    for name, v in times.items():
        print("%-28s us per call, %d windows of %d: %s" % (name, rounds, reps, " ".join("%.1f" % t for t in v)), flush=True)
    best = min(times["export_slices (1 launch)"])
    print("export_slices: %.1f us best window, %.2f TB/s over its 7 B/pixel (%.1f MB)" % (best, 7 * npix / best / 1e6, 7 * npix / 1e6))
    best = min(times["series_inputs (1 launch)"])
    print("series_inputs: %.1f us best window, %.2f TB/s over its 6 B/pixel" % (best, 6 * npix / best / 1e6))


def series(n=256, s=512, batch=16, rounds=3):
    import numpy as np
    from cta_gan_amd import nets, synth
    from cta_gan_amd.Model.HdGan import Generator
    from cta_gan_amd.infer import SeriesTranslator
    vol = np.random.RandomState(0).randint(-1100, 3000, size=(n, s, s)).astype(np.int16)
    for mode in ("bf16", "bf16x3"):
        nets.set_default_compute_dtype(torch.bfloat16 if mode == "bf16" else mode)
        g = synth.fill_module(Generator(1, 1), seed=0).cuda()
        tr = SeriesTranslator(g, batch=batch)
        x = synth.synth_smooth_images("bench_series", batch, s).cuda()
        with torch.no_grad():
            for _ in range(3):
                g(x)
        tr(vol[:2 * batch])
        torch.cuda.synchronize()
        for r in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.no_grad():
                e0.record()
                for _ in range(n // batch):
                    g(x)
                e1.record()
            torch.cuda.synchronize()
            fwd = n / (e0.elapsed_time(e1) / 1e3)
            t0 = time.perf_counter()
            tr(vol)
            torch.cuda.synchronize()
            ser = n / (time.perf_counter() - t0)
            print("%s round %d: forward alone %.1f slices/s, SeriesTranslator %.1f slices/s, ratio %.3f; host ms of the call: %s"
                  % (mode, r, fwd, ser, ser / fwd, " ".join("%s %.1f" % (k, v * 1e3) for k, v in tr.stats.items())), flush=True)
    nets.set_default_compute_dtype(torch.float32)


if __name__ == "__main__":
    print("build digest", _digest(), flush=True)
    {"kernels": kernels, "series": series}[sys.argv[1]]()
