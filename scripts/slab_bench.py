"""What the sliding thin-slab projections cost (LAB_NOTES: "Sliding thin slabs").

    python scripts/slab_bench.py kernels [REPS]     # the two new entry points on one chunk, next to ctg_project_accumulate
    python scripts/slab_bench.py series             # SeriesTranslator on a 256-slice 512 x 512 volume, slabs=... against slabs=None

`kernels`: a chunk of 16 x 512 x 512 int16 of a 256-slice volume, (thick, step) = (10, 5) and (10, 1), max, values and level:
`ctg_project_slabs_inplane` along y (coronal) and along x (sagittal), `ctg_project_accumulate_sliding`, and
`ctg_project_accumulate` (axial alone, thick 10, and all three axes) on the same chunk.  Device events around back-to-back
calls, the legs alternating inside every round; the chunk stays cache-resident between the calls, as it is behind
`ctg_export_slices` in the product.  These kernels are shorter than the gap between two launches from Python (about 10 us), so
the event figure is that gap: the kernel times come from the same run under `rocprofv3 --kernel-trace` (a small REPS is enough),
summed per (kernel, grid) by `scripts/trace_summary.py` -- every leg has a grid of its own.  The bytes of a leg are what it
must move: the chunk once plus every output byte once (in-plane), the chunk once plus the int32 planes of the slabs it meets
read and written (axial).  `series`: batch 16, bf16, host volume in pageable memory, the two translators alternating inside
every round.  Both print the build digest."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _digest():
    from cta_gan_amd import build
    return build._digest()[:16]


def kernels(reps=200, rounds=5, k=16, s=512, n=256, n0=112):
    from cta_gan_amd import ops
    vol = torch.randint(0, 4096, (k, s, s), generator=torch.Generator().manual_seed(0), dtype=torch.int16).cuda()
    chunk = vol.numel() * 2
    legs = []
    for thick, step in ((10, 5), (10, 1)):
        for axis in ("coronal", "sagittal"):
            j = ops.slab_count(s, thick, step)
            values = torch.empty((j, n, s), dtype=torch.int16, device="cuda")
            level = torch.empty((j, n, s), dtype=torch.uint8, device="cuda")
            legs.append(("inplane %-8s T=%d S=%d (J=%d)" % (axis, thick, step, j), chunk + 3 * j * k * s,
                         lambda a=axis, t=thick, st=step, v=values, lv=level:
                         ops.project_slabs_inplane(vol, n0, a, t, st, "max", values=v, level=lv)))
        j = ops.slab_count(n, thick, step)
        acc = torch.full((j, s, s), -32768, dtype=torch.int32, device="cuda")
        met = len([i for i in range(j) if i * step < n0 + k and i * step + thick > n0])
        legs.append(("axial sliding   T=%d S=%d (%d slabs met)" % (thick, step, met), chunk + 8 * met * s * s,
                     lambda t=thick, st=step, a=acc: ops.project_accumulate_sliding(vol, n0, n, t, st, "max", a)))
    old = {"axial": torch.full(((n + 9) // 10, s, s), -32768, dtype=torch.int32, device="cuda"),
           "coronal": torch.full((n, s), -32768, dtype=torch.int32, device="cuda"),
           "sagittal": torch.full((n, s), -32768, dtype=torch.int32, device="cuda")}
    met = (n0 + k - 1) // 10 - n0 // 10 + 1
    legs.append(("project_accumulate axial thick=10", chunk + 8 * met * s * s,
                 lambda: ops.project_accumulate(vol, n0, 10, "max", axial=old["axial"])))
    legs.append(("project_accumulate three axes", 2 * chunk + 8 * met * s * s,
                 lambda: ops.project_accumulate(vol, n0, 10, "max", **old)))
    for _, _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in legs}
    for _ in range(rounds):
        for name, _, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    for name, nbytes, _ in legs:
        v = times[name]
        print("%-44s us per call, %d windows: %s | best %.1f us, %.2f MB, %.0f GB/s"
              % (name, rounds, " ".join("%.1f" % x for x in v), min(v), nbytes / 1e6, nbytes / min(v) / 1e3), flush=True)


def series(n=256, s=512, batch=16, rounds=4):
    import numpy as np
    from cta_gan_amd import nets, synth
    from cta_gan_amd.Model.HdGan import Generator
    from cta_gan_amd.infer import SeriesTranslator
    vol = np.random.RandomState(0).randint(-1100, 3000, size=(n, s, s)).astype(np.int16)
    nets.set_default_compute_dtype(torch.bfloat16)
    g = synth.fill_module(Generator(1, 1), seed=0).cuda()
    legs = (("slabs=None", SeriesTranslator(g, batch=batch)),
            ("slabs 10/5", SeriesTranslator(g, batch=batch, slabs={"thick": 10, "step": 5})))
    for _, tr in legs:
        tr(vol[:2 * batch])
    torch.cuda.synchronize()
    rates = {name: [] for name, _ in legs}
    for r in range(rounds):
        for name, tr in legs:
            t0 = time.perf_counter()
            tr(vol)
            torch.cuda.synchronize()
            rates[name].append(n / (time.perf_counter() - t0))
            print("bf16 round %d %-10s %.1f slices/s; host ms of the call: %s"
                  % (r, name, rates[name][-1], " ".join("%s %.1f" % (k, v * 1e3) for k, v in tr.stats.items())), flush=True)
    for name, v in rates.items():
        print("%-10s slices/s: %s  (spread %.1f %%)" % (name, " ".join("%.1f" % x for x in v), 100 * (max(v) - min(v)) / max(v)), flush=True)
    a, b = rates[legs[0][0]], rates[legs[1][0]]
    print("slabs 10/5 / slabs=None, median of the rounds: %.3f" % (sorted(b)[len(b) // 2] / sorted(a)[len(a) // 2]), flush=True)
    nets.set_default_compute_dtype(torch.float32)


if __name__ == "__main__":
    print("build digest", _digest(), flush=True)
    if sys.argv[1] == "kernels":
        kernels(*[int(v) for v in sys.argv[2:3]])
    else:
        series()
