"""What the series projections cost (LAB_NOTES: "Series projections").

    python scripts/project_bench.py kernels     # one ctg_project_accumulate call (all three axes) vs the stock-torch composition
    python scripts/project_bench.py series      # SeriesTranslator on a 256-slice 512 x 512 volume, project="max" vs project=None
    python scripts/project_bench.py kernels --depth      # + ctg_project_accumulate_depth / ctg_project_finish_depth beside the plain calls

`kernels`: a (16, 512, 512) int16 chunk, mode max, whole-volume axial slab; the composition is `torch.amax` over each of the
three dims plus `torch.maximum` into the running axial plane (and the row stores into the coronal / sagittal arrays).  Device
events around back-to-back calls, alternating the two; both results are compared first.  `series`: batch = 16, bf16, host
volume in pageable memory, the two translators alternated in one job: the yardstick is the project=None leg of the same run.
Both print the build digest."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _digest():
    from cta_gan_amd import build
    return build._digest()[:16]


def kernels(reps=200, rounds=5, depth=False):
    from cta_gan_amd import ops
    k, s = 16, 512
    pix = torch.randint(-1024, 3072, (k, s, s), generator=torch.Generator().manual_seed(0), dtype=torch.int16).cuda()
    acc = {"axial": torch.empty((1, s, s), dtype=torch.int32, device="cuda"),
           "coronal": torch.empty((k, s), dtype=torch.int32, device="cuda"),
           "sagittal": torch.empty((k, s), dtype=torch.int32, device="cuda")}
    ref = {"axial": torch.empty((s, s), dtype=torch.int16, device="cuda"),
           "coronal": torch.empty((k, s), dtype=torch.int16, device="cuda"),
           "sagittal": torch.empty((k, s), dtype=torch.int16, device="cuda")}

    def clear():
        for t in acc.values():
            t.fill_(ops.PROJECT_IDENTITY[0])
        ref["axial"].fill_(-32768)

    def fused():
        ops.project_accumulate(pix, 0, k, 0, **acc)

    def composed():
        torch.maximum(ref["axial"], torch.amax(pix, dim=0), out=ref["axial"])
        torch.amax(pix, dim=1, out=ref["coronal"])
        torch.amax(pix, dim=2, out=ref["sagittal"])

    def rows_only():
        ops.project_accumulate(pix, 0, k, 0, axial=acc["axial"], sagittal=acc["sagittal"])

    def coronal_only():
        ops.project_accumulate(pix, 0, k, 0, coronal=acc["coronal"])

    keyed = {a: torch.empty_like(t) for a, t in acc.items()}

    def with_depth():
        ops.project_accumulate_depth(pix, 0, k, 0, **keyed)

    clear()
    fused()
    composed()
    print("same results: %s" % " ".join("%s %s" % (a, torch.equal(acc[a].reshape(ref[a].shape), ref[a].int())) for a in acc), flush=True)
    fns = (("project_accumulate (3 axes)", fused), ("torch composition", composed),
           ("project_accumulate (axial + sagittal)", rows_only),
           ("project_accumulate (coronal)", coronal_only))
    if depth:
        for t in keyed.values():
            t.fill_(ops.PROJECT_DEPTH_IDENTITY[0])
        with_depth()
        extent = {"axial": (k, k), "coronal": (s, s), "sagittal": (s, s)}
        print("depth: same values %s" % " ".join("%s %s" % (a, torch.equal(
            ops.project_finish_depth(keyed[a], 0, *extent[a], want_level=False, want_depth=False, want_cued=False)[0],
            ops.project_finish(acc[a], 0, want_level=False)[0])) for a in acc), flush=True)
        fns += (("project_accumulate_depth (3 axes)", with_depth),)
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
    npix = k * s * s
    for name, v in times.items():
        print("%-40s us per call, %d windows of %d: %s" % (name, rounds, reps, " ".join("%.1f" % t for t in v)), flush=True)
    best, comp = min(times["project_accumulate (3 axes)"]), min(times["torch composition"])
    print("project_accumulate: %.1f us best window, %.2f TB/s over 2 B/pixel (%.1f MB); composition %.1f us: fused is %.2fx"
          % (best, 2 * npix / best / 1e6, 2 * npix / 1e6, comp, comp / best))
    # finish: the three accumulators of a 256-slice volume -> values + levels
    big = {"axial": torch.zeros((1, s, s), dtype=torch.int32, device="cuda"),
           "coronal": torch.zeros((256, s), dtype=torch.int32, device="cuda"),
           "sagittal": torch.zeros((256, s), dtype=torch.int32, device="cuda")}
    for _ in range(5):
        for t in big.values():
            ops.project_finish(t, 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        for t in big.values():
            ops.project_finish(t, 0)
    e1.record()
    torch.cuda.synchronize()
    print("project_finish: %.1f us for the three projections of a 256-slice volume (3 launches, 6 allocations)"
          % (e0.elapsed_time(e1) * 1e3 / reps))
    if depth:
        other = min(times["project_accumulate_depth (3 axes)"])
        print("project_accumulate_depth %.1f us best window: %.3f x the plain call" % (other, other / best))
        extent = {"axial": (256, 256), "coronal": (s, s), "sagittal": (s, s)}
        for _ in range(5):
            for a, t in big.items():
                ops.project_finish_depth(t, 0, *extent[a], cue=128)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            for a, t in big.items():
                ops.project_finish_depth(t, 0, *extent[a], cue=128)
        e1.record()
        torch.cuda.synchronize()
        print("project_finish_depth: %.1f us for the same three accumulators, four planes each (3 launches, 12 allocations)"
              % (e0.elapsed_time(e1) * 1e3 / reps))


def series(n=256, s=512, batch=16, rounds=4):
    import numpy as np
    from cta_gan_amd import nets, synth
    from cta_gan_amd.Model.HdGan import Generator
    from cta_gan_amd.infer import SeriesTranslator
    vol = np.random.RandomState(0).randint(-1100, 3000, size=(n, s, s)).astype(np.int16)
    nets.set_default_compute_dtype(torch.bfloat16)
    g = synth.fill_module(Generator(1, 1), seed=0).cuda()
    legs = (("project=None", SeriesTranslator(g, batch=batch)), ("project=max", SeriesTranslator(g, batch=batch, project="max")))
    for _, tr in legs:
        tr(vol[:2 * batch])
    tr = legs[1][1]
    tr(vol)      # the projector of the full shape exists before the clock starts, as the staging slots do
    torch.cuda.synchronize()
    rate = {name: [] for name, _ in legs}
    for r in range(rounds):
        for name, tr in (legs if r % 2 == 0 else legs[::-1]):
            t0 = time.perf_counter()
            tr(vol)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rate[name].append(n / dt)
            print("round %d %-13s %.1f slices/s (%.1f ms); host ms of the call: %s"
                  % (r, name, n / dt, dt * 1e3, " ".join("%s %.1f" % (k, v * 1e3) for k, v in tr.stats.items())), flush=True)
    a, b = rate["project=None"], rate["project=max"]
    print("project=None best %.1f median %.1f slices/s; project=max best %.1f median %.1f slices/s; ratio of the medians %.4f"
          % (max(a), sorted(a)[len(a) // 2], max(b), sorted(b)[len(b) // 2], sorted(b)[len(b) // 2] / sorted(a)[len(a) // 2]))
    nets.set_default_compute_dtype(torch.float32)


if __name__ == "__main__":
    print("build digest", _digest(), flush=True)
    if sys.argv[1] == "kernels":
        kernels(depth="--depth" in sys.argv[2:])
    else:
        series()
