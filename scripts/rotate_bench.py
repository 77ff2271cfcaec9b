"""What the rotating projection costs (LAB_NOTES: "Rotating projections").

    python scripts/rotate_bench.py kernel      # one ctg_project_rotate launch vs the stock-torch composition, same tensors
    python scripts/rotate_bench.py series      # SeriesTranslator on a 256-slice 512 x 512 volume, rotate=36 against rotate=None
    ... [--sampling nearest|bilinear] [--oversample S] [--reps N]      # the rays of either leg (default: nearest, unit steps)
    python scripts/rotate_bench.py kernel --depth [--cue C]      # + one ctg_project_rotate_depth launch (all four planes) beside it
    python scripts/rotate_bench.py kernel --render               # + two ctg_project_render launches (rgb, opacity, depth) beside it

`kernel`: a chunk of 16 x 512 x 512 int16, A = 36 view angles, D = 725, max, values and level.  The composition gathers
`vol[:, yi, xi]` by the same integer tables (precomputed on the device, outside the timed window, as one linear index and one
mask per angle), masks, takes `amax` over the ray and fills the empty rays: the values only, bit-equal (checked first); it
materialises a [K, U, T] tensor per angle.  Device events around back-to-back calls, alternating the two.  With --sampling
bilinear there is no composition to compare with: the launch is timed alone.  `series`: batch 16,
bf16, host volume in pageable memory, the two translators alternating inside every round.  Both print the build digest.
--depth adds the depth launch (values, level, depth, cued) as a third leg of the same alternation, after checking that its values
and levels are the plain launch's.
--render adds two ctg_project_render launches (rgb, opacity, depth) on the same chunk, angles and sampling to the alternation: the
"vessels" preset in its default window with stop 128 -- on this random chunk most rays meet an opaque class within a few steps and
end -- and a thin fog (every alpha 64 of 32768, stop 0) that no ray ever leaves early: the full-length cost of the ordered fold."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _digest():
    from cta_gan_amd import build
    return build._digest()[:16]


def kernel(reps=50, torch_reps=3, rounds=5, k=16, s=512, count=36, sampling="nearest", oversample=1, depth=False, cue=128,
           render=False):
    from cta_gan_amd import ops
    from cta_gan_amd.infer import TRANSFER_PRESETS, default_detector, rotation_coefficients, transfer_function, view_angles
    d = default_detector(s, s)
    steps = d * oversample
    angles = view_angles(count)
    coef = [rotation_coefficients(a, s, s, oversample=oversample) for a in angles]
    table = ops.RotateTable(coef)
    vol = torch.randint(0, 4096, (k, s, s), generator=torch.Generator().manual_seed(0), dtype=torch.int16).cuda()
    values = torch.empty((count, k, d), dtype=torch.int16, device="cuda")
    level = torch.empty((count, k, d), dtype=torch.uint8, device="cuda")
    u = torch.arange(d, dtype=torch.int64, device="cuda")[:, None]
    t = torch.arange(steps, dtype=torch.int64, device="cuda")[None, :]
    index = []
    for c in coef if sampling == "nearest" else ():
        xi, yi = (c[0] + c[1] * u + c[2] * t) >> 16, (c[3] + c[4] * u + c[5] * t) >> 16
        ok = (xi >= 0) & (xi < s) & (yi >= 0) & (yi < s)
        index.append((torch.where(ok, yi * s + xi, 0).reshape(-1), ok[None], ok.any(dim=1)[None]))
    flat = vol.view(k, s * s)
    lowest = torch.tensor(-32768, dtype=torch.int16, device="cuda")
    air = torch.tensor(0, dtype=torch.int16, device="cuda")

    def fused():
        ops.project_rotate(vol, 0, table, steps, "max", values=values, level=level, sampling=sampling)
        return values

    def composed():
        out = []
        for lin, ok, seen in index:
            g = flat.index_select(1, lin).view(k, d, steps)
            out.append(torch.where(seen, torch.where(ok, g, lowest).amax(dim=2), air))
        return torch.stack(out)

    planes = {"values": torch.empty_like(values), "level": torch.empty_like(level), "depth": torch.empty_like(values),
              "cued": torch.empty_like(level)} if depth else None

    def with_depth():
        ops.project_rotate_depth(vol, 0, table, steps, "max", cue=cue, sampling=sampling, **planes)

    frames = {"rgb": torch.empty((count, k, d, 3), dtype=torch.uint8, device="cuda"), "opacity": torch.empty_like(level),
              "depth": torch.empty_like(values)} if render else None
    if render:
        import numpy as np
        preset = ops.TransferTable(transfer_function(TRANSFER_PRESETS["vessels"], oversample))
        thin = np.zeros((256, 4), dtype=np.uint16)
        thin[:, :3], thin[:, 3] = np.arange(256)[:, None], 64
        thin = ops.TransferTable(thin)

    def render_preset():
        ops.project_render(vol, 0, table, steps, preset, wc=300.0, ww=1500.0, stop=128, sampling=sampling, **frames)

    def render_fog():
        ops.project_render(vol, 0, table, steps, thin, wc=300.0, ww=1500.0, stop=0, sampling=sampling, **frames)

    print("sampling %s, %d step(s) per voxel: %d steps per ray" % (sampling, oversample, steps), flush=True)
    fns = (("project_rotate (1 launch)", fused, reps),)
    if render:
        fns += (("project_render, vessels", render_preset, reps), ("project_render, thin fog", render_fog, reps))
    if depth:
        fused()
        with_depth()
        print("depth launch: same values %s, same level %s" % (torch.equal(planes["values"], values), torch.equal(planes["level"], level)),
              flush=True)
        fns += (("project_rotate_depth (1 launch)", with_depth, reps),)
    if sampling == "nearest":
        print("same values: %s" % torch.equal(fused(), composed()), flush=True)
        fns += (("torch composition", composed, torch_reps),)
    for _, fn, _ in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in fns}
    for _ in range(rounds):
        for name, fn, n in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / n)
    for name, v in times.items():
        print("%-28s us per call, %d windows: %s" % (name, rounds, " ".join("%.1f" % x for x in v)), flush=True)
    best = min(times["project_rotate (1 launch)"])
    samples = count * k * d * steps
    print("project_rotate: %.1f us best window, %.1f G samples/s over %d samples" % (best, samples / best / 1e3, samples), flush=True)
    if depth:
        other = min(times["project_rotate_depth (1 launch)"])
        print("project_rotate_depth (cue %d, four planes) %.1f us best window: %.3f x the plain launch" % (cue, other, other / best),
              flush=True)
    if render:
        for name in ("project_render, vessels", "project_render, thin fog"):
            other = min(times[name])
            print("%s (rgb, opacity, depth) %.1f us best window: %.3f x the plain launch" % (name, other, other / best), flush=True)
    if sampling == "nearest":
        other = min(times["torch composition"])
        print("torch composition %.1f us: %.1f x" % (other, other / best), flush=True)


def series(n=256, s=512, batch=16, rounds=4, count=36, sampling="nearest", oversample=1):
    import numpy as np
    from cta_gan_amd import nets, synth
    from cta_gan_amd.Model.HdGan import Generator
    from cta_gan_amd.infer import SeriesTranslator
    vol = np.random.RandomState(0).randint(-1100, 3000, size=(n, s, s)).astype(np.int16)
    nets.set_default_compute_dtype(torch.bfloat16)
    g = synth.fill_module(Generator(1, 1), seed=0).cuda()
    print("sampling %s, %d step(s) per voxel" % (sampling, oversample), flush=True)
    legs = (("rotate=None", SeriesTranslator(g, batch=batch)),
            ("rotate=%d" % count, SeriesTranslator(g, batch=batch, rotate=count, rotate_sampling=sampling, rotate_oversample=oversample)))
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
    print("rotate=%d / rotate=None, median of the rounds: %.3f" % (count, sorted(b)[len(b) // 2] / sorted(a)[len(a) // 2]), flush=True)
    nets.set_default_compute_dtype(torch.float32)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["kernel", "series"])
    ap.add_argument("--sampling", choices=["nearest", "bilinear"], default="nearest")
    ap.add_argument("--oversample", type=int, default=1)
    ap.add_argument("--reps", type=int, default=None, help="kernel: calls per timed window (default 50)")
    ap.add_argument("--depth", action="store_true", help="kernel: also time ctg_project_rotate_depth on the same chunk")
    ap.add_argument("--cue", type=int, default=128, help="kernel: the depth cue of the --depth leg")
    ap.add_argument("--render", action="store_true", help="kernel: also time ctg_project_render on the same chunk")
    o = ap.parse_args()
    print("build digest", _digest(), flush=True)
    if o.leg == "kernel":
        kernel(sampling=o.sampling, oversample=o.oversample, depth=o.depth, cue=o.cue, render=o.render, **({} if o.reps is None else {"reps": o.reps}))
    else:
        series(sampling=o.sampling, oversample=o.oversample)
