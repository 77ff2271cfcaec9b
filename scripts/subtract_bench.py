"""What the subtraction volume costs (LAB_NOTES: "Subtraction volume").

    python scripts/subtract_bench.py kernel     # one ctg_subtract_slices launch vs ctg_export_slices and the stock-torch composition
    python scripts/subtract_bench.py series     # SeriesTranslator on a 256-slice 512 x 512 volume, subtract=True vs subtract=False

`kernel`: a (16, 512, 512) chunk, both outputs, median on and off (floor 60, band -900 .. 400); the yardstick is one
`ctg_export_slices` launch on the same shape in the same job (the same 7 bytes per pixel: 4 in, 3 out); the composition forms
the same sub and level from stock torch ops on the same tensors (the median as the sort of nine padded shifts).  Device events
around back-to-back calls, the legs alternated; the results are compared first.  `series`: batch = 16, bf16, host volume in
pageable memory, the two translators alternated in one job: the yardstick is the subtract=False leg of the same run.
Both print the build digest."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

FLOOR, BAND, WINDOW = 60, (-900, 400), (150.0, 300.0)


def _digest():
    from cta_gan_amd import build
    return build._digest()[:16]


def composed(cta, ct, median):
    """The same (sub, level) from stock torch ops: int32 planes, the 3 x 3 median as the sort of nine edge-padded shifts."""
    c = ct.int()
    d = cta.int() - (c + 1024).clamp_(min=0)
    if median:
        h, w = d.shape[1:]
        p = F.pad(d.float().unsqueeze(1), (1, 1, 1, 1), mode="replicate").squeeze(1)      # (exact: |d| < 2^24)
        d = torch.stack([p[:, y:y + h, x:x + w] for y in range(3) for x in range(3)]).sort(dim=0).values[4].int()
    d = torch.where((c < BAND[0]) | (c > BAND[1]) | (d < FLOOR), torch.zeros_like(d), d).clamp_(-32768, 32767)
    wmin = (2 * WINDOW[0] - WINDOW[1]) / 2.0 + 0.5
    t = (d + 1024).float()
    t = torch.where(t == 0, torch.full_like(t, -2000.0), t) - 1024.0 - wmin
    level = torch.trunc(t * (255.0 / WINDOW[1])).clamp_(0, 255).to(torch.uint8)
    return d.short(), level


def kernel(reps=200, rounds=5):
    from cta_gan_amd import ops
    k, s = 16, 512
    gen = torch.Generator().manual_seed(0)
    ct = torch.randint(-1100, 3201, (k, s, s), generator=gen, dtype=torch.int16).cuda()
    cta = torch.randint(0, 4096, (k, s, s), generator=gen, dtype=torch.int16).cuda()
    fake = (torch.rand((k, 1, s, s), generator=gen) * 2 - 1).cuda()
    wc, ww = torch.full((k,), 50.0, device="cuda"), torch.full((k,), 400.0, device="cuda")

    def sub(median):
        return ops.subtract_slices(cta, ct, median=median, floor=FLOOR, ct_range=BAND, wc=WINDOW[0], ww=WINDOW[1])

    for median in (True, False):
        got, want = sub(median), composed(cta, ct, median)
        print("median %s: same sub %s, same level %s, non-zero share %.3f"
              % (median, torch.equal(got[0], want[0]), torch.equal(got[1], want[1]), float((got[0] != 0).float().mean())), flush=True)
    fns = (("subtract_slices (median)", lambda: sub(True)), ("subtract_slices (no median)", lambda: sub(False)),
           ("export_slices", lambda: ops.export_slices(fake, wc, ww)),
           ("torch composition (median)", lambda: composed(cta, ct, True)),
           ("torch composition (no median)", lambda: composed(cta, ct, False)))
    for _, fn in fns:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in fns}
    for _ in range(rounds):
        for name, fn in fns:
            n = reps if "composition" not in name else max(reps // 10, 1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / n)
    npix = k * s * s
    for name, v in times.items():
        print("%-32s us per call, %d windows: %s" % (name, rounds, " ".join("%.1f" % t for t in v)), flush=True)
    best = {name: min(v) for name, v in times.items()}
    for name in ("subtract_slices (median)", "subtract_slices (no median)", "export_slices"):
        print("%-32s %.1f us best window, %.2f TB/s over 7 B/pixel (%.1f MB)" % (name, best[name], 7 * npix / best[name] / 1e6, 7 * npix / 1e6))
    print("median / export %.2f, no median / export %.2f; composition / fused: median %.1fx, no median %.1fx"
          % (best["subtract_slices (median)"] / best["export_slices"], best["subtract_slices (no median)"] / best["export_slices"],
             best["torch composition (median)"] / best["subtract_slices (median)"],
             best["torch composition (no median)"] / best["subtract_slices (no median)"]))


def series(n=256, s=512, batch=16, rounds=6):
    import numpy as np
    from cta_gan_amd import nets, synth
    from cta_gan_amd.Model.HdGan import Generator
    from cta_gan_amd.infer import SeriesTranslator
    vol = np.random.RandomState(0).randint(-1100, 3000, size=(n, s, s)).astype(np.int16)
    nets.set_default_compute_dtype(torch.bfloat16)
    g = synth.fill_module(Generator(1, 1), seed=0).cuda()
    legs = (("subtract=False", SeriesTranslator(g, batch=batch)), ("subtract=True", SeriesTranslator(g, batch=batch, subtract=True)))
    for _, tr in legs:
        tr(vol[:2 * batch])
    torch.cuda.synchronize()
    rate = {name: [] for name, _ in legs}
    for r in range(rounds):
        for name, tr in (legs if r % 2 == 0 else legs[::-1]):
            t0 = time.perf_counter()
            out = tr(vol)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            del out      # giving the result arrays back to the system is part of what a caller in a loop pays
            dt = time.perf_counter() - t0
            rate[name].append(n / dt)
            print("round %d %-15s %.1f slices/s (%.1f ms, of which releasing the result %.1f); host ms of the call: %s"
                  % (r, name, n / dt, dt * 1e3, (dt - (t1 - t0)) * 1e3, " ".join("%s %.1f" % (k, v * 1e3) for k, v in tr.stats.items())),
                  flush=True)
    a, b = sorted(rate["subtract=False"]), sorted(rate["subtract=True"])
    print("subtract=False min %.1f median %.1f max %.1f slices/s; subtract=True min %.1f median %.1f max %.1f slices/s; "
          "ratio of the medians %.4f" % (a[0], a[len(a) // 2], a[-1], b[0], b[len(b) // 2], b[-1], b[len(b) // 2] / a[len(a) // 2]))
    nets.set_default_compute_dtype(torch.float32)


if __name__ == "__main__":
    print("build digest", _digest(), flush=True)
    {"kernel": kernel, "series": series}[sys.argv[1]]()
