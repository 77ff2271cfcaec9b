"""What the connected components cost (LAB_NOTES: "Connected components"): kernel times from `rocprofv3 --kernel-trace`.

    python scripts/components_bench.py [--out DIR] [--reps 20] [--slices 256] [--side 512]
    python scripts/components_bench.py --e2e [--slices 256] [--side 512] [--reps 3]      # SeriesTranslator with / without components

The parent (no GPU work of its own) runs this file as a child under `rocprofv3 --kernel-trace`, once per case, reads the trace back
and prints one line per kernel: launches, the mean microseconds per launch, and for the streaming kernels the bytes a launch has to
move and the rate, beside `export_stream_kernel` moving a volume of the same voxel count in the same job (7 bytes per voxel).

Cases, each one int16 volume of `--slices` x `--side` x `--side` that stays on the device, connectivity 26:
  phantom    the tube phantom of reformat_bench.py --phantom at a threshold that keeps the tubes (lo = 1400): a few hundred long
             components, 0.9 % foreground
  random     uniform random values at a threshold that leaves a tenth of the voxels foreground: millions of small components
Each repetition is label + select (largest 8, top 8: eight ranking passes) + apply with both outputs.  CTG_LIB picks another build
of the library (the A/B against a build with -DCC_LOCAL=0: no LDS phase, the merge kernel over every forward neighbour).

--e2e times `SeriesTranslator(components=...)(volume)` against `components=None` on a synthetic generator, alternating, `--reps`
calls each after one warm-up call each, and prints every call's seconds beside the ratio of the medians."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CASES = ("phantom", "random")
# bytes per voxel a launch has to move (reads + writes that cannot be avoided), for the streaming kernels
MOVED = {"cc_flatten_kernel": 4, "cc_sizes_kernel": 4, "cc_apply_kernel": 2 + 4 + 2 + 1, "export_stream_kernel": 4 + 2 + 1,
         "cc_select_zero_kernel": 5, "cc_local_kernel": 2 + 4}


def volume(case, n, s):
    import torch
    from reformat_bench import phantom
    if case == "phantom":
        return phantom(n, s).cuda(), 1400
    vol = torch.randint(0, 4096, (n, s, s), generator=torch.Generator().manual_seed(0), dtype=torch.int16).cuda()
    return vol, 4096 - 410      # 410 of 4096 values: a tenth


def child(o):
    import torch
    from cta_gan_amd import build, ops
    n, s = o.slices, o.side
    vol, lo = volume(o.case, n, s)
    fake = torch.rand((64, 1, s, s), generator=torch.Generator().manual_seed(1)).cuda() * 2 - 1
    wc, ww = torch.full((64,), 50.0, device="cuda"), torch.full((64,), 400.0, device="cuda")
    labels = sizes = keep = None
    stats = None
    for rep in range(o.reps + 2):      # (two warm-up repetitions are traced too: the parent drops nothing, the means barely move)
        labels, stats = ops.components_label(vol, lo, 32767, 26, labels=labels, stats=stats)
        sizes, keep, top = ops.components_select(labels, stats, largest=8, ntop=8, sizes=sizes, keep=keep)
        values, level = ops.components_apply(vol, labels, keep)
        for _ in range(n // 64):
            ops.export_slices(fake, wc, ww)
        torch.cuda.synchronize()
    with open(o.child, "w") as fh:
        json.dump({"stats": stats.tolist(), "top": top.tolist(), "digest": build._digest()[:16], "voxels": vol.numel(),
                   "lib": os.environ.get("CTG_LIB", "")}, fh)


def report(trace, made, n_export):
    by = {}
    for r in csv.DictReader(open(trace)):
        name = r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "")
        if name.startswith("cc_") or name.startswith("export_stream"):
            by.setdefault(name, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    v = made["voxels"]
    for name, ns in by.items():
        us = sum(ns) / len(ns) / 1e3
        vox = v // n_export if name.startswith("export_stream") else v
        rate = "  %6.1f MB to move = %5.2f TB/s" % (MOVED[name] * vox / 1e6, MOVED[name] * vox / us / 1e6) if name in MOVED else ""
        print("%-26s %5d launches  %9.1f us mean  %9.1f us shortest%s" % (name, len(ns), us, min(ns) / 1e3, rate), flush=True)


def parent(o):
    os.makedirs(o.out, exist_ok=True)
    for case in CASES:
        where, plan = os.path.join(o.out, case), os.path.join(o.out, case + "_plan.json")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", where, "-o", "p", "--", sys.executable,
               os.path.abspath(__file__), "--child", plan, "--case", case, "--reps", str(o.reps), "--slices", str(o.slices), "--side",
               str(o.side)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=o.timeout)
        if r.returncode != 0:
            raise SystemExit("the %s child failed (%d):\n%s" % (case, r.returncode, r.stderr[-4000:]))
        traces = glob.glob(os.path.join(where, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise SystemExit("one kernel trace expected under %s, found %r" % (where, traces))
        made = json.load(open(plan))
        print("case %s: %d x %d x %d, build digest %s%s; stats %s; top %s" % (case, o.slices, o.side, o.side, made["digest"],
              " (CTG_LIB=%s)" % made["lib"] if made["lib"] else "", made["stats"], made["top"][:3]), flush=True)
        report(traces[0], made, o.slices // 64)


def e2e(o):
    import numpy as np
    import torch
    from cta_gan_amd import nets, synth
    from cta_gan_amd.infer import SeriesTranslator
    from cta_gan_amd.Model.HdGan import Generator
    nets.set_default_compute_dtype(torch.bfloat16)
    g = synth.fill_module(Generator(1, 1), seed=0).cuda()
    vol = np.random.RandomState(0).randint(-1100, 3200, size=(o.slices, o.side, o.side)).astype(np.int16)
    legs = {"plain": SeriesTranslator(g, batch=16, project="max"),
            "components": SeriesTranslator(g, batch=16, project="max", project_source="vessels",
                                           components=dict(threshold=2500, min_voxels=4, largest=8))}
    took = {k: [] for k in legs}
    for rep in range(o.reps + 1):
        for name, tr in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = tr(vol)
            dt = time.perf_counter() - t0
            if rep:
                took[name].append(dt)
    for name, ts in took.items():
        print("%-11s %s s  median %.3f  spread %.1f %%" % (name, " ".join("%.3f" % t for t in ts), statistics.median(ts),
                                                           100 * (max(ts) - min(ts)) / statistics.median(ts)), flush=True)
    print("components / plain = %.3f; stats %s" % (statistics.median(took["components"]) / statistics.median(took["plain"]),
                                                   out["vessels"]["stats"].tolist()), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="components_bench_out", help="where the traces and the plans go")
    ap.add_argument("--reps", type=int, default=None, help="timed repetitions per case (default 20; 3 with --e2e)")
    ap.add_argument("--slices", type=int, default=256)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--timeout", type=int, default=400, help="seconds a child may take")
    ap.add_argument("--child", default=None, help="(internal) run the launches and write the plan here")
    ap.add_argument("--case", choices=CASES, default="phantom", help="(internal) the child's case")
    ap.add_argument("--e2e", action="store_true", help="SeriesTranslator with and without components instead")
    o = ap.parse_args()
    if o.slices % 64:
        raise SystemExit("--slices: a multiple of 64 expected")
    o.reps = o.reps if o.reps is not None else (3 if o.e2e else 20)
    e2e(o) if o.e2e else (child(o) if o.child else parent(o))
