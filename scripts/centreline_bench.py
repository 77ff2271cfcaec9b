"""What the vessel centreline costs (LAB_NOTES: "Vessel centreline"): kernel times from `rocprofv3 --kernel-trace`.

    python scripts/centreline_bench.py [--out DIR] [--reps 5] [--slices 256] [--side 512] [--radius 8] [--reverse]
    python scripts/centreline_bench.py --e2e [--slices 256] [--side 512] [--reps 3]      # SeriesTranslator with / without centreline

The parent (no GPU work of its own) runs this file as a child under `rocprofv3 --kernel-trace`, reads the trace back and prints one
line per kernel: launches and the mean microseconds per launch; for the relaxation also the rounds of a repetition, the rounds in
which a tile was active, and the time of a whole relaxation.  The volume is the tube phantom of reformat_bench.py --phantom at a
threshold that keeps the tubes (lo = 1400), the start and the end the two ends of the first tube; each repetition is clearance +
field + trace.  CTG_LIB picks another build of the library (the A/B against a build with -DCL_LOCAL=0: no LDS iteration, an active
tile relaxes each voxel once per round on global memory).  The child also times, for context, the same shortest paths on the host:
the copy of the clearance back, and scipy's Dijkstra on the start's component.

--e2e times `SeriesTranslator(centreline=...)(volume)` against `centreline=None` on a synthetic generator, alternating, `--reps`
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


def host_dijkstra(clear, pen, steps, start, end):
    """scipy's Dijkstra on the component of `start` (found by scipy.ndimage.label inside the tube's bounding box) -> (voxels of the
    component, seconds of graph + Dijkstra, dist[end])."""
    import numpy as np
    from scipy.ndimage import label
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    t0 = time.perf_counter()
    n, h, w = clear.shape
    lab, _ = label(clear > 0, structure=np.ones((3, 3, 3)))
    member = lab.reshape(-1) == lab.reshape(-1)[start]
    ids = np.flatnonzero(member)
    slot = np.full(clear.size, -1, dtype=np.int64)
    slot[ids] = np.arange(ids.size)
    cost = np.clip(pen.astype(np.int64), 1, 4095)[np.minimum(clear.reshape(-1)[ids].astype(np.int64), len(pen) - 1)]
    z, y, x = ids // (h * w), (ids // w) % h, ids % w
    rows, cols, vals = [], [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) == (0, 0, 0):
                    continue
                k = (dy != 0) + (dx != 0)
                vz, vy, vx = z + dz, y + dy, x + dx
                ok = (vz >= 0) & (vz < n) & (vy >= 0) & (vy < h) & (vx >= 0) & (vx < w)
                v = slot[((vz * h + vy) * w + vx)[ok]]
                keep = v >= 0
                rows.append(np.flatnonzero(ok)[keep])
                cols.append(v[keep])
                vals.append(steps[k - 1 if dz == 0 else 2 + k] * cost[v[keep]])
    graph = csr_matrix((np.concatenate(vals).astype(np.float64), (np.concatenate(rows), np.concatenate(cols))), shape=(ids.size,) * 2)
    d = dijkstra(graph, directed=True, indices=int(slot[start]))
    return int(ids.size), time.perf_counter() - t0, float(d[slot[end]])


def child(o):
    import numpy as np
    import torch
    from reformat_bench import phantom
    from cta_gan_amd import build, ops
    from cta_gan_amd.infer import centreline_penalty, centreline_steps
    n, s, r = o.slices, o.side, o.radius
    vol = phantom(n, s).cuda()
    start, end = (0 * s + 2) * s + 2, ((n - 1) * s + 2) * s + 2      # the axis of the first tube, first and last slice
    if o.reverse:      # against the order in which a thread walks its voxels: the global-sweep build then gains one slice per round
        start, end = end, start
    pen_host, steps = centreline_penalty(r), centreline_steps(1.0)
    pen = torch.from_numpy(pen_host.view(np.int16)).cuda().view(torch.uint16)
    ends = torch.tensor([end], dtype=torch.int32, device="cuda")
    scratch = clear = dist = None
    for rep in range(o.reps + 1):      # (the warm-up repetition is traced too)
        scratch = torch.empty(vol.shape, dtype=torch.uint16, device="cuda") if scratch is None else scratch
        clear = ops.centreline_clearance(vol, 1400, 32767, r, 256, scratch=scratch, clear=clear)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dist, stats = ops.centreline_field(clear, pen, steps, start, r, rounds_per_call=o.rounds_per_call, max_rounds=o.max_rounds, dist=dist)
        torch.cuda.synchronize()
        field_s = time.perf_counter() - t0
        paths, counts = ops.centreline_trace(clear, pen, steps, dist, ends, r, 4 * (n + 2 * s), stats=stats)
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    clear_host = clear.cpu().numpy()
    copy_s = time.perf_counter() - t0
    voxels, dijkstra_s, d_end = host_dijkstra(clear_host, pen_host, steps, start, end)
    with open(o.child, "w") as fh:
        json.dump({"stats": stats.tolist(), "count": int(counts[0]), "rounds": ops.centreline_field.rounds, "field_s": field_s,
                   "dist_end": int(dist.reshape(-1)[end].item()), "dijkstra_end": d_end, "component": voxels, "copy_s": copy_s,
                   "dijkstra_s": dijkstra_s, "digest": build._digest()[:16], "lib": os.environ.get("CTG_LIB", "")}, fh)


def parent(o):
    os.makedirs(o.out, exist_ok=True)
    where, plan = os.path.join(o.out, "phantom"), os.path.join(o.out, "phantom_plan.json")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", where, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
           "--child", plan, "--reps", str(o.reps), "--slices", str(o.slices), "--side", str(o.side), "--radius", str(o.radius),
           "--rounds-per-call", str(o.rounds_per_call), "--max-rounds", str(o.max_rounds)] + (["--reverse"] if o.reverse else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=o.timeout)
    if r.returncode != 0:
        raise SystemExit("the child failed (%d):\n%s" % (r.returncode, r.stderr[-4000:]))
    traces = glob.glob(os.path.join(where, "**", "*kernel_trace.csv"), recursive=True)
    if len(traces) != 1:
        raise SystemExit("one kernel trace expected under %s, found %r" % (where, traces))
    made = json.load(open(plan))
    print("phantom %d x %d x %d, R = %d, build digest %s%s: %d rounds launched per field, path of %d voxels, dist[end] %d (scipy %.0f), "
          "stats %s" % (o.slices, o.side, o.side, o.radius, made["digest"], " (CTG_LIB=%s)" % made["lib"] if made["lib"] else "",
                        made["rounds"], made["count"], made["dist_end"], made["dijkstra_end"], made["stats"]), flush=True)
    by = {}
    for row in csv.DictReader(open(traces[0])):
        name = row["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "")
        if name.startswith("cl_"):
            by.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for name, us in by.items():
        print("%-22s %6d launches  %9.1f us mean  %9.1f us shortest  %9.1f us longest" % (name, len(us), sum(us) / len(us), min(us), max(us)),
              flush=True)
    relax, fields = by.get("cl_relax_kernel", []), o.reps + 1
    if relax:
        idle = min(relax)
        busy = [u for u in relax if u > 2 * idle]
        print("relaxation: %.1f us of kernels per field (%d rounds, %.1f us per round; %d rounds above twice the shortest launch, %.1f us each); "
              "%.2f ms on the host clock with one synchronisation per %d rounds"
              % (sum(relax) / fields, len(relax) // fields, sum(relax) / len(relax), len(busy) // fields, sum(busy) / max(1, len(busy)),
                 1e3 * made["field_s"], o.rounds_per_call), flush=True)
    print("host, for context: %.1f ms to copy the clearance back, %.1f ms for scipy's label + graph + Dijkstra on the start's component "
          "(%d voxels)" % (1e3 * made["copy_s"], 1e3 * made["dijkstra_s"], made["component"]), flush=True)


def e2e(o):
    import numpy as np
    import torch
    from cta_gan_amd import nets, synth
    from cta_gan_amd.infer import SeriesTranslator
    from cta_gan_amd.Model.HdGan import Generator
    nets.set_default_compute_dtype(torch.bfloat16)
    g = synth.fill_module(Generator(1, 1), seed=0).cuda()
    vol = np.random.RandomState(0).randint(-1100, 3200, size=(o.slices, o.side, o.side)).astype(np.int16)
    plain = SeriesTranslator(g, batch=16, project="max")
    pix = plain(vol)["pix"]
    # the synthesized volume of noise is noise: at its median half the voxels are foreground and one component spans the volume
    lo = int(np.median(pix[::8, ::8, ::8]))
    from scipy.ndimage import label
    lab, _ = label(pix >= lo, structure=np.ones((3, 3, 3)))
    members = np.flatnonzero(lab.reshape(-1) == int(np.argmax(np.bincount(lab.reshape(-1))[1:])) + 1)
    start, end = (tuple(int(v) for v in np.unravel_index(i, pix.shape)) for i in (members[0], members[-1]))
    legs = {"plain": plain,
            "centreline": SeriesTranslator(g, batch=16, project="max",
                                           centreline=dict(threshold=lo, start=start, ends=[end], radius=o.radius, max_points=1 << 16))}
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
    from cta_gan_amd import ops
    print("centreline / plain = %.3f; threshold %d, %d rounds, path of %d voxels, stats %s"
          % (statistics.median(took["centreline"]) / statistics.median(took["plain"]), lo, ops.centreline_field.rounds,
             int(out["centreline"]["counts"][0]), out["centreline"]["stats"].tolist()), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="centreline_bench_out", help="where the trace and the plan go")
    ap.add_argument("--reps", type=int, default=None, help="timed repetitions (default 5; 3 with --e2e)")
    ap.add_argument("--slices", type=int, default=256)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--rounds-per-call", type=int, default=16)
    ap.add_argument("--max-rounds", type=int, default=4096)
    ap.add_argument("--reverse", action="store_true", help="trace from the last slice to the first")
    ap.add_argument("--timeout", type=int, default=400, help="seconds the child may take")
    ap.add_argument("--child", default=None, help="(internal) run the launches and write the plan here")
    ap.add_argument("--e2e", action="store_true", help="SeriesTranslator with and without centreline instead")
    o = ap.parse_args()
    o.reps = o.reps if o.reps is not None else (3 if o.e2e else 5)
    e2e(o) if o.e2e else (child(o) if o.child else parent(o))
