"""What the lumen sections cost beside the centreline they are measured along (LAB_NOTES: "Lumen profile").

    python scripts/lumen_bench.py [--reps 10] [--slices 64] [--side 512] [--rays 32] [--reach 16] [--oversample 2] [--recentre 0]

The volume is the tube phantom of reformat_bench.py (tubes 6 voxels thick along z on a grid of 64, stored 1400 .. 1499 over 1000 ..
1099).  The table is the fan of `lumen_lines` along the axes of 1024 / slices tubes, slices sections each: R = 1024 sections at the
defaults, K = 32 rays, T = 33 steps.  One `ops.lumen_sections` call per repetition after a warm-up call, timed by device events,
trilinear and nearest alternating; beside it the host clock of clearance + field + trace of `VolumeCentreline`'s three ops from one end
of the first tube to the other, synchronised.  Prints every repetition, the median and the spread (max - min over the median)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def report(name, ms):
    med = statistics.median(ms)
    print("%-34s %s ms  median %.3f  spread %.1f %%" % (name, " ".join("%.3f" % t for t in ms), med, 100 * (max(ms) - min(ms)) / med), flush=True)


def main(o):
    import numpy as np
    import torch
    from reformat_bench import phantom
    from cta_gan_amd import ops
    from cta_gan_amd.infer import centreline_penalty, centreline_steps, lumen_lines
    n, s = o.slices, o.side
    vol = phantom(n, s).cuda()
    tubes = max(1, 1024 // n)
    side = max(1, min(s // 64 - 1, int(tubes ** 0.5 + 0.999)))      # tubes off the volume's edge: a fan there would leave the volume
    axes = [(64.0 * (1 + t // side % side) + 2.5, 64.0 * (1 + t % side) + 2.5) for t in range(tubes)]
    fans = [lumen_lines(n, s, s, [[0.0, y, x], [n - 1.0, y, x]], rays=o.rays, reach=o.reach, oversample=o.oversample) for y, x in axes]
    steps = fans[0].steps
    table = ops.LineTable(np.concatenate([f[0] for f in fans]), o.rays, steps, vol.device)
    print("volume %d x %d x %d, R = %d sections, K = %d rays, T = %d steps, recentre %d" % (n, s, s, table.shape[0], o.rays, steps, o.recentre), flush=True)
    took = {"trilinear": [], "nearest": []}
    for rep in range(o.reps + 1):
        for sampling in took:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            radii, cross, sections, centres = ops.lumen_sections(vol, table, o.rays, steps, 1400, sampling=sampling, recentre=o.recentre)
            b.record()
            b.synchronize()
            if rep:
                took[sampling].append(a.elapsed_time(b))
        if not rep:
            sec = sections.cpu().numpy()
            print("valid sections %d of %d, mean diameter %.2f px" % (int(((sec[:, 5] == 0) & (sec[:, 6] == 0)).sum()), len(sec),
                                                                     float(sec[:, 0].mean()) * 2.0 / o.rays / (256.0 * o.oversample)), flush=True)
    for sampling, ms in took.items():
        report("lumen_sections, %s" % sampling, ms)
    # the centreline of the same volume, for scale: clearance + field + trace along the first tube
    r = 8
    pen_host, lengths = centreline_penalty(r), centreline_steps(1.0)
    pen = torch.from_numpy(pen_host.view(np.int16)).cuda().view(torch.uint16)
    start, end = (0 * s + 2) * s + 2, ((n - 1) * s + 2) * s + 2
    ends = torch.tensor([end], dtype=torch.int32, device="cuda")
    scratch = clear = dist = None
    ms = []
    for rep in range(min(o.reps, 5) + 1):
        scratch = torch.empty(vol.shape, dtype=torch.uint16, device="cuda") if scratch is None else scratch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clear = ops.centreline_clearance(vol, 1400, 32767, r, 256, scratch=scratch, clear=clear)
        dist, stats = ops.centreline_field(clear, pen, lengths, start, r, dist=dist)
        paths, counts = ops.centreline_trace(clear, pen, lengths, dist, ends, r, 4 * (n + 2 * s), stats=stats)
        torch.cuda.synchronize()
        if rep:
            ms.append(1e3 * (time.perf_counter() - t0))
    report("centreline (clearance+field+trace)", ms)
    print("path of %d voxels in %d rounds, stats %s" % (int(counts[0]), ops.centreline_field.rounds, stats.tolist()), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--rays", type=int, default=32)
    ap.add_argument("--reach", type=float, default=16.0)
    ap.add_argument("--oversample", type=int, default=2)
    ap.add_argument("--recentre", type=int, default=0)
    main(ap.parse_args())
