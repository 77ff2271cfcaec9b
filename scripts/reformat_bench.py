"""What the lines in any direction cost (LAB_NOTES: "Reformats"): kernel times from `rocprofv3 --kernel-trace`.

    python scripts/reformat_bench.py [--out DIR] [--launches 100] [--slices 256] [--side 512] [--angles 36]
    python scripts/reformat_bench.py --render [--phantom] ...      # the legs of ctg_render_lines instead (`child_render`)

The parent (no GPU work of its own) runs this file twice as a child under `rocprofv3 --kernel-trace --stats`, once per layout of
the T = 1 kernel (CTG_REFORMAT_T1 = 1 / 2, read once per process), reads the traces back and prints one line per leg: the mean
kernel time over `--launches` launches, the samples per second, and the bytes a launch has to move (the volume once, the table,
3 bytes per ray out) beside the bytes its gathers ask the caches for (2 per nearest sample, 16 per trilinear one).

Legs, on one int16 volume of `--slices` x `--side` x `--side` that stays on the device:
  rotate nearest / bilinear      ctg_project_rotate / _bilinear, `--angles` views about z, the volume in chunks of 16 slices: the time
                                 of a leg is that of the 16 launches that make one volume's views
  lines z / x, nearest / tri     ctg_reformat_lines on infer.orbit_lines about z (the same rays as the rotation: the outputs are
                                 compared first) and about x (the tumble, at its default detector: the volume's diagonal)
  planes <normal> nearest / tri  `--slices` parallel planes, T = 1, with the normal (1, 1, 1) (oblique), +y (coronal: the lines run along
                                 x) and +x (sagittal: the lines run along y): the legs that differ between the layouts

The kernels are told apart by the order of their launches, which the child writes down (plan.json) and the parent checks against
the kernel names of the trace."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 16


def child(o):
    import torch
    from cta_gan_amd import build, ops
    from cta_gan_amd.infer import default_detector, oblique_lines, orbit_lines, plan_chunks, rotation_coefficients, view_angles
    n, s, count = o.slices, o.side, o.angles
    angles = view_angles(count)
    d = default_detector(s, s)
    vol = torch.randint(0, 4096, (n, s, s), generator=torch.Generator().manual_seed(0), dtype=torch.int16).cuda()
    plan, legs = [], {}

    def leg(name, kernel, fn, per_rep, samples, moved, gathered, reps):
        for _ in range(2):
            fn()
        plan.append(("warm-up " + name, kernel, 2 * per_rep, 0))
        for _ in range(reps):
            fn()
        plan.append((name, kernel, reps * per_rep, per_rep))
        legs[name] = {"samples": samples, "moved": moved, "gathered": gathered}
        torch.cuda.synchronize()

    reps = max(1, -(-o.launches // (n // CHUNK)))      # >= --launches launches of the chunked legs
    table = ops.RotateTable([rotation_coefficients(a, s, s) for a in angles])
    rv = torch.empty((count, n, d), dtype=torch.int16, device="cuda")
    rl = torch.empty((count, n, d), dtype=torch.uint8, device="cuda")
    z = orbit_lines(n, s, s, angles, axis="z", rows=n, cols=d, depth=d)
    zt = ops.LineTable(z[0], d, z[1])
    if not o.planes_only:
        for sampling, rotating in (("nearest", "nearest"), ("trilinear", "bilinear")):      # the same rays: the same bits
            for st, e, _ in plan_chunks(n, CHUNK):
                ops.project_rotate(vol[st:e], st, table, d, "max", values=rv, level=rl, sampling=rotating)
            got = ops.reformat_lines(vol, zt, d, z[1], "max", sampling=sampling)
            plan.extend([("check rotate " + rotating, "project_rotate_kernel", n // CHUNK, 0),
                         ("check lines " + sampling, "reformat_rays_kernel", 1, 0)])
            print("lines z %s equals project_rotate %s: values %s, level %s"
                  % (sampling, rotating, torch.equal(got[0], rv), torch.equal(got[1], rl)), flush=True)
            del got
        rays = count * n * d
        for rotating, per in (("nearest", 2), ("bilinear", 8)):
            def fn(rotating=rotating):
                for st, e, _ in plan_chunks(n, CHUNK):
                    ops.project_rotate(vol[st:e], st, table, d, "max", values=rv, level=rl, sampling=rotating)
            leg("rotate " + rotating, "project_rotate_kernel", fn, n // CHUNK, rays * d, 2 * vol.numel() + 3 * rays, per * rays * d, reps)
        x = orbit_lines(n, s, s, angles, axis="x")
        xt = ops.LineTable(x[0], x.cols, x[1])
        for name, made, tab in (("z", z, zt), ("x", x, xt)):
            rays = tab.count * tab.u
            for sampling, per in (("nearest", 2), ("trilinear", 16)):
                leg("lines %s %s" % (name, sampling), "reformat_rays_kernel",
                    lambda tab=tab, sampling=sampling: ops.reformat_lines(vol, tab, tab.u, tab.t, "max", sampling=sampling), 1,
                    rays * tab.t, 2 * vol.numel() + 36 * tab.count + 3 * rays, per * rays * tab.t, o.launches)
    shapes = {"z": [zt.count, zt.u, zt.t]}
    for name, normal in (("oblique", (1, 1, 1)), ("coronal", (0, 1, 0)), ("sagittal", (1, 0, 0))):
        p = oblique_lines(n, s, s, normal, count=n)
        pt = ops.LineTable(p[0], p.cols, p[1])
        rays = pt.count * pt.u
        shapes[name] = [pt.count, pt.u, pt.t]
        for sampling, per in (("nearest", 2), ("trilinear", 16)):
            leg("planes %s %s" % (name, sampling), "reformat_plane_kernel",
                lambda pt=pt, sampling=sampling: ops.reformat_lines(vol, pt, pt.u, 1, "max", sampling=sampling), 1, rays,
                2 * vol.numel() + 36 * pt.count + 3 * rays, per * rays, o.launches)
    layout = {"1": "an 8 x 8 patch", "2": "64 columns of one line"}[os.environ["CTG_REFORMAT_T1"]]
    with open(o.child, "w") as fh:
        json.dump({"plan": plan, "legs": legs, "layout": layout, "digest": build._digest()[:16],
                   "shapes": shapes}, fh)


def phantom(n, s):
    """Soft tissue (stored 1000 .. 1099: transparent under the `vessels` preset) with contrast-filled tubes along z (1400 .. 1499:
    near-opaque), 6 voxels thick on a grid of 64: about 0.9 % of the voxels, so most samples are transparent and a ray ends where
    it meets a tube."""
    import torch
    g = torch.Generator().manual_seed(0)
    vol = torch.randint(1000, 1100, (n, s, s), generator=g, dtype=torch.int16)
    at = torch.arange(s) % 64 < 6
    tube = (at[:, None] & at[None, :])[None].expand(n, s, s)
    return torch.where(tube, vol + 400, vol)


def child_render(o):
    """The legs of the shaded line renderer (LAB_NOTES: "Shaded volume rendering along lines"): ctg_render_lines about z and about x,
    nearest / trilinear, flat / shaded, under the `vessels` preset (stop 128) and under a thin fog that no ray leaves early (every
    alpha 64 / 32768, stop 0), beside ctg_reformat_lines max on the same table and, about z, the sixteen chunked
    ctg_project_render launches."""
    import numpy as np
    import torch
    from cta_gan_amd import build, ops
    from cta_gan_amd.infer import (TRANSFER_PRESETS, default_detector, headlight, orbit_lines, plan_chunks, rotation_coefficients,
                                   transfer_function, view_angles)
    n, s, count = o.slices, o.side, o.angles
    angles = view_angles(count)
    d = default_detector(s, s)
    g = torch.Generator().manual_seed(0)
    vol = (phantom(n, s) if o.phantom else torch.randint(0, 4096, (n, s, s), generator=g, dtype=torch.int16)).cuda()
    fog = np.zeros((256, 4), dtype=np.uint16)
    fog[:, :3], fog[:, 3] = np.arange(256)[:, None], 64
    luts = {"vessels": (ops.TransferTable(transfer_function(TRANSFER_PRESETS["vessels"])), 128), "fog": (ops.TransferTable(fog), 0)}
    plan, legs = [], {}

    def leg(name, kernel, fn, per_rep, samples, reps):
        for _ in range(2):
            fn()
        plan.append(("warm-up " + name, kernel, 2 * per_rep, 0))
        for _ in range(reps):
            fn()
        plan.append((name, kernel, reps * per_rep, per_rep))
        legs[name] = {"samples": samples, "moved": 0, "gathered": 0}
        torch.cuda.synchronize()

    reps = max(1, -(-o.launches // (n // CHUNK)))
    coef = ops.RotateTable([rotation_coefficients(a, s, s) for a in angles])
    out = {"rgb": torch.empty((count, n, d, 3), dtype=torch.uint8, device="cuda"),
           "opacity": torch.empty((count, n, d), dtype=torch.uint8, device="cuda"),
           "depth": torch.empty((count, n, d), dtype=torch.int16, device="cuda")}
    z = orbit_lines(n, s, s, angles, axis="z", rows=n, cols=d, depth=d)
    x = orbit_lines(n, s, s, angles, axis="x")
    tabs = {"z": (z, ops.LineTable(z[0], d, z[1])), "x": (x, ops.LineTable(x[0], x.cols, x[1]))}
    lamps = {name: ops.LightTable(headlight(made), tab.count) for name, (made, tab) in tabs.items()}
    for sampling, rotating in (("nearest", "nearest"), ("trilinear", "bilinear")):      # the same rays: the same bits
        for st, e, _ in plan_chunks(n, CHUNK):
            ops.project_render(vol[st:e], st, coef, d, luts["vessels"][0], sampling=rotating, wc=300.0, ww=1500.0, **out)
        got = ops.render_lines(vol, tabs["z"][1], d, z[1], luts["vessels"][0], sampling=sampling)
        plan.extend([("check render " + rotating, "project_render_kernel", n // CHUNK, 0),
                     ("check lines " + sampling, "render_lines_kernel", 1, 0)])
        print("render_lines z %s equals project_render %s: %s" % (sampling, rotating, [torch.equal(t, out[p]) for p, t in zip(out, got)]),
              flush=True)
        del got
    for lut_name, (lut, stop) in luts.items():
        for rotating in ("nearest", "bilinear"):
            def fn(rotating=rotating, lut=lut, stop=stop):
                for st, e, _ in plan_chunks(n, CHUNK):
                    ops.project_render(vol[st:e], st, coef, d, lut, sampling=rotating, stop=stop, wc=300.0, ww=1500.0, **out)
            leg("project_render z %s %s" % (rotating, lut_name), "project_render_kernel", fn, n // CHUNK, count * n * d * d, reps)
    for name, (made, tab) in tabs.items():
        rays = tab.count * tab.u
        for sampling in ("nearest", "trilinear"):
            leg("reformat max %s %s" % (name, sampling), "reformat_rays_kernel",
                lambda tab=tab, sampling=sampling: ops.reformat_lines(vol, tab, tab.u, tab.t, "max", sampling=sampling), 1, rays * tab.t,
                o.launches)
            for lut_name, (lut, stop) in luts.items():
                for shaded in (False, True):
                    leg("render %s %s %s %s" % (name, sampling, lut_name, "shaded" if shaded else "flat"), "render_lines_kernel",
                        lambda tab=tab, sampling=sampling, lut=lut, stop=stop, lamp=lamps[name] if shaded else None:
                        ops.render_lines(vol, tab, tab.u, tab.t, lut, light=lamp, sampling=sampling, stop=stop), 1, rays * tab.t,
                        o.launches)
    with open(o.child, "w") as fh:
        json.dump({"plan": plan, "legs": legs, "layout": "(T > 1 only)", "digest": build._digest()[:16],
                   "shapes": {k: [t.count, t.u, t.t] for k, (_, t) in tabs.items()}}, fh)


KERNELS = ("reformat_", "project_rotate_kernel", "render_lines_kernel", "project_render_kernel")


def report(trace, plan):
    rows = [r for r in csv.DictReader(open(trace)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(rows) != sum(p[2] for p in plan["plan"]):
        raise SystemExit("%s: %d launches traced, %d planned" % (trace, len(rows), sum(p[2] for p in plan["plan"])))
    at = 0
    for name, kernel, launches, per_rep in plan["plan"]:
        mine, at = rows[at:at + launches], at + launches
        if any(kernel not in r["Kernel_Name"] for r in mine):
            raise SystemExit("%s: the launches of %r are not all %s" % (trace, name, kernel))
        if not per_rep:
            continue
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in mine]
        us = sum(ns) / 1e3 / (launches // per_rep)
        leg = plan["legs"][name]
        print("%-28s %9.1f us (%3d launches, shortest %.1f us%s)  %6.1f G samples/s  %7.1f MB to move = %5.2f TB/s  %8.1f MB gathered"
              % (name, us, launches, min(ns) / 1e3, ", %d a volume" % per_rep if per_rep > 1 else "", leg["samples"] / us / 1e3,
                 leg["moved"] / 1e6, leg["moved"] / us / 1e6, leg["gathered"] / 1e6), flush=True)


def parent(o):
    os.makedirs(o.out, exist_ok=True)
    runs = (("patch", {"CTG_REFORMAT_T1": "1"}, []), ("rows", {"CTG_REFORMAT_T1": "2"}, ["--planes-only"]))
    if o.render:      # the legs of the shaded line renderer alone
        runs = (("render_phantom" if o.phantom else "render", {}, ["--render"] + (["--phantom"] if o.phantom else [])),)
    for tag, env, extra in runs:
        where = os.path.join(o.out, tag)
        plan = os.path.join(o.out, tag + "_plan.json")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", where, "-o", "p", "--", sys.executable,
               os.path.abspath(__file__), "--child", plan, "--launches", str(o.launches), "--slices", str(o.slices), "--side", str(o.side),
               "--angles", str(o.angles)] + extra
        r = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=o.timeout)
        print(r.stdout[-3000:], flush=True)
        if r.returncode != 0:
            raise SystemExit("the %s child failed (%d):\n%s" % (tag, r.returncode, r.stderr[-4000:]))
        traces = glob.glob(os.path.join(where, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise SystemExit("one kernel trace expected under %s, found %r" % (where, traces))
        made = json.load(open(plan))
        print("T = 1 layout: a wave on %s; build digest %s; lines x U x T: %s" % (made["layout"], made["digest"], made["shapes"]), flush=True)
        report(traces[0], made)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="reformat_bench_out", help="where the traces and the plans go")
    ap.add_argument("--launches", type=int, default=100, help="timed launches per leg")
    ap.add_argument("--slices", type=int, default=256)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--angles", type=int, default=36)
    ap.add_argument("--timeout", type=int, default=500, help="seconds a child may take")
    ap.add_argument("--child", default=None, help="(internal) run the launches and write the plan here")
    ap.add_argument("--planes-only", action="store_true", help="(internal) the T = 1 legs only")
    ap.add_argument("--render", action="store_true", help="the legs of ctg_render_lines instead (one child)")
    ap.add_argument("--phantom", action="store_true", help="with --render: soft tissue with sparse tubes instead of uniform random values")
    o = ap.parse_args()
    if o.slices % CHUNK:
        raise SystemExit("--slices: a multiple of %d expected" % CHUNK)
    (child_render(o) if o.render else child(o)) if o.child else parent(o)
