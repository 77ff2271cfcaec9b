"""A/B of the four plain projection entries between two whole builds of the library, one process, alternating legs.

    python scripts/ab_project_libs.py PARENT.so [NEW.so] [--only parent|new] [--rounds 9] [--scale 1]      # NEW defaults to this tree's build

scripts/build_prev.sh swaps one source file; a library that predates an entry point cannot be loaded through cta_gan_amd._lib
(the binding requires every declared symbol), so both libraries are opened with ctypes directly and only ctg_project_rotate,
ctg_project_rotate_bilinear, ctg_project_accumulate and ctg_project_finish are bound, with the signatures written out below
(those of include/ctagan_hip.h under ABI 15).  The chunk of scripts/rotate_bench.py and scripts/project_bench.py (16 x 512 x 512,
36 angles, max); the outputs of the two libraries are compared first; HIP events, --rounds windows per leg of 50 / 30 / 200 / 100
calls times --scale, the order of the legs swapped every round.  --only runs one library alone (for a kernel trace: the kernel
names are the same in both)."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_I, _L, _P, _F = ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_float
ROTATE = [_P, _I, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _F, _F, _I, _P, _P, _P]
ENTRIES = {"ctg_project_rotate": ROTATE, "ctg_project_rotate_bilinear": ROTATE,
           "ctg_project_accumulate": [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P],
           "ctg_project_finish": [_P, _I, _L, _I, _I, _I, _F, _F, _I, _P, _P, _P]}


def load(path):
    if not os.path.isfile(path):
        raise SystemExit("ab_project_libs: no library at %s" % path)
    lib = ctypes.CDLL(path)
    for name, argtypes in ENTRIES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, _I
    return lib


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("parent", help="the library of the other build (a whole build of the parent commit)")
    ap.add_argument("new", nargs="?", default=os.path.join(ROOT, "cta_gan_amd", "_build", "libctagan_hip.so"))
    ap.add_argument("--only", choices=["parent", "new"], default=None, help="time one library alone")
    ap.add_argument("--rounds", type=int, default=9, help="timed windows per leg")
    ap.add_argument("--scale", type=int, default=1, help="multiplies the calls per window")
    o = ap.parse_args(argv)
    if o.rounds < 1 or o.scale < 1:
        ap.error("--rounds and --scale: at least 1")
    import torch      # before the libraries: the load order cta_gan_amd/_lib.py pins
    from cta_gan_amd.infer import default_detector, rotation_coefficients, view_angles
    libs = {"parent": load(o.parent), "new": load(o.new)}
    if o.only:
        libs = {o.only: libs[o.only]}
    k, s, count = 16, 512, 36
    d = default_detector(s, s)
    coef = torch.tensor([rotation_coefficients(a, s, s) for a in view_angles(count)], dtype=torch.int32).cuda()
    vol = torch.randint(0, 4096, (k, s, s), generator=torch.Generator().manual_seed(0), dtype=torch.int16).cuda()
    values = torch.empty((count, k, d), dtype=torch.int16, device="cuda")
    level = torch.empty((count, k, d), dtype=torch.uint8, device="cuda")
    acc = [torch.full(sh, -32768, dtype=torch.int32, device="cuda") for sh in ((1, s, s), (k, s), (k, s))]
    big = [torch.zeros(sh, dtype=torch.int32, device="cuda") for sh in ((1, s, s), (256, s), (256, s))]
    fv = [torch.empty(t.shape, dtype=torch.int16, device="cuda") for t in big]
    fl = [torch.empty(t.shape, dtype=torch.uint8, device="cuda") for t in big]
    st = torch.cuda.current_stream().cuda_stream

    def rotate(lib, name):
        assert getattr(lib, name)(vol.data_ptr(), k, s, s, 0, k, coef.data_ptr(), count, d, d, 0, 0, 50.0, 400.0, 0,
                                  values.data_ptr(), level.data_ptr(), st) == 0

    def accumulate(lib):
        assert lib.ctg_project_accumulate(vol.data_ptr(), k, s, s, 0, k, 0, acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr(),
                                          st) == 0

    def finish(lib):
        for t, v, l in zip(big, fv, fl):
            planes = t.shape[0] if t.dim() == 3 else 1
            assert lib.ctg_project_finish(t.data_ptr(), planes, t.numel() // planes, 0, 1, 1, 50.0, 400.0, 0, v.data_ptr(),
                                          l.data_ptr(), st) == 0

    legs = [("ctg_project_rotate", lambda lib: rotate(lib, "ctg_project_rotate"), 50),
            ("ctg_project_rotate_bilinear", lambda lib: rotate(lib, "ctg_project_rotate_bilinear"), 30),
            ("ctg_project_accumulate", accumulate, 200), ("ctg_project_finish x3", finish, 100)]
    for name, fn, reps in legs:
        reps *= o.scale
        out = {}
        for which, lib in libs.items():      # same bits first
            values.zero_(), level.zero_()
            for t in acc:
                t.fill_(-32768)
            fn(lib)
            torch.cuda.synchronize()
            out[which] = [t.clone() for t in (values, level, *acc, *fv, *fl)]
        same = len(out) < 2 or all(torch.equal(a, b) for a, b in zip(out["parent"], out["new"]))
        for lib in libs.values():
            for _ in range(10):
                fn(lib)
        torch.cuda.synchronize()
        times = {w: [] for w in libs}
        for r in range(o.rounds):
            order = list(libs.items()) if r % 2 == 0 else list(libs.items())[::-1]
            for which, lib in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn(lib)
                e1.record()
                torch.cuda.synchronize()
                times[which].append(e0.elapsed_time(e1) * 1e3 / reps)
        med = {w: sorted(v)[len(v) // 2] for w, v in times.items()}
        print("%-30s same bits %s; us per call, %d windows of %d" % (name, same, o.rounds, reps), flush=True)
        for w, v in times.items():
            print("    %-7s %s   median %.2f min %.2f" % (w, " ".join("%.1f" % x for x in v), med[w], min(v)), flush=True)
        if len(libs) == 2:
            print("    new / parent: median %.4f, min %.4f" % (med["new"] / med["parent"], min(times["new"]) / min(times["parent"])),
                  flush=True)


if __name__ == "__main__":
    main()
