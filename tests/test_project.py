"""CPU: the series projections (csrc/project.hip, cta_gan_amd/infer.py, predict.py --mip-dir) -- the two entry points are declared,
bound and exported; the numpy restatement the GPU tests compare against agrees with cases worked out by hand; the slab and
aspect bookkeeping of the host side; predict.py's new options."""
import ctypes
import os
import sys

import numpy as np
import pytest

import project_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"ctg_project_accumulate": "piiiiiipppp", "ctg_project_finish": "piliiiffippp"}


def test_header_and_binding_carry_the_two_entries():
    from cta_gan_amd import _lib
    from test_abi import parse_header
    decls = parse_header()
    for name, sig in ENTRIES.items():
        assert decls.get(name) == sig, name
        assert _lib.SIGNATURES.get(name) == sig, name
    assert _lib.ABI_VERSION == 15
    text = open(os.path.join(ROOT, "include", "ctagan_hip.h")).read()
    assert "#define CTG_ABI_VERSION 15" in text and "infer.py" in text.split("ctg_project_accumulate")[0][-1200:]


def test_built_library_exports_the_two_entries():
    from cta_gan_amd import build
    lib = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    lib.ctg_abi_version.restype = ctypes.c_int
    assert lib.ctg_abi_version() == 15


VOL = np.array([[[1, -2, 3], [4, 5, -6]], [[-7, 8, 9], [10, -11, 12]]], dtype=np.int16)      # [N=2][H=2][W=3]
BY_HAND = {
    "max": ([[[1, 8, 9], [10, 5, 12]]], [[4, 5, 3], [10, 8, 12]], [[3, 5], [9, 12]]),
    "min": ([[[-7, -2, 3], [4, -11, -6]]], [[1, -2, -6], [-7, -11, 9]], [[-2, -6], [-7, -11]]),
    # sums (-6 6 12 / 14 -6 6), (5 3 -3 / 3 -3 21), (2 3 / 10 11), divided toward zero by 2, 2, 3
    "mean": ([[[-3, 3, 6], [7, -3, 3]]], [[2, 1, -1], [1, -1, 10]], [[0, 1], [3, 3]]),
}


@pytest.mark.parametrize("mode", ["max", "min", "mean"])
def test_restatement_on_a_volume_written_out_by_hand(mode):
    got = project_np.project(VOL, mode)
    for g, want in zip(got, BY_HAND[mode]):
        assert g.dtype == np.int16 and np.array_equal(g, np.array(want, dtype=np.int16)), (mode, g)
    assert got[0].shape == (1, 2, 3) and got[1].shape == (2, 3) and got[2].shape == (2, 2)
    # every slice its own slab: the axial projection is the volume
    assert np.array_equal(project_np.project(VOL, mode, thick=1)[0], VOL)
    assert np.array_equal(project_np.project(VOL, mode, thick=100)[0], got[0])


def test_restatement_truncates_a_negative_mean_toward_zero():
    vol = np.array([-1, -1, -3], dtype=np.int16).reshape(3, 1, 1)
    axial, coronal, sagittal = project_np.project(vol, "mean")
    assert axial.tolist() == [[[-1]]]      # -5 / 3: floor division would say -2
    assert coronal.tolist() == [[-1], [-1], [-3]] and sagittal.tolist() == [[-1], [-1], [-3]]
    # a short last slab divides by its own count: slabs {0, 1}, {2}
    assert project_np.project(vol, "mean", thick=2)[0].reshape(-1).tolist() == [-1, -3]
    big = np.full((3, 2, 2), 32767, dtype=np.int16)
    assert np.array_equal(project_np.project(big, "mean")[0], big[:1])


def test_restatement_levels_of_the_50_400_window():
    # win_min = -149.5, dFactor = 255 / 400: level = trunc((t - 874.5) * 0.6375) clamped
    stored = np.array([0, 1, 874, 875, 876, 877, 1274, 1275, 4095, -1024, 32767], dtype=np.int16)
    want = [0, 0, 0, 0, 0, 1, 254, 255, 255, 0, 255]
    assert project_np.level(stored, 50.0, 400.0).tolist() == want
    # stored value 0 goes through the -2000 rule: in a window that reaches below it, its neighbour 1 has a level and 0 has none
    assert project_np.level(np.array([0, 1, 2], dtype=np.int16), -1000.0, 400.0).tolist() == [0, 112, 113]
    # hu: the values are stored values minus 1024
    assert project_np.level(stored.astype(np.int32) - 1024, 50.0, 400.0, hu=True).tolist() == want
    lv = project_np.level(np.arange(-2048, 4096, dtype=np.int16), 300.0, 1500.0)
    assert lv.dtype == np.uint8 and np.unique(lv).size == 256 and (np.diff(lv.astype(int)[2049:]) >= 0).all()


def test_slab_bookkeeping():
    from cta_gan_amd.infer import slab_plan
    assert slab_plan(7, 3) == (3, 1)
    assert slab_plan(6, 3) == (2, 3)
    assert slab_plan(7, 1) == (7, 1) and slab_plan(7, 7) == (1, 7) and slab_plan(7, 100) == (1, 7)
    for n, thick in ((7, 3), (6, 3), (5, 100)):
        s, last = slab_plan(n, thick)
        assert project_np.project(np.zeros((n, 1, 1), dtype=np.int16), "max", thick)[0].shape[0] == s
        assert n - range(0, n, thick)[-1] == last
    with pytest.raises(ValueError):
        slab_plan(3, 0)


def test_aspect_row_index():
    from cta_gan_amd.infer import aspect_rows
    assert aspect_rows(5, 1.0).tolist() == [0, 1, 2, 3, 4]
    assert aspect_rows(7, 2.0).tolist() == [i // 2 for i in range(14)]
    assert aspect_rows(4, 0.5).tolist() == [0, 2]
    assert aspect_rows(3, 1.5).tolist() == [0, 0, 1, 2]      # round(4.5) = 4 rows, scale 0.75
    assert aspect_rows(1, 0.1).tolist() == [0]
    r = aspect_rows(300, 2.5)
    assert len(r) == 750 and r[0] == 0 and r[-1] == 299 and (np.diff(r) >= 0).all()


def test_predict_projection_arguments():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import predict
    p = predict.build_parser()
    base = ["--weights", "g.pth", "--input", "in.npy", "--output", "out.npy"]
    o = p.parse_args(base)
    assert o.mip_dir is None and o.mip_mode == "max" and o.slab is None and o.aspect == 1.0      # nothing new happens
    o = p.parse_args(base + ["--mip-dir", "mip", "--mip-mode", "mean", "--slab", "10", "--aspect", "2.5"])
    assert (o.mip_dir, o.mip_mode, o.slab, o.aspect) == ("mip", "mean", 10, 2.5)
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--mip-dir", "mip", "--mip-mode", "median"])
