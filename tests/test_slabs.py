"""CPU: the sliding thin-slab projections (csrc/project_slabs.hip, cta_gan_amd/infer.py: slab_windows, predict.py --sts-dir) --
the two entry points are declared and bound; the slab rule against brute enumeration; the numpy restatement the GPU tests
compare against (tests/slabs_np.py) against project_np, sliding_window_view and cases worked out by hand; predict.py's options."""
import os
import sys

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import project_np
import slabs_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"ctg_project_slabs_inplane": "piiiiiiiiiffippp", "ctg_project_accumulate_sliding": "piiiiiiiipp"}
MODES = ["max", "min", "mean"]


def test_header_and_binding_carry_the_two_entries():
    from cta_gan_amd import _lib
    from test_abi import parse_header
    decls = parse_header()
    for name, sig in ENTRIES.items():
        assert decls.get(name) == sig, name
        assert _lib.SIGNATURES.get(name) == sig, name
    assert _lib.ABI_VERSION == 15      # purely additive
    assert "#define CTG_ABI_VERSION 15" in open(os.path.join(ROOT, "include", "ctagan_hip.h")).read()


def test_slab_windows_against_brute_enumeration():
    from cta_gan_amd.infer import slab_plan, slab_windows
    for length in range(1, 13):
        for thick in range(1, 15):
            for step in range(1, thick + 1):
                j, clipped, last = slab_windows(length, thick, step)
                wins = slabs_np.windows(length, thick, step)
                assert (j, clipped, last) == (len(wins), min(thick, length), wins[-1][1] - wins[-1][0]), (length, thick, step)
                assert wins == [(i * step, min(i * step + clipped, length)) for i in range(j)]
                # the windows cover [0, length), and only the last may be short
                covered = np.zeros(length, dtype=bool)
                for a, b in wins:
                    covered[a:b] = True
                assert covered.all() and wins[0][0] == 0 and wins[-1][1] == length
                assert all(b - a == clipped for a, b in wins[:-1]) and 1 <= last <= clipped
                assert all(b < length for a, b in wins[:-1])      # no window before the last reaches the end
                if step == thick:
                    assert (j, last) == slab_plan(length, thick)
    for bad in ((0, 1, 1), (5, 0, 1), (5, 3, 0), (5, 3, 4), (5, 100, 101)):
        with pytest.raises(ValueError):
            slab_windows(*bad)
    assert slab_windows(5, 100, 100) == (1, 5, 5)
    assert slab_windows(5, 100, 7) == (1, 5, 5)      # the step is checked against the thickness given, before the clip
    assert slab_windows(512, 10, 5) == (102, 10, 7) and slab_windows(512, 10, 1) == (503, 10, 10)


@pytest.fixture(scope="module")
def volume():
    return np.random.RandomState(11).randint(-32768, 32768, size=(7, 9, 11)).astype(np.int16)


@pytest.mark.parametrize("mode", MODES)
def test_restatement_without_overlap_is_the_axial_projection(volume, mode):
    for thick in (1, 2, 3, 7, 100):
        assert np.array_equal(slabs_np.slabs(volume, mode, thick, thick, "axial"), project_np.project(volume, mode, thick)[0])
    # one slab over the whole axis: the whole-volume projections
    whole = project_np.project(volume, mode)
    assert np.array_equal(slabs_np.slabs(volume, mode, 100, 3, "coronal")[0], whole[1])
    assert np.array_equal(slabs_np.slabs(volume, mode, 100, 100, "sagittal")[0], whole[2])


@pytest.mark.parametrize("mode", ["max", "min"])
def test_restatement_equals_sliding_window_view_where_windows_are_full(volume, mode):
    red = {"max": np.max, "min": np.min}[mode]
    for axis, ax in slabs_np.AXIS.items():
        length = volume.shape[ax]
        for thick, step in ((1, 1), (3, 1), (3, 2), (4, 3), (5, 5)):
            got = slabs_np.slabs(volume, mode, thick, step, axis)
            wins = slabs_np.windows(length, thick, step)
            view = red(sliding_window_view(volume, thick, axis=ax), axis=-1)      # the window's start where the axis was
            view = np.moveaxis(view, ax, 0)[::step]
            full = [i for i, (a, b) in enumerate(wins) if b - a == thick]
            assert len(full) >= len(wins) - 1 and got.shape[0] == len(wins)
            assert np.array_equal(got[full], view[:len(full)]), (axis, thick, step)
            assert got.shape[1:] == tuple(s for i, s in enumerate(volume.shape) if i != ax)


def test_restatement_mean_truncates_toward_zero_with_the_short_slab_s_own_divisor():
    line = np.array([-1, -1, -3, -2, 5], dtype=np.int16)
    # thick 3, step 2: windows [0, 3) and [2, 5): -5 / 3 and 0 / 3; floor division would say -2
    for axis, shape in (("axial", (5, 1, 1)), ("coronal", (1, 5, 1)), ("sagittal", (1, 1, 5))):
        assert slabs_np.slabs(line.reshape(shape), "mean", 3, 2, axis).reshape(-1).tolist() == [-1, 0]
        # thick 3, step 3: windows [0, 3) and the short [3, 5): 3 / 2 = 1
        assert slabs_np.slabs(line.reshape(shape), "mean", 3, 3, axis).reshape(-1).tolist() == [-1, 1]
        # thick 4, step 3: [0, 4) -> -7 / 4 = -1, short [3, 5) -> 3 / 2 = 1 (3 / 4 would say 0)
        assert slabs_np.slabs(line.reshape(shape), "mean", 4, 3, axis).reshape(-1).tolist() == [-1, 1]
    big = np.full((3, 2, 2), 32767, dtype=np.int16)
    assert np.array_equal(slabs_np.slabs(big, "mean", 2, 1, "axial"), np.full((2, 2, 2), 32767, dtype=np.int16))


def test_predict_thin_slab_arguments():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import predict
    base = ["--weights", "g.pth", "--input", "in.npy", "--output", "out.npy"]
    o = predict.parse_args(base)
    assert o.sts_dir is None and o.sts is None      # nothing new happens
    o = predict.parse_args(base + ["--sts-dir", "sts", "--sts-thick", "10"])
    assert o.sts == {"thick": {"axial": 10, "coronal": 10, "sagittal": 10}, "step": {"axial": 10, "coronal": 10, "sagittal": 10},
                     "mode": "max", "axes": ("axial", "coronal", "sagittal")}
    o = predict.parse_args(base + ["--sts-dir", "sts", "--sts-thick", "10,8,6", "--sts-step", "5", "--sts-axes", "sagittal,axial",
                                   "--mip-mode", "mean"])
    assert o.sts == {"thick": {"axial": 10, "sagittal": 6}, "step": {"axial": 5, "sagittal": 5}, "mode": "mean",
                     "axes": ("axial", "sagittal")}
    # a step above the thickness of an axis that is not kept does not matter
    o = predict.parse_args(base + ["--sts-dir", "sts", "--sts-thick", "10,2,6", "--sts-step", "5,5,5", "--sts-axes", "axial"])
    assert o.sts["thick"] == {"axial": 10} and o.sts["step"] == {"axial": 5}
    for bad in (["--sts-dir", "sts"],                                                   # no thickness
                ["--sts-thick", "3"],                                                   # no directory
                ["--sts-step", "3"],
                ["--sts-dir", "sts", "--sts-thick", "0"],
                ["--sts-dir", "sts", "--sts-thick", "3,4"],                             # one count or three
                ["--sts-dir", "sts", "--sts-thick", "three"],
                ["--sts-dir", "sts", "--sts-thick", "3", "--sts-step", "4"],            # step above thick
                ["--sts-dir", "sts", "--sts-thick", "3", "--sts-step", "0"],
                ["--sts-dir", "sts", "--sts-thick", "9,9,2", "--sts-step", "3"],        # above the sagittal thickness
                ["--sts-dir", "sts", "--sts-thick", "3", "--sts-axes", "axial,oblique"],
                ["--sts-dir", "sts", "--sts-thick", "3", "--sts-axes", ""],
                ["--sts-dir", "sts", "--sts-thick", "3", "--sts-axes", "axial,axial"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
