"""CPU: the numpy restatement of the connected components (tests/components_np.py) against scipy.ndimage.label where scipy is
installed, the selection order on ties, and the host-side argument checks of VolumeComponents, SeriesTranslator(components=...)
and predict.py's --cc options.  The kernels themselves: tests/test_components_gpu.py."""
import numpy as np
import pytest

import components_np as cnp

LO, HI = cnp.LO, cnp.HI
STRUCTURE_RANK = {6: 1, 18: 2, 26: 3}


def canonical(labelled, count):
    """scipy's labels 1 .. count -> the smallest linear index per label, -1 on background."""
    flat = labelled.reshape(-1)
    first = np.full(count + 1, -1, dtype=np.int64)
    idx = np.flatnonzero(flat > 0)
    first[flat[idx][::-1]] = idx[::-1]      # the last write wins: the smallest index
    return first[flat].astype(np.int32).reshape(labelled.shape)


@pytest.mark.parametrize("conn", (6, 18, 26))
def test_restatement_equals_scipy(conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(3, STRUCTURE_RANK[conn])
    density = {6: 0.31, 18: 0.14, 26: 0.10}[conn]
    volumes = [cnp.random_field((9, 33, 131), density, 1), cnp.random_field((3, 15, 37), density, 2), cnp.random_field((5, 9, 67), 0.5, 3),
               cnp.snake((9, 33, 131)), cnp.snake((5, 9, 67)), cnp.snake((3, 5, 7)), cnp.snake((9, 33, 131), (4, 16, 65)),
               cnp.checkerboard((4, 6, 10)), cnp.random_field((1, 1, 1), 1.0, 4), cnp.random_field((2, 3, 4), 0.0, 5)]
    for vol in volumes:
        got = cnp.label(vol, LO, HI, conn)
        labelled, count = ndimage.label((vol >= LO) & (vol <= HI), structure=structure)
        assert np.array_equal(got, canonical(labelled, count)), (conn, vol.shape)
        size = cnp.sizes(got)
        assert int((size > 0).sum()) == count and int(size.sum()) == int((got >= 0).sum())
        roots = np.flatnonzero(size.reshape(-1) > 0)
        assert np.array_equal(got.reshape(-1)[roots], roots)      # a root labels itself


def test_the_documented_counts_of_the_test_volumes():
    for conn in (6, 18, 26):
        for shape in ((5, 9, 67), (9, 17, 131), (3, 5, 7)):
            assert int((cnp.sizes(cnp.label(cnp.snake(shape), LO, HI, conn)) > 0).sum()) == 1
        cut = cnp.label(cnp.snake((9, 17, 131), (4, 8, 65)), LO, HI, conn)
        assert int((cnp.sizes(cut) > 0).sum()) == 2
    board = cnp.checkerboard((4, 6, 10))
    assert [int((cnp.sizes(cnp.label(board, LO, HI, c)) > 0).sum()) for c in (6, 18, 26)] == [120, 1, 1]
    assert len(cnp.offsets(6)) == 3 and len(cnp.offsets(18)) == 9 and len(cnp.offsets(26)) == 13


def test_selection_order_on_ties_and_seeds():
    vol = np.zeros((3, 6, 12), dtype=np.int16)
    vol[0, 0, 0:3] = vol[0, 2, 4:7] = vol[2, 5, 9:12] = 1500      # three of 3 voxels: roots 0, 28, 213
    vol[1, 3, 0:5] = 1500                                        # one of 5: root 108
    vol[2, 0, 0] = 1500                                          # one of 1: root 144
    lab = cnp.label(vol, LO, HI, 6)
    keep, top, stats = cnp.select(lab, ntop=6)
    assert top.tolist() == [[108, 5], [0, 3], [28, 3], [213, 3], [144, 1], [-1, 0]]
    assert stats.tolist() == [15, 5, 5, 5, 15, 0, 0, 0] and int(keep.sum()) == 5
    keep, top, stats = cnp.select(lab, largest=2, ntop=3)
    assert top.tolist() == [[108, 5], [0, 3], [-1, 0]] and stats.tolist() == [15, 5, 5, 2, 8, 0, 0, 0]
    assert np.flatnonzero(keep.reshape(-1)).tolist() == [0, 108]
    keep, top, stats = cnp.select(lab, min_voxels=3, seeds=[30, 29, 215, 500, -1], largest=1, ntop=2)
    assert stats.tolist() == [15, 5, 2, 1, 3, 2, 0, 0] and top.tolist() == [[28, 3], [-1, 0]]
    out = cnp.apply(vol, lab, keep, False, -7)
    assert (out[0, 2, 4:7] == 1500).all() and int((out == -7).sum()) == vol.size - 3
    out = cnp.apply(vol, lab, keep, True, -7)
    assert int((out == -7).sum()) == 12 and int((out == 0).sum()) == vol.size - 15


def test_root_voxel():
    from cta_gan_amd.infer import root_voxel
    assert root_voxel(0, 5, 7) == (0, 0, 0) and root_voxel((3 * 5 + 4) * 7 + 6, 5, 7) == (3, 4, 6)
    z, y, x = root_voxel(np.array([0, 34, 35, 2 ** 31 - 1]), 5, 7)
    assert z.tolist() == [0, 0, 1, (2 ** 31 - 1) // 35] and y.tolist()[:3] == [0, 4, 0] and x.tolist()[:3] == [0, 6, 0]
    for bad in ((-1, 5, 7), (3, 0, 7), (3, 5, 0), (np.array([4, -1]), 5, 7)):
        with pytest.raises(ValueError):
            root_voxel(*bad)


def test_refusals_that_need_no_gpu():
    from cta_gan_amd import ops
    from cta_gan_amd.infer import PROJECT_SOURCES, SeriesTranslator, VolumeComponents
    assert ops.COMPONENTS_TILE == (4, 16, 64) and ops.COMPONENTS_MAX_TOP == 64 and "vessels" in PROJECT_SOURCES
    for kw in (dict(threshold=None), dict(threshold=(1, 2, 3)), dict(threshold=(5, 4)), dict(threshold=1.5), dict(threshold=40000),
               dict(threshold=(-40000, 5)), dict(connectivity=8), dict(connectivity="26"), dict(min_voxels=0), dict(largest=-1),
               dict(largest=65), dict(top=65), dict(top=-1), dict(largest=True), dict(fill=40000), dict(seeds=[]),
               dict(seeds=[(0, 0)]), dict(seeds=[(4, 0, 0)]), dict(seeds=[(0, 5, 0)]), dict(seeds=[(0, 0, 6)]), dict(seeds=[(-1, 0, 0)]),
               dict(seeds=[(0.5, 0, 0)])):
        with pytest.raises(ValueError):
            VolumeComponents(4, 5, 6, **{"threshold": 100, **kw})
    for shape in ((0, 5, 6), (4097, 5, 6), (4, 5, 4097), (4096, 4096, 128)):
        with pytest.raises(ValueError):
            VolumeComponents(*shape, 100)
    view = VolumeComponents(4, 5, 6, (100, 200), seeds=[(0, 0, 0), (3, 4, 5)], hu=True)
    assert (view.lo, view.hi, view.fill) == (100, 200, -1024) and view.seeds_host.tolist() == [0, 119]
    assert view.nbytes == (11 + 3) * 120 + 4 * (8 + 16) + 8
    assert VolumeComponents(4, 5, 6, 7, level=False, top=0).nbytes == (11 + 2) * 120 + 32
    with pytest.raises(RuntimeError, match="exactly once"):
        view.result()      # before any slice has arrived
    comp = {"threshold": 100}
    for kw in (dict(components_source="sub"),                                       # a source without components
               dict(project_source="vessels"),                                      # "vessels" without components
               dict(components={"min_voxels": 3}),                                  # no threshold
               dict(components={"threshold": 1, "angle": 3}),                       # an unknown option
               dict(components=comp, components_source="sub"),                      # "sub" without subtract
               dict(components=comp, components_source="vessels"),
               dict(components=comp, project_source="sub")):
        with pytest.raises(ValueError):
            SeriesTranslator(None, **kw)


def test_predict_options():
    import predict
    base = ["--weights", "w", "--input", "i", "--output", "o"]
    o = predict.parse_args(base)
    assert o.cc is None and o.cc_output is None and o.mip_source == "cta"      # nothing new happens
    o = predict.parse_args(base + ["--cc-output", "v.npy", "--cc-threshold", "40", "--mip-dir", "mip", "--mip-source", "vessels"])
    assert o.cc == {"threshold": (40, 32767), "connectivity": 26, "min_voxels": 1, "largest": 0, "seeds": None, "background": False,
                    "level": False, "labels": False, "top": 8} and o.cc_source is None and o.mip_source == "vessels"
    o = predict.parse_args(base + ["--cc-output", "v.npy", "--cc-threshold=-5,300", "--cc-connectivity", "6", "--cc-min-voxels", "9",
                                   "--cc-largest", "3", "--cc-seed", "1,2,3", "--cc-seed", "4,5,6", "--cc-despeckle", "--cc-level-dir", "lv",
                                   "--cc-labels", "l.npy", "--sub-output", "s.npy", "--cc-source", "sub"])
    assert o.cc == {"threshold": (-5, 300), "connectivity": 6, "min_voxels": 9, "largest": 3, "seeds": [(1, 2, 3), (4, 5, 6)],
                    "background": True, "level": True, "labels": True, "top": 8} and o.cc_source == "sub"
    for bad in (["--mip-source", "vessels"], ["--cc-threshold", "40"], ["--cc-seed", "1,2,3"], ["--cc-despeckle"],
                ["--cc-output", "v.npy"], ["--cc-output", "v.npy", "--cc-threshold", "5,4"],
                ["--cc-output", "v.npy", "--cc-threshold", "x"], ["--cc-output", "v.npy", "--cc-threshold", "1,2,3"],
                ["--cc-output", "v.npy", "--cc-threshold", "40", "--cc-connectivity", "8"],
                ["--cc-output", "v.npy", "--cc-threshold", "40", "--cc-min-voxels", "0"],
                ["--cc-output", "v.npy", "--cc-threshold", "40", "--cc-largest", "65"],
                ["--cc-output", "v.npy", "--cc-threshold", "40", "--cc-seed", "1,2"],
                ["--cc-output", "v.npy", "--cc-threshold", "40", "--cc-seed", "1,-2,3"],
                ["--cc-output", "v.npy", "--cc-threshold", "40", "--cc-source", "sub"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
