"""GPU: the plumbing the eight series displays share (cta_gan_amd/infer.py: the view protocol of SeriesProjector, SeriesRotator,
SeriesSlabs, SeriesRenderer, VolumeReformatter, VolumeRenderer, VolumeComponents and VolumeCentreline, the one chunk loop of the
*_volume functions, the one table of views, the one resident volume per source and the one staging path of SeriesTranslator) and the
argument checks the bindings of a family share in ops.py.  What every display computes is pinned by its own file against a numpy
restatement; here the translator's views are held against the stand-alone functions, reuse against rebuilding, a switched-off
display against a translator that never heard of it, and the launches of a call against the list of the code before the views
shared their volume.  Exact integers: np.array_equal."""
import numpy as np
import pytest
import torch

import components_np as cnp
from test_rotate_gpu import make_generator, synthetic_hu

pytestmark = pytest.mark.gpu

SHAPES = ((5, 64, 64), (3, 48, 40))      # at batch 2 the last chunk is short; the second is resized to the generator's 64 x 64
DISPLAYS = ("projections", "rotation", "slabs", "render", "reformat", "render3d", "vessels", "centreline")
WHOLE = ("reformat", "render3d", "vessels", "centreline")      # the displays that read the whole volume

# The entry points that pass _lib.check during one all-displays call on the first volume (bf16, batch 2: three chunks), recorded
# with the code before the whole-volume views shared one resident volume: the chunk copies never were among them, so none may move.
GENERATOR = (["ctg_series_inputs", "ctg_conv_smallcin"] + ["ctg_in_finalize", "ctg_in_apply", "ctg_conv_igemm"] * 3
             + ["ctg_conv_igemm"] * 17 + ["ctg_conv_igemm_classes", "ctg_in_finalize", "ctg_in_apply"] * 2 + ["ctg_conv_tail7"])
PER_CHUNK = GENERATOR + ["ctg_export_slices", "ctg_subtract_slices", "ctg_project_accumulate_depth", "ctg_project_rotate_depth",
                         "ctg_project_slabs_inplane", "ctg_project_slabs_inplane", "ctg_project_accumulate_sliding", "ctg_project_render"]
AFTER = (["ctg_components_label", "ctg_components_select", "ctg_components_apply"] + ["ctg_project_finish_depth"] * 3
         + ["ctg_project_finish"] + ["ctg_reformat_lines"] * 2 + ["ctg_render_lines"] * 2
         + ["ctg_centreline_clearance", "ctg_centreline_seed", "ctg_centreline_relax", "ctg_centreline_saturated", "ctg_centreline_trace"]
         + ["ctg_reformat_lines"] * 2)
LAUNCHES = PER_CHUNK * 3 + AFTER


def reformat_tables():
    from cta_gan_amd.infer import oblique_lines, orbit_lines
    return {"planes": lambda n, h, w: oblique_lines(n, h, w, (1, 1, 2), count=3, pitch=2.0, thick=2),
            "tumble": lambda n, h, w: orbit_lines(n, h, w, [0.0, 40.0], axis="x")}


def picks(volumes):
    """(lo, start, ends) for the components and the centreline of every one of `volumes`: the median of the first as the
    threshold, and three voxels that lie in the biggest 26-connected component of the foreground of each."""
    lo = max(1, int(np.percentile(volumes[0], 50)))
    common = None
    for vol in volumes:
        n, h, w = vol.shape
        lab = cnp.label(np.ascontiguousarray(vol), lo, 32767, 26).reshape(-1)
        roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
        members = np.flatnonzero(lab == roots[np.argmax(sizes)])
        zyx = set(zip((members // (h * w)).tolist(), ((members // w) % h).tolist(), (members % w).tolist()))
        common = zyx if common is None else common & zyx
    common = sorted(common)
    assert len(common) > 100
    return lo, common[0], [common[-1], common[len(common) // 2]]


def whole_options(lo, start, ends):
    """(components, centreline): the keyword arguments of the two views beyond their window."""
    return (dict(threshold=lo, largest=2, min_voxels=4, labels=True),
            dict(threshold=lo, start=start, ends=ends, radius=3, aspect=2.0, clearance=True, cpr=dict(cols=9)))


def all_on(pick, **more):
    components, centreline = whole_options(*pick)
    return dict(batch=2, size=64, project="max", slab=2, rotate=3, depth=True, depth_cue=128, slabs={"thick": 3, "step": 2}, render=3,
                reformat=reformat_tables(), render3d=reformat_tables(), render3d_options={"shading": {}}, components=components,
                centreline=centreline, subtract=True, **more)


def standalone(volume, wc, ww, hu, pick, keys=DISPLAYS):
    """What the eight *_volume functions return for `volume` under the options of `all_on`, by the translator's output key."""
    from cta_gan_amd import infer
    components, centreline = whole_options(*pick)
    calls = {"projections": lambda: infer.project_volume(volume, mode="max", slab=2, wc=wc, ww=ww, hu=hu, batch=2, depth=True, cue=128),
             "rotation": lambda: infer.rotate_volume(volume, 3, mode="max", wc=wc, ww=ww, hu=hu, batch=2, depth=True, cue=128),
             "slabs": lambda: infer.slab_volume(volume, 3, step=2, wc=wc, ww=ww, hu=hu, batch=2),
             "render": lambda: infer.render_volume(volume, 3, batch=2, hu=hu),
             "reformat": lambda: infer.reformat_volume(volume, reformat_tables(), wc=wc, ww=ww, hu=hu, batch=2),
             "render3d": lambda: infer.render_lines_volume(volume, reformat_tables(), batch=2, hu=hu, shading={}),
             "vessels": lambda: infer.components_volume(volume, batch=2, wc=wc, ww=ww, hu=hu, **components),
             "centreline": lambda: infer.centreline_volume(volume, batch=2, wc=wc, ww=ww, hu=hu, **centreline)}
    return {key: calls[key]() for key in keys}


def assert_same(got, want, where=""):
    """Two result trees: the same keys, the same kinds, the same bits."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), where
        for k in want:
            assert_same(got[k], want[k], "%s/%s" % (where, k))
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), where
        for k, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, "%s/%d" % (where, k))
    elif want is None:
        assert got is None, where
    else:
        assert type(got) is type(want) and got.dtype == want.dtype and np.array_equal(np.asarray(got), np.asarray(want)), where


def buffers(tree):
    """The tensors of a tree of page-locked buffers."""
    if isinstance(tree, (dict, list)):
        return [t for v in (tree.values() if isinstance(tree, dict) else tree) for t in buffers(v)]
    return [] if tree is None else [tree]


def counted(check, launched):
    return lambda status, what: (launched.append(what), check(status, what))[1]


@pytest.fixture(scope="module")
def run():
    """One translator with every display on, driven over first shape, first shape, second shape, first shape -- with what it held
    after each call and what it launched in the first -- and one that shows the subtraction volume, over both shapes."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib, nets
    from cta_gan_amd.infer import SeriesTranslator
    _lib.load()
    nets.set_default_compute_dtype(torch.bfloat16)
    check, launched = _lib.check, []
    try:
        g = make_generator()
        vols = [synthetic_hu(*shape, seed=11 + i) for i, shape in enumerate(SHAPES)]
        plain = [SeriesTranslator(g, batch=2, size=64, subtract=True)(vol) for vol in vols]
        pick, sub_pick = picks([p["pix"] for p in plain]), picks([p["sub"] for p in plain])
        tr = SeriesTranslator(g, **all_on(pick))
        outs, held = [], []
        for vol in (vols[0], vols[0], vols[1], vols[0]):
            _lib.check = counted(check, launched) if not outs else check
            outs.append(tr(vol))
            _lib.check = check
            held.append({"views": dict(tr._views), "host": {k: buffers(t) for k, t in tr._view_host.items()},
                         "slots": list(tr._in) + [t for slot in tr._out for t in slot.values()], "residents": dict(tr._residents),
                         "volumes": {k: r.volume for k, r in tr._residents.items()}})
        sub_tr = SeriesTranslator(g, **all_on(sub_pick, project_source="sub"))
        return {"g": g, "vols": vols, "plain": plain, "pick": pick, "sub_pick": sub_pick, "outs": outs, "held": held,
                "launched": launched, "sub_outs": [sub_tr(vol) for vol in vols]}
    finally:
        _lib.check = check
        nets.set_default_compute_dtype(torch.float32)


@pytest.mark.parametrize("which", (0, 1))
def test_views_equal_the_standalone_functions(run, which):
    out = run["outs"][2 * which]
    assert sorted(out) == sorted(DISPLAYS + ("pix", "level", "sub", "sub_level")) and out["pix"].shape == SHAPES[which]
    assert list(out)[-len(DISPLAYS):] == list(DISPLAYS)
    want = standalone(out["pix"], 50.0, 400.0, False, run["pick"])
    for key in DISPLAYS:
        assert_same(out[key], want[key], key)
    assert out["vessels"]["stats"][3] >= 1 and (out["centreline"]["counts"] > 1).all()      # (something was kept, something traced)
    out = run["sub_outs"][which]      # the views of the subtraction volume: its own window, a HU difference
    want = standalone(out["sub"], 150.0, 300.0, True, run["sub_pick"])
    for key in DISPLAYS:
        assert_same(out[key], want[key], "sub:" + key)


def test_views_and_buffers_are_kept_for_one_shape_and_replaced_for_another(run):
    first, again, other, back = run["held"]
    assert sorted(first["views"]) == sorted(first["host"]) == sorted(DISPLAYS)
    for key in DISPLAYS:
        assert again["views"][key] is first["views"][key]
        assert [t.data_ptr() for t in again["host"][key]] == [t.data_ptr() for t in first["host"][key]]
        assert all(t.is_pinned() for t in first["host"][key]) and first["host"][key]
        assert other["views"][key] is not first["views"][key]
        assert (other["views"][key].n, other["views"][key].h, other["views"][key].w) == SHAPES[1]
        assert all(a is not b for a in other["host"][key] for b in first["host"][key])
        assert (back["views"][key].n, back["views"][key].h, back["views"][key].w) == SHAPES[0]
    assert [t.data_ptr() for t in again["slots"]] == [t.data_ptr() for t in first["slots"]]
    assert all(a is not b and a.shape[1:] == SHAPES[1][1:] for a, b in zip(other["slots"], first["slots"]))
    outs = run["outs"]
    assert_same(outs[1], outs[0], "second call")
    assert_same(outs[3], outs[0], "back on the first shape")


def test_the_whole_volume_views_read_one_resident_volume(run):
    from cta_gan_amd.infer import ResidentVolume
    first, again, other, back = run["held"]
    for held, shape in ((first, SHAPES[0]), (other, SHAPES[1])):
        assert list(held["residents"]) == ["cta"] and type(held["residents"]["cta"]) is ResidentVolume
        res = held["residents"]["cta"]
        assert (res.n, res.h, res.w) == shape and tuple(held["volumes"]["cta"].shape) == shape
        for key in WHOLE:
            assert held["views"][key].source is res and not held["views"][key].owns
        assert len({held["views"][key].volume.data_ptr() for key in WHOLE}) == 1
    assert again["residents"]["cta"] is first["residents"]["cta"] and again["volumes"]["cta"] is first["volumes"]["cta"]
    assert other["residents"]["cta"] is not first["residents"]["cta"] and other["volumes"]["cta"] is not first["volumes"]["cta"]
    assert back["residents"]["cta"] is not other["residents"]["cta"]
    assert (first["residents"]["cta"].seen == 1).all()
    for key in ("projections", "rotation", "slabs", "render"):
        assert not hasattr(first["views"][key], "source")


def test_the_launches_of_an_all_displays_call_are_those_of_the_private_copies(run):
    assert run["launched"] == LAUNCHES


def test_two_sources_are_two_resident_volumes(run):
    from cta_gan_amd import nets
    from cta_gan_amd.infer import SeriesTranslator
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        options = all_on(run["pick"], project_source="cta", components_source="sub")
        options["components"] = whole_options(*run["sub_pick"])[0]
        tr = SeriesTranslator(run["g"], **options)
        out = tr(run["vols"][0])
    finally:
        nets.set_default_compute_dtype(torch.float32)
    assert sorted(tr._residents) == ["cta", "sub"] and tr._residents["cta"].volume.data_ptr() != tr._residents["sub"].volume.data_ptr()
    assert tr._views["vessels"].source is tr._residents["sub"]
    assert all(tr._views[key].source is tr._residents["cta"] for key in ("reformat", "render3d", "centreline"))
    assert np.array_equal(tr._residents["cta"].volume.cpu().numpy(), out["pix"])
    assert np.array_equal(tr._residents["sub"].volume.cpu().numpy(), out["sub"])
    assert_same(out["vessels"], run["sub_outs"][0]["vessels"], "vessels of sub")
    for key in ("reformat", "render3d", "centreline", "projections"):
        assert_same(out[key], run["outs"][0][key], key)


def test_the_cleaned_volume_is_read_where_it_is(run, monkeypatch):
    from cta_gan_amd import infer, nets
    pix = run["plain"][0]["pix"]
    cleaned = infer.components_volume(pix, batch=2, **whole_options(*run["pick"])[0])["values"]
    # the centreline keeps the components' threshold: it lies above the fill, so the kept components are the foreground it sees
    pick = (run["pick"][0],) + picks([cleaned])[1:]
    results = []
    monkeypatch.setattr(infer.VolumeComponents, "result", (lambda f: lambda view: (results.append(f(view)), results[-1])[1])(
        infer.VolumeComponents.result))
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        tr = infer.SeriesTranslator(run["g"], **all_on(pick, project_source="vessels"))
        outs = []
        for call in range(2):
            outs.append(tr(run["vols"][0]))
            assert len(results) == call + 1 and sorted(tr._residents) == ["cta", "vessels"]
            assert tr._residents["vessels"].volume.data_ptr() == results[-1]["values"].data_ptr()
            assert tr._views["vessels"].source is tr._residents["cta"]
            assert all(tr._views[key].source is tr._residents["vessels"] for key in ("reformat", "render3d", "centreline"))
    finally:
        nets.set_default_compute_dtype(torch.float32)
    out = outs[0]
    assert np.array_equal(out["vessels"]["values"], cleaned) and (out["vessels"]["values"] != pix).any()
    want = standalone(out["vessels"]["values"], 50.0, 400.0, False, pick, keys=[key for key in DISPLAYS if key != "vessels"])
    for key in want:
        assert_same(out[key], want[key], "vessels:" + key)
    assert_same(outs[1], outs[0], "second call")


def test_adopt_takes_the_tensor_and_refuses_what_it_cannot_read(run):
    from cta_gan_amd import infer
    vol = torch.from_numpy(synthetic_hu(4, 8, 8, seed=5)).cuda()
    res = infer.ResidentVolume(4, 8, 8)
    for bad in (vol.int(), vol[:, :, :7], vol[:3], vol.cpu(), vol.transpose(1, 2), vol.repeat_interleave(2, dim=2)[:, :, ::2]):
        with pytest.raises(RuntimeError, match="ResidentVolume: adopt"):
            res.adopt(bad)
    res.adopt(vol)
    assert res.volume is vol and res.device == vol.device and (res.seen == 1).all()
    view = infer.VolumeReformatter(4, 8, 8, {"a": lambda n, h, w: infer.oblique_lines(n, h, w, (0, 0, 1), count=4)}, source=res)
    assert view.tables is None and view.volume is vol
    assert np.array_equal(view.result()["a"]["values"].cpu().numpy(), vol.cpu().numpy()) and view.tables is not None
    res.update(vol[:2], 0)      # never into the adopted tensor
    assert res.volume is not vol and res.seen.tolist() == [2, 2, 1, 1]
    res.adopt(vol)
    res.reset()
    assert res.volume is None and (res.seen == 0).all()
    before = vol.clone()
    for fn in (lambda v: infer.reformat_volume(v, {"a": lambda n, h, w: infer.oblique_lines(n, h, w, (0, 0, 1))}),
               lambda v: infer.components_volume(v, 0), lambda v: infer.centreline_volume(v, -2000, (0, 0, 0), [(3, 7, 7)])):
        fn(vol)
    assert torch.equal(vol, before)      # a volume that is read where it is comes back as it was


def test_all_displays_off_is_a_translator_without_displays(run, monkeypatch):
    from cta_gan_amd import _lib, nets
    from cta_gan_amd.infer import SeriesTranslator
    launched = []
    monkeypatch.setattr(_lib, "check", counted(_lib.check, launched))
    nets.set_default_compute_dtype(torch.bfloat16)
    try:
        seen = []
        for kw in ({}, dict(project=None, slab=None, rotate=None, slabs=None, depth=False, render=None, reformat=None, subtract=False,
                            render3d=None, components=None, centreline=None)):
            tr = SeriesTranslator(run["g"], batch=2, size=64, **kw)
            del launched[:]
            outs = [tr(vol) for vol in run["vols"]]
            seen.append((set(launched), outs))
            assert tr._views == {} and tr._view_host == {} and tr._displays == {} and sorted(tr._out[0]) == ["level", "pix"]
            assert tr._residents == {}
            assert all(sorted(out) == ["level", "pix"] for out in outs)
        assert seen[0][0] == seen[1][0] and not any(word in what for what in seen[0][0] for word in (
            "project", "reformat", "subtract", "render_lines", "components", "centreline"))
        for got, want, shown in zip(seen[1][1], seen[0][1], (run["outs"][0], run["outs"][2])):
            assert_same(got, want)
            assert_same(got, {"pix": shown["pix"], "level": shown["level"]})      # and the displays do not touch the pixels
    finally:
        nets.set_default_compute_dtype(torch.float32)


def test_every_view_refuses_a_chunk_outside_the_volume_and_a_cpu_device(run):
    from cta_gan_amd import infer
    n, h, w = 4, 8, 8
    tables = {"a": lambda n, h, w: infer.oblique_lines(n, h, w, (0, 0, 1))}
    make = {"SeriesProjector": lambda **kw: infer.SeriesProjector(n, h, w, **kw),
            "SeriesSlabs": lambda **kw: infer.SeriesSlabs(n, h, w, 2, **kw),
            "SeriesRotator": lambda **kw: infer.SeriesRotator(n, h, w, [0.0], **kw),
            "SeriesRenderer": lambda **kw: infer.SeriesRenderer(n, h, w, [0.0], **kw),
            "VolumeReformatter": lambda **kw: infer.VolumeReformatter(n, h, w, tables, **kw),
            "VolumeRenderer": lambda **kw: infer.VolumeRenderer(n, h, w, tables, **kw),
            "VolumeComponents": lambda **kw: infer.VolumeComponents(n, h, w, 100, **kw),
            "VolumeCentreline": lambda **kw: infer.VolumeCentreline(n, h, w, 100, (0, 0, 0), [(3, 7, 7)], **kw)}
    for name, ctor in make.items():
        with pytest.raises(RuntimeError, match="GPU device"):
            ctor(device="cpu")
        view = ctor()
        for shape, n0 in (((2, h, w), 3), ((2, h, w), -1), ((2, h, w + 1), 0), ((2, h - 1, w), 0), ((n + 1, h, w), 0)):
            with pytest.raises(RuntimeError, match=name + ".*does not lie in the volume"):
                view.update(torch.zeros(shape, dtype=torch.int16, device="cuda"), n0)
        view.update(torch.zeros((2, h, w), dtype=torch.int16, device="cuda"), 2)      # the last chunk that does


def test_every_volume_function_refuses_another_dtype_and_an_empty_batch(run):
    from cta_gan_amd import infer
    vol = synthetic_hu(3, 8, 8, seed=5)
    tables = {"a": lambda n, h, w: infer.oblique_lines(n, h, w, (0, 0, 1))}
    calls = {"project_volume": lambda v, **kw: infer.project_volume(v, **kw),
             "slab_volume": lambda v, **kw: infer.slab_volume(v, 2, **kw),
             "rotate_volume": lambda v, **kw: infer.rotate_volume(v, 2, **kw),
             "render_volume": lambda v, **kw: infer.render_volume(v, 2, **kw),
             "reformat_volume": lambda v, **kw: infer.reformat_volume(v, tables, **kw),
             "render_lines_volume": lambda v, **kw: infer.render_lines_volume(v, tables, **kw),
             "components_volume": lambda v, **kw: infer.components_volume(v, 0, **kw),
             "centreline_volume": lambda v, **kw: infer.centreline_volume(v, -2000, (0, 0, 0), [(2, 7, 7)], **kw)}
    for name, call in calls.items():
        for bad in (vol.astype(np.int32), torch.from_numpy(vol).int(), torch.from_numpy(vol).cuda().int(), vol[0], [[1]]):
            with pytest.raises(RuntimeError, match=name):
                call(bad)
        with pytest.raises(ValueError, match=name):
            call(vol, batch=0)
        for v in (vol, torch.from_numpy(vol), torch.from_numpy(vol).cuda()):      # and each kind comes back as its own
            leaf = buffers(call(v, batch=2))[0]
            assert type(leaf) is type(v) and (not torch.is_tensor(v) or leaf.device == v.device)


def test_accumulate_refuses_what_is_not_a_tensor(run):
    from cta_gan_amd import ops
    acc = torch.zeros((1, 2, 2), dtype=torch.int32, device="cuda")
    for pix in ([[[1, 2], [3, 4]]], np.zeros((1, 2, 2), dtype=np.int16), None):
        with pytest.raises(RuntimeError, match="project_accumulate"):
            ops.project_accumulate(pix, 0, 1, "max", axial=acc)
    with pytest.raises(RuntimeError, match="project_accumulate"):
        ops.project_accumulate(torch.zeros((1, 2, 2), dtype=torch.int16, device="cuda"), 0, 1, "max", axial=[[0]])
    with pytest.raises(RuntimeError, match="project_finish"):
        ops.project_finish(np.zeros((2, 2), dtype=np.int32), "max")
