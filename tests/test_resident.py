"""CPU: `ResidentVolume` (cta_gan_amd/infer.py), the whole volume as an object that the four `Volume*` views read -- its
bookkeeping, what `adopt` refuses, a view with `source=` -- and the argument checks those views share.  Nothing here touches a
device: device=None resolves at the first chunk only."""
import numpy as np
import pytest
import torch

N, H, W = 4, 5, 6


def makers():
    """What makes each of the four views on a 4 x 5 x 6 volume, by class name."""
    from cta_gan_amd import infer
    tables = {"tumble": lambda n, h, w: infer.orbit_lines(n, h, w, [0.0], axis="x")}
    return {"VolumeReformatter": lambda **kw: infer.VolumeReformatter(N, H, W, tables, **kw),
            "VolumeRenderer": lambda **kw: infer.VolumeRenderer(N, H, W, tables, shading={}, **kw),
            "VolumeComponents": lambda **kw: infer.VolumeComponents(N, H, W, 100, seeds=[(0, 0, 0)], **kw),
            "VolumeCentreline": lambda **kw: infer.VolumeCentreline(N, H, W, 100, (0, 0, 0), [(3, 4, 5)], **kw)}


def views(**kw):
    return {name: make(**kw) for name, make in makers().items()}


def test_resident_volume_bookkeeping():
    from cta_gan_amd.infer import ResidentVolume
    res = ResidentVolume(N, H, W)
    assert (res.n, res.h, res.w) == (N, H, W) and res.nbytes == 2 * N * H * W
    assert res.volume is None and res.device is None and res.seen.shape == (N,) and (res.seen == 0).all()
    with pytest.raises(RuntimeError, match="SomeView: every slice must have arrived exactly once: 4 of 4 missing, 0 more than once"):
        res.whole("SomeView")
    res.seen[:] = 1
    res.whole("SomeView")
    res.seen[2] = 2
    res.seen[0] = 0
    with pytest.raises(RuntimeError, match="SomeView: every slice must have arrived exactly once: 1 of 4 missing, 1 more than once"):
        res.whole("SomeView")
    res.reset()
    assert (res.seen == 0).all() and res.volume is None
    for bad in ((0, H, W), (N, 0, W), (N, H, 0)):
        with pytest.raises(ValueError, match="at least one voxel"):
            ResidentVolume(*bad)
    with pytest.raises(RuntimeError, match="ResidentVolume: a GPU device is required"):
        ResidentVolume(N, H, W, device="cpu")


def test_resident_volume_refuses_a_chunk_with_the_words_of_the_views():
    from cta_gan_amd.infer import ResidentVolume
    res = ResidentVolume(N, H, W)
    for chunk, n0 in ((torch.zeros((2, H, W), dtype=torch.int16), 3), (torch.zeros((2, H, W), dtype=torch.int16), -1),
                      (torch.zeros((2, H, W + 1), dtype=torch.int16), 0), (torch.zeros((2, H, W), dtype=torch.int32), 0)):
        with pytest.raises(RuntimeError, match=r"ResidentVolume: int16 chunk \(2, 5, %d\) at slice %d does not lie in the volume \(4, 5, 6\)"
                           % (chunk.shape[2], n0)):
            res.update(chunk, n0)
        with pytest.raises(RuntimeError, match="VolumeRenderer: int16 chunk"):
            res.update(chunk, n0, who="VolumeRenderer")
    res.update(torch.zeros((0, H, W), dtype=torch.int16), 2)      # an empty chunk: nothing arrives, no device is asked for
    assert res.volume is None and res.device is None and (res.seen == 0).all()


def test_adopt_refuses_what_is_not_the_whole_volume_on_a_gpu():
    from cta_gan_amd.infer import ResidentVolume
    res = ResidentVolume(N, H, W)
    whole = torch.zeros((N, H, W), dtype=torch.int16)
    for bad, got in ((whole.int(), "torch.int32"), (torch.zeros((N, H, W + 1), dtype=torch.int16), r"\(4, 5, 7\)"),
                     (whole, "device\\(type='cpu'\\)"), (torch.zeros((N, W, H), dtype=torch.int16).transpose(1, 2), "False"),
                     (whole.numpy(), "array"), (None, "None")):
        with pytest.raises(RuntimeError, match=r"ResidentVolume: adopt: a contiguous int16 tensor \(4, 5, 6\) on a GPU expected, got .*" + got):
            res.adopt(bad)
    assert res.volume is None and (res.seen == 0).all()


def test_a_view_reads_its_source():
    from cta_gan_amd.infer import ResidentVolume
    alone = views()
    res = ResidentVolume(N, H, W)
    shared = views(source=res)
    for name, view in shared.items():
        assert view.source is res and not view.owns and view.volume is None and view.device is None
        assert view.nbytes == alone[name].nbytes - 2 * N * H * W and alone[name].owns and alone[name].source is not res
        with pytest.raises(RuntimeError, match=name + ": update: the volume is fed through its source"):
            view.update(torch.zeros((1, H, W), dtype=torch.int16), 0)
        with pytest.raises(RuntimeError, match=name + ": every slice must have arrived exactly once: 4 of 4 missing"):
            view.result()
        res.seen[:] = 1
        view.reset()      # the source is not the view's to reset
        assert (res.seen == 1).all()
        res.reset()
    for bad in (ResidentVolume(N, H, W + 1), ResidentVolume(N + 1, H, W), torch.zeros((N, H, W), dtype=torch.int16), "cta"):
        for name, make in makers().items():
            with pytest.raises(ValueError, match=name + r": source: a ResidentVolume of \(4, 5, 6\) expected"):
                make(source=bad)


def test_the_views_own_volume_is_a_resident_volume():
    from cta_gan_amd.infer import ResidentVolume
    for name, view in views().items():
        assert isinstance(view.source, ResidentVolume) and (view.source.n, view.source.h, view.source.w) == (N, H, W)
        assert view.volume is None and view.device is None and (view.source.seen == 0).all()
        view.source.seen[:] = 1
        view.reset()
        assert (view.source.seen == 0).all()


def test_the_shared_checks_refuse_what_the_views_refused():
    from cta_gan_amd import infer
    for bad in (None, (1, 2, 3), (5, 4), 1.5, 40000, (-40000, 5), True, (1, 2.0)):
        with pytest.raises(ValueError, match="Who: threshold: "):
            infer._band("Who", bad)
    assert infer._band("Who", 7) == (7, 32767) and infer._band("Who", [np.int16(-5), 300]) == (-5, 300)
    for bad in ([], [(0, 0)], [(4, 0, 0)], [(0, 5, 0)], [(0, 0, 6)], [(-1, 0, 0)], [(0.5, 0, 0)]):
        with pytest.raises(ValueError, match="Who: seeds: "):
            infer._voxel_indices("Who", "seeds", bad, N, H, W)
    assert infer._voxel_indices("Who", "seeds", [(0, 0, 0), (3, 4, 5)], N, H, W).tolist() == [0, 119]
    with pytest.raises(ValueError, match="Who: ends: 2 .. 3 integer"):
        infer._voxel_indices("Who", "ends", [(0, 0, 0)] * 4, N, H, W, 2, 3)
    for bad in (0, 65, True, 2.0, "3", None):
        with pytest.raises(ValueError, match="Who: top: an integer in 1 .. 64 expected, got"):
            infer._int_in("Who", "top", bad, 1, 64)
    with pytest.raises(ValueError, match="Who: oversample: an integer >= 1 expected, got 0"):
        infer._int_in("Who", "oversample", 0, 1)
    assert infer._int_in("Who", "top", np.int64(64), 1, 64) == 64 and infer._int_in("Who", "oversample", 9, 1) == 9


def test_the_option_dicts_of_the_translator():
    from cta_gan_amd.infer import _option_dict
    assert _option_dict("x_options", None, ("a",), needs=("x", None, "table")) == {}
    assert _option_dict("x_options", {"a": 1}, ("a", "b"), needs=("x", {"t": 0}, "table")) == {"a": 1}
    with pytest.raises(ValueError, match="SeriesTranslator: x_options need x"):
        _option_dict("x_options", {"a": 1}, ("a",), needs=("x", None, "table"))
    with pytest.raises(ValueError, match="SeriesTranslator: x needs at least one table"):
        _option_dict("x_options", None, ("a",), needs=("x", {}, "table"))
    with pytest.raises(ValueError, match="SeriesTranslator: x_options .*: a dict with any of \\('a',\\) expected"):
        _option_dict("x_options", {"c": 1}, ("a",), needs=("x", {"t": 0}, "table"))
    with pytest.raises(ValueError, match="SeriesTranslator: y .*: a dict with 'lo', any of \\('lo', 'b'\\) expected"):
        _option_dict("y", {"b": 1}, ("lo", "b"), ("lo",))
