"""LPIPS (AlexNet) -- CPU side: the float64 restatement's self-checks (tests/lpips_ref.py) and the weight loader
(cta_gan_amd/lpips.py).  No GPU, no compute call into the library."""
import pytest
import torch

import lpips_ref
from cta_gan_amd import synth
from cta_gan_amd.lpips import CONVS, KEYS, LPIPS, feature_sizes

SD = synth.lpips_state_dict(seed=0)

# H x W -> (f1, f2, f3..f5) map sizes
SIZES = {(31, 35): ((7, 8), (3, 3), (1, 1)), (64, 64): ((15, 15), (7, 7), (3, 3)), (67, 95): ((16, 23), (7, 11), (3, 5)),
         (131, 259): ((32, 64), (15, 31), (7, 15)), (512, 512): ((127, 127), (63, 63), (31, 31))}


def test_restatement_is_zero_on_identical_inputs():
    x, _ = lpips_ref.make_pairs(64, 64)
    for dtype in (torch.float64, torch.float32):
        assert torch.equal(lpips_ref.lpips(x, x.clone(), SD, dtype), torch.zeros(3, 5, dtype=dtype))


@pytest.mark.parametrize("hw", [(31, 35), (64, 64), (67, 95)])
def test_folded_stem_equals_the_three_channel_stem(hw):
    """The two-plane stem (image, ones; both zero padded) against scaling layer + 3-channel conv1 in float64: every feature map and
    every per-layer value within 1e-12 -- the border, where the shift term must vanish, included (the top rows are -1, not 0)."""
    x, y = lpips_ref.make_pairs(*hw)
    a, b = lpips_ref.features(x, SD), lpips_ref.features_folded(x, SD)
    for fa, fb in zip(a, b):
        assert float((fa - fb).abs().max()) <= 1e-12
    va, vb = lpips_ref.lpips(x, y, SD), lpips_ref.lpips(x, y, SD, folded=True)
    assert float((va - vb).abs().max()) <= 1e-12
    assert float(va.min()) > 0


@pytest.mark.parametrize("hw", sorted(SIZES))
def test_map_sizes(hw):
    f1, f2, f3 = SIZES[hw]
    assert feature_sizes(*hw) == [f1, f2, f3, f3, f3]
    if hw[0] <= 131:
        feats = lpips_ref.features(torch.zeros(1, *hw), SD, torch.float32)
        assert [tuple(f.shape[2:]) for f in feats] == [f1, f2, f3, f3, f3]
        assert [f.shape[1] for f in feats] == [c[0] for c in CONVS]


def test_float32_restatement_stays_near_float64():
    x, y = lpips_ref.make_pairs(64, 64)
    v64, v32 = lpips_ref.lpips(x, y, SD), lpips_ref.lpips(x, y, SD, torch.float32).double()
    assert float(((v32 - v64).abs() / v64).max()) < 1e-5


def _same(p, q):
    return sorted(p) == sorted(q) and all(torch.equal(p[k], q[k]) for k in p)


def test_loader_both_formats_give_identical_packs(tmp_path):
    full = LPIPS().load_state_dict(SD)
    alex, lins = synth.lpips_state_dict(seed=0, fmt="two")
    two = LPIPS().load_two(alex, lins)
    assert _same(full.params, two.params)
    assert sorted(full.params) == sorted(["stem_w"] + ["w%d" % k for k in range(2, 6)] + ["b%d" % k for k in range(1, 6)]
                                         + ["lin%d" % k for k in range(5)])
    assert full.params["stem_w"].shape == (64, 242) and full.params["stem_w"].dtype == torch.float32
    assert [full.params["lin%d" % k].shape[0] for k in range(5)] == [c[0] for c in CONVS]
    # through files, as config['lpips_weights'] names them
    torch.save(SD, tmp_path / "full.pth")
    torch.save(alex, tmp_path / "alexnet.pth")
    torch.save(lins, tmp_path / "lins.pth")
    assert _same(LPIPS.from_files(str(tmp_path / "full.pth")).params, full.params)
    assert _same(LPIPS.from_files(alexnet=str(tmp_path / "alexnet.pth"), lins=str(tmp_path / "lins.pth")).params, full.params)
    assert _same(LPIPS.from_config({"alexnet": str(tmp_path / "alexnet.pth"), "lins": str(tmp_path / "lins.pth")}).params, full.params)
    # the scaling layer's keys are optional (the constants are the default) and override when present
    bare = {k: v for k, v in SD.items() if not k.startswith("scaling_layer") and not k.startswith("lins.")}
    assert _same(LPIPS().load_state_dict(bare).params, full.params)
    other = dict(SD)
    other[KEYS["scale"]] = SD[KEYS["scale"]] * 2
    assert torch.allclose(LPIPS().load_state_dict(other).params["stem_w"][:, :121] * 2, full.params["stem_w"][:, :121], rtol=1e-6)


def test_loader_names_the_offending_key():
    for key in (KEYS["full_conv"][2] + ".weight", KEYS["full_conv"][0] + ".bias", KEYS["lin"][3]):
        sd = dict(SD)
        del sd[key]
        with pytest.raises(ValueError) as e:
            LPIPS().load_state_dict(sd)
        assert key in str(e.value) and "expected shape" in str(e.value)
    sd = dict(SD)
    sd[KEYS["full_conv"][1] + ".weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError) as e:
        LPIPS().load_state_dict(sd)
    assert KEYS["full_conv"][1] + ".weight" in str(e.value) and "(192, 64, 5, 5)" in str(e.value)
    sd = dict(SD)
    sd[KEYS["lin"][4]] = torch.zeros(256)
    with pytest.raises(ValueError) as e:
        LPIPS().load_state_dict(sd)
    assert KEYS["lin"][4] in str(e.value) and "(1, 256, 1, 1)" in str(e.value)
    sd = dict(SD)
    sd[KEYS["lin_duplicate"][1]] = SD[KEYS["lin"][1]] + 1
    with pytest.raises(ValueError) as e:
        LPIPS().load_state_dict(sd)
    assert KEYS["lin_duplicate"][1] in str(e.value)
    alex, lins = synth.lpips_state_dict(seed=0, fmt="two")
    del alex["features.6.bias"]
    with pytest.raises(ValueError) as e:
        LPIPS().load_two(alex, lins)
    assert "features.6.bias" in str(e.value)


def test_unsupported_arguments_raise():
    for kw in (dict(net="vgg"), dict(net="squeeze"), dict(spatial=True), dict(lpips=False)):
        with pytest.raises(ValueError):
            LPIPS(**kw)
    m = LPIPS().load_state_dict(SD)
    with pytest.raises(ValueError):
        m.forward(torch.zeros(1, 64, 64), torch.zeros(1, 64, 64), normalize=True)
    with pytest.raises(RuntimeError):      # CPU tensors: no fallback
        m.forward(torch.zeros(1, 64, 64), torch.zeros(1, 64, 64))
    with pytest.raises(RuntimeError):
        LPIPS().forward(torch.zeros(1, 64, 64), torch.zeros(1, 64, 64))
