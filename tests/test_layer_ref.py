"""CPU checks of tests/layer_ref.py: every case of the table meets the conditions of the exactness argument, sits on the dispatch
path the table says (the pure-Python predicates of cta_gan_amd.ops), and the float64 reference reproduces torch's float32
autograd.  Runs anywhere; the engine itself is driven through the table in tests/test_layer_glue_exact_gpu.py."""
import dataclasses

import numpy as np
import pytest
import torch

import layer_ref as L

FP32_TOL = 4e-4      # GTOL[fp32] of tests/test_kernels_gpu.py (its module is GPU-only: the figure is repeated here)


@pytest.mark.parametrize("name", list(L.CASES))
def test_case_meets_the_exactness_conditions(name):
    case = L.CASES[name]
    rep = L.check_case(case)
    print(name, rep)
    if case.exact:
        assert rep["S_max"] < 2 ** 24
    b, c, h, w = case.shape
    assert 1 <= b <= 3 and all(cv.cin == c for cv in case.convs)
    assert set(case.calls) == {"fp32", "bf16"} and all(n.split(":")[0] in L.TRACKED for d in case.calls.values() for n in d)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", [n for n, c in L.CASES.items() if len(c.convs) == 1])
def test_case_predicates(name, mode):
    """A case cannot slide onto another path unnoticed when a predicate changes: the table states which hold."""
    case = L.CASES[name]
    assert L.predicates(case, L.DTYPES[mode]) == case.preds[mode], (name, mode)


def test_engine_decisions_the_table_relies_on():
    """The decisions of engine._conv_backward that are not `ops` predicates, evaluated as the engine spells them."""
    from cta_gan_amd import engine as E
    from cta_gan_amd import ops
    for case in L.CASES.values():
        for cv in case.convs:
            spec = E.ConvSpec(**dataclasses.asdict(cv))
            assert dataclasses.asdict(spec) == dataclasses.asdict(cv)
            assert E.conv_out_hw(spec, case.shape[2], case.shape[3]) == L.out_hw(cv, case.shape[2], case.shape[3])
        cv = case.convs[0]
        ho, wo = L.out_hw(cv, case.shape[2], case.shape[3])
        if case.family == "tail" and cv.cout > 1:
            # the [:16] slice of the bf16 weight gradient: only from 8 x 16 outputs on
            assert case.wgrad_g == ((16, 32) if (ho >= 8 and wo >= 16) else (32, 32)), case.name
            n = case.shape[0] * cv.cout * ho * wo
            assert ("act_bwd_f32" in case.calls["bf16"]) == bool(n % 4), case.name
        if case.family == "head":
            assert cv.cin * cv.k * cv.k == 98 and E._round_up(98, 32) == 128      # Kpad of the packed im2col matrix
        if case.family == "fanout":
            h, w = case.shape[2:]
            framed = h % 16 == 0 and w % 16 == 0 and h >= 32 and w >= 32
            assert framed == ("conv_igemm:frame" in case.calls["bf16"]), case.name
            assert not framed or ops.conv_fusable(64, h, w)
        if case.family == "stride2":
            h, w = case.shape[2:]
            merged = h % 2 == 0 and w % 2 == 0 and h // 2 >= 16 and w // 2 >= 16      # ops.conv_igemm_classes: bf16, >= 16 x 16
            assert merged == ("conv_igemm_classes" in case.calls["bf16"]), case.name
            assert "conv_igemm_classes" not in case.calls["fp32"]
    # every path the GPU module exists for has a case
    assert all(L.PATH_CASES[n] for n in range(1, 9)), L.PATH_CASES


def test_transposed_classes_and_odd_grids_cover_the_input():
    """engine._bwd_data_launch on odd sizes: the class grids (hi - py + 1) // 2 tile the input exactly once."""
    for hi in (9, 13, 16):
        rows = sorted(2 * j + py for py in (0, 1) for j in range((hi - py + 1) // 2))
        assert rows == list(range(hi))


@pytest.mark.parametrize("name", ["tail_64to3_tanh_8x16", "head_2to64_17x33_bias_dx", "dlast_512to1_sigmoid_5x7",
                                  "preq_plain_lrelu_all", "fanout_reflect_plain_1x1_9x11", "s2_64to128_9x13", "convT_128to64_5x7"])
def test_reference_reproduces_float32_autograd(name):
    """One random (off-grid) case per family: the float64 reference against the same layer in torch float32."""
    case = L.CASES[name]
    rng = np.random.default_rng(5)
    x, ws, bs, gs = L.operands(case)

    def rnd(t, scale=1.0):
        return torch.from_numpy(rng.standard_normal(tuple(t.shape)) * scale).double()
    ops_ = (rnd(x), [rnd(w, (2.0 / (w[0].numel() if not cv.transposed else w[:, 0].numel())) ** 0.5) for w, cv in zip(ws, case.convs)],
            [rnd(b, 0.3) for b in bs], [rnd(g) for g in gs])
    ops32 = tuple(t.float().double() if isinstance(t, torch.Tensor) else [u.float().double() for u in t] for t in ops_)
    want = L.reference(case, ops32)
    got = L.reference(case, ops32, dtype=torch.float32)

    def rel(a, b):
        return float((a.double() - b).abs().max() / b.abs().max())
    for i in range(len(case.convs)):
        assert rel(got.y[i], want.y[i]) < FP32_TOL and rel(got.dw[i], want.dw[i]) < FP32_TOL
        if want.db[i] is not None:
            assert rel(got.db[i], want.db[i]) < FP32_TOL
    assert rel(got.dx, want.dx) < FP32_TOL


def test_reference_padded_grid_gradient_folds_to_the_input_gradient():
    """dxp, the gradient on the reflection-padded grid (what condition 2 bounds), folds to dx by the transpose of F.pad."""
    case = L.CASES["fanout_reflect_reflect_9x11"]
    ref = L.reference(case)
    for dxp, dx in zip(ref.dxp, ref.dx_each):
        xp = torch.zeros_like(dx).requires_grad_(True)
        torch.nn.functional.pad(xp, (1,) * 4, mode="reflect").backward(dxp)
        assert torch.equal(xp.grad, dx)
