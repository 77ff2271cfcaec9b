"""GPU: the channel configurations the networks accept beyond the reference's 1 -> 1, against the CPU oracle (oracle/).

GeneratorNet takes input_nc in {1, 2} and output_nc in 1..4, the PatchGAN stacks input_nc in {1, 2}, and the trainers hand
config["input_nc"] / config["output_nc"] straight through -- yet every other network-level test builds Generator(1, 1).  A
generator with two input planes runs its 7x7 head through im2col_pack + a 1x1 gather instead of the image-plane kernel, and one
with 2..4 output channels runs its tail, and the tail's three gradients, through the MFMA kernels zero-padded to 32 channels
instead of the one-channel tail kernels (tests/test_layer_glue_exact_gpu.py holds those layers bit for bit; here they sit inside
the whole network).

Bounds are the project's (tests/test_parity_gpu.py): fp32 mode output rel-L2 <= 1e-3, gradients -- the input gradient and EVERY
parameter gradient, per element, not as norms -- rel-L2 <= 5e-3; bf16 mode output <= 3e-2 and finite gradients.  A bias in front
of an affine-free InstanceNorm is mathematically dead: the HIP path returns no gradient for it (None), and only for such biases.
The CycleGAN step uses the bounds of test_hip_step_matches_reference_golden.  Generators here have two residual blocks, not nine:
the blocks are 256 -> 256 whatever the image channels, and the CPU oracle then finishes in about a second.
"""
import functools
import itertools
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL, BF16_OUT_TOL = 1e-3, 5e-3, 3e-2


@pytest.fixture(scope="module")
def ns():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib, nets
    _lib.load()
    nets.set_default_compute_dtype(torch.float32)
    from hip_ns import hip_namespace
    return hip_namespace()


def _ons():
    from oracle import golden_cases
    return golden_cases.oracle_namespace()


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).norm() / want.norm().clamp_min(1e-30))


def _run(net, x, weight, dev):
    """out, d/dx and {key: d/dparam} of sum(net(x) * weight)."""
    xg = x.detach().clone().to(dev).requires_grad_(True)      # (a fresh leaf: `x` is shared between tests)
    out = net(xg)
    (out * weight.to(dev)).sum().backward()
    return out.detach(), xg.grad, {k: p.grad for k, p in net.named_parameters()}


def _compare(name, got, want, must_have):
    """fp32 bounds on (out, dx, parameter gradients); the HIP path may leave out dead biases only."""
    errs = {"out": rel_l2(got[0], want[0]), "dx": rel_l2(got[1], want[1])}
    for k, w in want[2].items():
        g = got[2][k]
        if g is None:
            assert k.endswith(".bias") and k not in must_have, (name, k, "no gradient")
            continue
        errs[k] = rel_l2(g, w)
    print(name, {k: "%.1e" % v for k, v in errs.items() if k in ("out", "dx") or k in must_have}, "worst parameter gradient %.1e"
          % max(v for k, v in errs.items() if k not in ("out", "dx")))
    assert all(k in errs for k in must_have)
    assert errs["out"] <= OUT_TOL, (name, errs["out"])
    bad = {k: v for k, v in errs.items() if k != "out" and not v <= GRAD_TOL}
    assert not bad, (name, bad)


# ---------------------------------------------------------------------------- generators
GEN_CONFIGS = [(2, 1), (1, 2), (1, 3), (2, 4)]


@functools.lru_cache(maxsize=None)
def _gen_reference(ci, co):
    """Oracle result of Generator(ci, co, 2 blocks) on a 32 x 48 batch of 2: computed once, shared by the fp32 and bf16 tests."""
    from cta_gan_amd import synth
    x = synth.synth_images("mc_gen_x", 2, 48, channels=ci)[:, :, :32].contiguous()      # (synth_images is square-only: crop)
    wgt = synth.synth_images("mc_gen_w", 2, 48, channels=co)[:, :, :32].contiguous()
    ref = synth.fill_module(_ons().Generator(ci, co, n_residual_blocks=2), seed=31)
    return x, wgt, _run(ref, x, wgt, "cpu")


@pytest.mark.parametrize("ci,co", GEN_CONFIGS, ids=["%dto%d" % c for c in GEN_CONFIGS])
def test_generator_fp32(ci, co, ns):
    from cta_gan_amd import synth
    x, wgt, want = _gen_reference(ci, co)
    hip = synth.fill_module(ns.Generator(ci, co, n_residual_blocks=2), seed=31).to("cuda")
    got = _run(hip, x, wgt, "cuda")
    _compare("generator %d->%d" % (ci, co), got, want,
             ("model_head.1.weight", "model_tail.7.weight", "model_tail.7.bias"))


@pytest.mark.parametrize("ci,co", GEN_CONFIGS, ids=["%dto%d" % c for c in GEN_CONFIGS])
def test_generator_bf16(ci, co, ns):
    from cta_gan_amd import synth
    x, wgt, want = _gen_reference(ci, co)
    hip = synth.fill_module(ns.Generator(ci, co, n_residual_blocks=2), seed=31).to("cuda")
    hip.compute_dtype = torch.bfloat16
    out, dx, grads = _run(hip, x, wgt, "cuda")
    err = rel_l2(out, want[0])
    print("generator %d->%d bf16: out rel-L2 %.2e, dx rel-L2 %.2e" % (ci, co, err, rel_l2(dx, want[1])))
    assert err <= BF16_OUT_TOL
    assert bool(torch.isfinite(dx).all()) and tuple(dx.shape) == tuple(x.shape)
    for k in ("model_head.1.weight", "model_tail.7.weight", "model_tail.7.bias"):
        assert grads[k] is not None and bool(torch.isfinite(grads[k]).all()), k
    assert all(g is None or bool(torch.isfinite(g).all()) for g in grads.values())


# ---------------------------------------------------------------------------- discriminators
def _d_loss_run(net, x, dev):
    xg = x.detach().clone().to(dev).requires_grad_(True)
    out = net(xg)
    ((out - 1.0) ** 2).mean().backward()
    return out.detach(), xg.grad, {k: p.grad for k, p in net.named_parameters()}


@pytest.mark.parametrize("kind", ["discriminator", "nlayer_instance"])
def test_two_channel_discriminators_fp32(kind, ns):
    from cta_gan_amd import synth
    inorm = functools.partial(torch.nn.InstanceNorm2d, affine=False)

    def make(space):
        if kind == "discriminator":
            return space.Discriminator(2)
        return space.NLayerDiscriminator(2, norm_layer=inorm)
    x = synth.synth_images("mc_disc_x", 2, 64, channels=2)
    ref = synth.fill_module(make(_ons()), seed=13)
    hip = synth.fill_module(make(ns), seed=13).to("cuda")
    want = _d_loss_run(ref, x, "cpu")
    got = _d_loss_run(hip, x, "cuda")
    keys = list(want[2])
    first, last = keys[0].rsplit(".", 1)[0], keys[-1].rsplit(".", 1)[0]
    _compare(kind + "(2)", got, want, (first + ".weight", first + ".bias", last + ".weight", last + ".bias"))


# ---------------------------------------------------------------------------- one CycleGAN step on two-channel images
def _cyc(space, dev):
    from cta_gan_amd import synth
    from oracle import ref_steps
    random.seed(42)
    nets_ = dict(G_A2B=synth.fill_module(space.Generator(2, 2, n_residual_blocks=2), seed=0).to(dev),
                 G_B2A=synth.fill_module(space.Generator(2, 2, n_residual_blocks=2), seed=5).to(dev),
                 D_A=synth.fill_module(space.Discriminator(2), seed=6).to(dev),
                 D_B=synth.fill_module(space.Discriminator(2), seed=1).to(dev))
    opts = dict(G=ref_steps.make_adam(itertools.chain(nets_["G_A2B"].parameters(), nets_["G_B2A"].parameters())),
                D_A=ref_steps.make_adam(nets_["D_A"].parameters()), D_B=ref_steps.make_adam(nets_["D_B"].parameters()))
    bufs = dict(A=ref_steps.ReplayBuffer(), B=ref_steps.ReplayBuffer())
    batch = {k: torch.cat([synth.synth_smooth_images("mc_cyc_%s%d" % (k, c), 2, 64) for c in (0, 1)], dim=1).to(dev)
             for k in ("A", "B")}
    out = ref_steps.cyc_step(nets_, opts, bufs, batch)
    with torch.no_grad():
        out["fake_B_after"] = nets_["G_A2B"](batch["A"])
    return {k: (v if isinstance(v, float) else v.detach().float().cpu()) for k, v in out.items()}


def test_cyclegan_step_two_channels(ns):
    """oracle.ref_steps.cyc_step once on the oracle networks and once on the HIP networks (torch's Adam on both): the cycle
    terms back-propagate through a generator's two-plane input, the GAN terms through a two-plane discriminator input."""
    want = _cyc(_ons(), "cpu")
    got = _cyc(ns, "cuda")
    rep = {}
    for k, w in want.items():
        g = got[k]
        if isinstance(w, float):
            rep[k] = abs(g - w) / max(abs(w), 1e-6)
            assert abs(g - w) <= 2e-3 * max(abs(w), 1e-6) + 1e-6, (k, g, w)
        else:
            rep[k] = rel_l2(g, w)
            assert rep[k] <= (2e-2 if "after" in k else 1e-3), (k, rep[k])
    print("cyc step 2ch", {k: "%.1e" % v for k, v in rep.items()})


# ---------------------------------------------------------------------------- what the constructors refuse
def test_constructors_refuse_unsupported_channel_counts(ns):
    from cta_gan_amd import nets
    for make in (lambda: ns.Generator(3, 1), lambda: ns.Generator(1, 5), lambda: ns.Generator(1, 0), lambda: ns.Discriminator(3),
                 lambda: ns.NLayerDiscriminator(3), lambda: nets.RegNet(2, 1)):
        with pytest.raises(NotImplementedError):
            make()
