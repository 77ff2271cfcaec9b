"""Test infrastructure (never imported by the product path): a torch-CPU restatement of `lpips.LPIPS(net='alex')` (version 0.1)
as the reference's test() loops call it -- `loss_fn_alex.forward(torch.tensor(x), torch.tensor(y))` on two 2-D arrays in [-1, 1]
(trainer/HdTrainer.py:26-28, 504-513) -- written from the published algorithm with stock torch ops, parameterised by dtype so
that it runs in float64 (the yardstick of the GPU tests) and in float32.

  scaling layer   (x - shift) / scale, shift / scale of shape [1, 3, 1, 1]: a 2-D input broadcasts to [1, 3, H, W]
  features        conv 3->64 k11 s4 p2 | pool 3/2, conv 64->192 k5 p2 | pool 3/2, conv 192->384 k3 p1 | conv 384->256 k3 p1 |
                  conv 256->256 k3 p1; bias + ReLU after each; zero padding
  per layer       n(f) = f / (sqrt(sum_c f^2) + 1e-10); d = sum_c lin[c] (n(fx) - n(fy))^2; l = mean over pixels
  result          l_1 + ... + l_5

PARITY UNPINNED: neither `lpips` nor `torchvision` can be installed here, so no fixture of the real package exists.  Weights are
passed in the layout of `lpips.LPIPS(net='alex').state_dict()` (cta_gan_amd.lpips.KEYS, cta_gan_amd.synth.lpips_state_dict)."""
import torch
import torch.nn.functional as F

from cta_gan_amd.lpips import CONVS, KEYS, SCALE, SHIFT


def _weights(sd, dtype):
    convs = [(sd[KEYS["full_conv"][k] + ".weight"].to(dtype), sd[KEYS["full_conv"][k] + ".bias"].to(dtype)) for k in range(5)]
    lins = [sd[KEYS["lin"][k]].to(dtype) for k in range(5)]
    shift = sd.get(KEYS["shift"], torch.tensor(SHIFT).reshape(1, 3, 1, 1)).to(dtype)
    scale = sd.get(KEYS["scale"], torch.tensor(SCALE).reshape(1, 3, 1, 1)).to(dtype)
    return convs, lins, shift, scale


def _tail(f1, convs):
    """f1 (after conv1 + ReLU) -> [f1 .. f5]."""
    feats = [f1]
    f = f1
    for k in range(1, 5):
        if k <= 2:
            f = F.max_pool2d(f, 3, 2)
        f = F.relu(F.conv2d(f, convs[k][0], convs[k][1], stride=CONVS[k][3], padding=CONVS[k][4]))
        feats.append(f)
    return feats


def features(img, sd, dtype=torch.float64):
    """img [B, H, W] -> [f1 .. f5], each [B, C, h, w]: the 3-channel form, as the package computes it."""
    convs, _, shift, scale = _weights(sd, dtype)
    x = (img.to(dtype)[:, None] - shift) / scale                  # [B, 3, H, W]
    f1 = F.relu(F.conv2d(x, convs[0][0], convs[0][1], stride=4, padding=2))
    return _tail(f1, convs)


def features_folded(img, sd, dtype=torch.float64):
    """The same through the folded two-plane stem (cta_gan_amd.lpips.fold_stem): planes (image, ones), both zero padded."""
    from cta_gan_amd.lpips import fold_stem
    convs, _, shift, scale = _weights(sd, dtype)
    w = fold_stem(convs[0][0], shift.reshape(3), scale.reshape(3)).to(dtype).reshape(64, 2, 11, 11)
    x = torch.stack([img.to(dtype), torch.ones_like(img, dtype=dtype)], dim=1)
    f1 = F.relu(F.conv2d(x, w, convs[0][1], stride=4, padding=2))
    return _tail(f1, convs)


def layer_distance(fx, fy, lin):
    """fx, fy [B, C, h, w], lin [1, C, 1, 1] -> [B]."""
    nx = fx / (torch.sqrt((fx ** 2).sum(1, keepdim=True)) + 1e-10)
    ny = fy / (torch.sqrt((fy ** 2).sum(1, keepdim=True)) + 1e-10)
    d = F.conv2d((nx - ny) ** 2, lin)
    return d.mean((1, 2, 3))


def lpips(x, y, sd, dtype=torch.float64, folded=False):
    """x, y [B, H, W] in [-1, 1] -> per-layer values [B, 5] (their sum over the last axis is LPIPS)."""
    fn = features_folded if folded else features
    _, lins, _, _ = _weights(sd, dtype)
    fx, fy = fn(x, sd, dtype), fn(y, sd, dtype)
    return torch.stack([layer_distance(fx[k], fy[k], lins[k]) for k in range(5)], dim=1)


def make_pairs(h, w, b=3, seed=0):
    """The input recipe of the GPU tests: x ~ U(-1, 1), y = clamp(x + 0.3 N(0, 1)); the top third of y and the top quarter of x are
    the background (-1) that masked images really have -- zero-norm feature pixels and the border."""
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    x = torch.rand((b, h, w), generator=g) * 2 - 1
    y = (x + 0.3 * torch.randn((b, h, w), generator=g)).clamp(-1, 1)
    y[:, :h // 3] = -1
    x[:, :h // 4] = -1
    return x, y
