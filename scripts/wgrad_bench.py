"""Micro-benchmark of the halo-resident weight-gradient launches of the bf16 Hd step, alone on the card (us per launch, reduce
excluded): the residual blocks' 256 x 256 3x3 at B = 16, 128^2; Reg's 32 x 32 3x3 at 512^2; the discriminator's 256 -> 512 4x4
at 63^2; the merged stride-2 launch of the generator's 64 -> 128 down-sampling conv (G on 256^2, X on 512^2).
    python scripts/wgrad_bench.py [REPS]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cta_gan_amd import ops
from cta_gan_amd.engine import PAD_REFLECT, PAD_ZERO, pack_tap
dev = torch.device("cuda:0")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def taps(k, pad):
    return [pack_tap(ky - pad, kx - pad, ky * k + kx) for ky in range(k) for kx in range(k)]


CASES = [  # name, Mc, Nc, taps, B, Hs, Hi, input stride, padding
    ("256x256 3x3 reflect B16 128^2", 256, 256, taps(3, 1), 16, 128, 128, 1, PAD_REFLECT),
    ("32x32 3x3 zero B16 512^2", 32, 32, taps(3, 1), 16, 512, 512, 1, PAD_ZERO),
    ("512x256 4x4 zero B16 63^2", 512, 256, taps(4, 1), 16, 63, 64, 1, PAD_ZERO),
    ("128x64 3x3 stride 2 B16 256^2", 128, 64, taps(3, 1), 16, 256, 512, 2, PAD_ZERO),
]
for name, mc, nc, tp, B, hs, hi, is_, pad in CASES:
    g = torch.randn(B, hs, hs, mc, device=dev).bfloat16()
    x = torch.randn(B, hi, hi, nc, device=dev).bfloat16()
    dst = torch.empty(mc * nc * len(tp), dtype=torch.float32, device=dev)
    f = lambda: ops.conv_wgrad(g, x, tp, is_, pad, dst, mc, nc, nc * len(tp), len(tp), 1, defer=[])
    for _ in range(3): f()
    torch.cuda.synchronize()
    for rnd in range(2):      # the second pass is the one to read
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): f()
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / n * 1e3
    print("wgrad %-32s %8.1f us  %6.0f TF" % (name, us, 2.0 * B * hs * hs * mc * nc * len(tp) / us / 1e6))
    del g, x, dst
