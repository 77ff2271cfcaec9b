"""Micro-benchmark of the InstanceNorm elementwise kernels at the three large maps they run at in the benchmarked step
(bf16, B = 16): the residual-block shape 128 x 128 x 256, and 256 x 256 x 64 / 512 x 512 x 32 of the outer layers."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cta_gan_amd import ops
dev = torch.device("cuda:0")

def t(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3

for B, S, C in ((16, 128, 256), (16, 256, 64), (16, 512, 32)):
    x = torch.randn(B, S, S, C, device=dev).bfloat16()
    r = torch.randn(B, S, S, C, device=dev).bfloat16()
    g = torch.randn(B, S, S, C, device=dev).bfloat16()
    gp = torch.randn(B, S + 2, S + 2, C, device=dev).bfloat16()
    o = torch.empty_like(x)
    xi = x.clone()          # normalised in place over and over: the values do not matter to the timing
    mean, rstd = ops.in_stats(x)
    mb = x.numel() * 2 / 1e6
    print("B=%d %dx%dx%d bf16 (%.0f MB per tensor)" % (B, S, S, C, mb))
    for name, fn, passes in (("in_apply relu", lambda: ops.in_apply(x, mean, rstd, 1, None, o), 2),
                             ("in_apply relu in place", lambda: ops.in_apply(xi, mean, rstd, 1, None, xi), 2),
                             ("in_apply +res", lambda: ops.in_apply(x, mean, rstd, 0, r, o), 3),
                             ("in_stats", lambda: ops.in_stats(x), 1),
                             ("in_bwd pad0", lambda: ops.in_bwd(x, g, 0, mean, rstd, 1, o), 5),
                             ("in_bwd pad1", lambda: ops.in_bwd(x, gp, 1, mean, rstd, 1, o), 5),
                             ("grad_combine", lambda: ops.grad_combine(g, gp, 1, None, 0, o), 3)):
        us = t(fn)
        print("  %-22s %7.1f us  %5.2f TB/s (%d tensor passes)" % (name, us, passes * mb / us, passes))
    del x, r, g, gp, o, xi
