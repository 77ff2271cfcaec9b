"""numpy restatement (test infrastructure only) of the lumen sections, csrc/lumen.hip (ctg_lumen_sections), written from the
definitions in include/ctagan_hip.h on top of reformat_np.sample / counted:

  sections(vol, lines, T, lo, hi, sampling, edge, base, recentre)   -> (radii int32 [R, K], cross int64 [R], sections int32 [R, 8],
                                                                     centres int32 [R, 3]) for a table [R, K, 9]: section r has the
                                                                     centre (x0, y0, z0) of row (r, 0), ray j the step (xk, yk, zk)
                                                                     of row (r, j)
  area(cross, K), equivalent_diameter(cross, K)                      the polygon's area sin(2 pi / K) / 2 * cross and 2 sqrt(area / pi),
                                                                     in squared / plain units of rho

A plain loop over the walks and over k with masks: no lanes, no shuffles, no samples in flight.  int64 inside; the int32 and int64
ranges the kernel relies on are asserted."""
import math

import numpy as np

from reformat_np import counted, sample

EDGES = ("band", "half")
RAYS = (8, 16, 32, 64)


def sections(vol, lines, T, lo, hi=32767, sampling="trilinear", edge="band", base=None, recentre=0):
    vol = np.asarray(vol)
    c = np.asarray(lines).astype(np.int64)
    assert vol.dtype == np.int16 and vol.ndim == 3 and c.ndim == 3 and c.shape[2] == 9, (vol.dtype, vol.shape, c.shape)
    R, K = c.shape[:2]
    assert K in RAYS and 2 <= T <= 256 and 0 <= recentre <= 4 and edge in EDGES and -32768 <= lo <= hi <= 32767
    logk = K.bit_length() - 1
    if edge == "half":
        assert base is not None and -32768 <= base <= lo
    C = c[:, 0, 0::3].copy()      # [R, 3]: x, y, z
    D = c[:, :, 2::3]             # [R, K, 3]
    # the range ops.lumen_sections promises the kernel: no fixed-point sum leaves int32
    assert (np.abs(C) + (1 + 2 * recentre) * (T - 1) * np.abs(D).max(axis=1)).max() < 2 ** 31
    rho = np.zeros((R, K), dtype=np.int64)
    opened = np.zeros((R, K), dtype=bool)
    outside = np.zeros(R, dtype=np.int64)
    lor = np.full(R, lo, dtype=np.int64)
    act = np.ones(R, dtype=bool)
    for it in range(recentre + 1):
        assert np.abs(C).max() < 2 ** 31
        cin = counted(vol.shape, C[:, 0], C[:, 1], C[:, 2])
        s0 = sample(vol, C[:, 0], C[:, 1], C[:, 2], sampling)
        out = ~cin | (s0 < lo) | (s0 > hi)
        low = np.full(R, lo, dtype=np.int64)
        if edge == "half":
            low = np.where(out, lo, np.maximum(lo, (s0 + base) >> 1))
        assert (out | (low <= s0)).all()
        walk = act & ~out
        r_new = np.zeros((R, K), dtype=np.int64)
        o_new = np.zeros((R, K), dtype=bool)
        stopped = np.repeat(~walk[:, None], K, axis=1)
        prev = np.repeat(s0[:, None], K, axis=1)
        lowk = low[:, None]
        for k in range(1, T):
            P = C[:, None, :] + D * k
            assert np.abs(P).max() < 2 ** 31
            ok = counted(vol.shape, P[..., 0], P[..., 1], P[..., 2])
            v = sample(vol, P[..., 0], P[..., 1], P[..., 2], sampling)
            going = ~stopped
            leaves = going & ~ok
            below = going & ok & (v < lowk)
            above = going & ok & ~(v < lowk) & (v > hi)
            assert (~below | ((prev - lowk >= 0) & (prev - v > prev - lowk))).all()
            assert (~above | ((hi - prev >= 0) & (v - prev > hi - prev))).all()
            at = (k - 1) * 256
            r_new = np.where(leaves, at, r_new)
            o_new |= leaves
            r_new = np.where(below, at + ((prev - lowk) * 256) // np.where(below, prev - v, 1), r_new)
            r_new = np.where(above, at + ((hi - prev) * 256) // np.where(above, v - prev, 1), r_new)
            stopped = stopped | leaves | below | above
            prev = np.where(going & ~stopped, v, prev)
        never = ~stopped
        r_new = np.where(never, (T - 1) * 256, r_new)
        o_new |= never
        assert r_new.min() >= 0 and r_new.max() <= 65280
        # the last walk's numbers are the ones kept
        rho = np.where(act[:, None], r_new, rho)
        opened = np.where(act[:, None], o_new, opened)
        outside = np.where(act, out.astype(np.int64), outside)
        lor = np.where(act, low, lor)
        if it == recentre:
            break
        act = act & (outside == 0) & (opened.sum(axis=1) == 0)
        S = (rho[:, :, None] * D).sum(axis=1)      # [R, 3], below 2^53
        assert np.abs(S).max() < 2 ** 62
        C = np.where(act[:, None], C + ((S + (K << 6)) >> (7 + logk)), C)
        if not act.any():
            break
    cross = (rho * np.roll(rho, -1, axis=1)).sum(axis=1)
    assert cross.max() < 2 ** 62
    chord = rho[:, :K // 2] + rho[:, K // 2:]
    sec = np.stack([rho.sum(axis=1), chord.min(axis=1), chord.max(axis=1), chord.argmin(axis=1), chord.argmax(axis=1),
                    opened.sum(axis=1), outside, lor], axis=1)      # (argmin / argmax: the first on a tie)
    assert np.abs(sec).max() < 2 ** 31 and np.abs(C).max() < 2 ** 31
    return rho.astype(np.int32), cross.astype(np.int64), sec.astype(np.int32), C.astype(np.int32)


def area(cross, rays):
    return 0.5 * math.sin(2.0 * math.pi / rays) * np.asarray(cross, dtype=np.float64)


def equivalent_diameter(cross, rays):
    return 2.0 * np.sqrt(area(cross, rays) / math.pi)
