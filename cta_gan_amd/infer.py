"""Series inference: a raw HU volume in, the synthesized volume out in the scanner's pixel format.

The export half of the reference's test() loop (trainer/HdTrainer.py:539-552) without its DICOM container: int16 HU crosses
PCIe at 2 B/pixel, `ops.series_inputs` makes the generator's plane on the device, the generator runs without autograd, and
`ops.export_slices` turns its output into int16 pixels (+ the 8-bit window level) that cross back at 3 B/pixel.  Chunks of
`batch` slices go through two page-locked slots per direction; the H2D and the D2H copies run on streams of their own behind
events, so both hide behind the forward of the neighbouring chunks and the host only ever waits to get a slot back.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from . import ops

SLOTS = 2


def plan_chunks(n, batch):
    """[(start, stop, slot), ...]: `n` slices in chunks of at most `batch` (the last may be shorter), chunk i in slot i % 2."""
    n, batch = int(n), int(batch)
    if n < 0 or batch < 1:
        raise ValueError("plan_chunks: n >= 0 and batch >= 1 expected, got n=%d batch=%d" % (n, batch))
    return [(s, min(s + batch, n), i % SLOTS) for i, s in enumerate(range(0, n, batch))]


def _pair(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


class SeriesTranslator:
    """`SeriesTranslator(generator)(volume)`: int16 HU volume [N, H, W] (numpy array or CPU tensor, SimpleITK convention) ->
    {"pix": int16 [N, H, W], "level": uint8 [N, H, W] or None}, of the input's kind.

    size: the side(s) the generator runs at (None: the volume's own); a volume of another size is resized (nearest) on the way
    in and comes back at its own size.  wc / ww: the window of the 8-bit level; hu: pixels minus 1024 (SimpleITK) instead of
    the reference's stored values; level=False skips the 8-bit plane.  Runs in whatever compute mode is set, on the current
    stream, outside any captured graph."""

    def __init__(self, generator, batch=16, size=None, wc=50.0, ww=400.0, hu=False, level=True, device=None):
        if int(batch) < 1:
            raise ValueError("SeriesTranslator: batch >= 1 expected")
        self.generator = generator
        self.batch = int(batch)
        self.size = None if size is None else _pair(size)
        self.hu, self.level = bool(hu), bool(level)
        if device is None:
            p = next(generator.parameters(), None)
            device = p.device if p is not None and p.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SeriesTranslator: a GPU device is required (no CPU fallback)")
        self.wc = torch.full((self.batch,), float(wc), dtype=torch.float32, device=self.device)
        self.ww = torch.full((self.batch,), float(ww), dtype=torch.float32, device=self.device)
        self.h2d = torch.cuda.Stream(device=self.device)
        self.d2h = torch.cuda.Stream(device=self.device)
        self._hw = None
        self._in = self._pix = self._lvl = None
        # host seconds of the last call (scripts/export_bench.py): waiting to get a slot back, copying into the input slots,
        # copying out of the output slots, the whole call
        self.stats = {"wait": 0.0, "stage_in": 0.0, "stage_out": 0.0, "total": 0.0}

    def _stage(self, h, w):
        """The page-locked slots for planes of h x w (kept between calls on volumes of one size)."""
        if self._hw != (h, w):
            shape = (self.batch, h, w)
            self._in = [torch.empty(shape, dtype=torch.int16, pin_memory=True) for _ in range(SLOTS)]
            self._pix = [torch.empty(shape, dtype=torch.int16, pin_memory=True) for _ in range(SLOTS)]
            self._lvl = [torch.empty(shape, dtype=torch.uint8, pin_memory=True) for _ in range(SLOTS)] if self.level else None
            self._hw = (h, w)

    def __call__(self, volume):
        is_np = isinstance(volume, np.ndarray)
        vol = torch.from_numpy(np.ascontiguousarray(volume)) if is_np else volume
        if not torch.is_tensor(vol) or vol.is_cuda or vol.dtype != torch.int16 or vol.dim() != 3:
            raise RuntimeError("SeriesTranslator: an int16 volume [N, H, W] on the host (numpy array or CPU tensor) expected")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("SeriesTranslator: runs outside a captured graph (it waits on events from the host)")
        clock = time.perf_counter
        stats = self.stats = {"wait": 0.0, "stage_in": 0.0, "stage_out": 0.0, "total": 0.0}
        t_call = clock()
        vol = vol.contiguous()
        n, h, w = vol.shape
        gsize = self.size or (h, w)
        out_pix = torch.empty((n, h, w), dtype=torch.int16)
        out_lvl = torch.empty((n, h, w), dtype=torch.uint8) if self.level else None
        if n == 0:
            return self._result(out_pix, out_lvl, is_np)
        self._stage(h, w)
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream()
            in_free = [None] * SLOTS       # event: the slot's H2D copy has drained, the host may rewrite it
            pending = [None] * SLOTS       # (event, start, stop): the slot's D2H copy, not yet moved into the result

            def drain(slot):
                if pending[slot] is None:
                    return
                ev, s, e = pending[slot]
                t0 = clock()
                ev.synchronize()
                t1 = clock()
                out_pix[s:e].copy_(self._pix[slot][:e - s])
                if out_lvl is not None:
                    out_lvl[s:e].copy_(self._lvl[slot][:e - s])
                pending[slot] = None
                stats["wait"] += t1 - t0
                stats["stage_out"] += clock() - t1

            for s, e, slot in plan_chunks(n, self.batch):
                k = e - s
                t0 = clock()
                if in_free[slot] is not None:
                    in_free[slot].synchronize()      # two chunks ago: long finished in steady state
                t1 = clock()
                self._in[slot][:k].copy_(vol[s:e])
                stats["wait"] += t1 - t0
                stats["stage_in"] += clock() - t1
                arrived = torch.cuda.Event()
                with torch.cuda.stream(self.h2d):
                    dev_hu = self._in[slot][:k].to(self.device, non_blocking=True)
                    arrived.record()
                in_free[slot] = arrived
                cur.wait_event(arrived)
                dev_hu.record_stream(cur)            # allocated on the copy stream, consumed on this one
                with torch.no_grad():
                    x = ops.series_inputs(dev_hu, gsize).unsqueeze(1)
                    fake = self.generator(x)
                    pix, lvl = ops.export_slices(fake, self.wc[:k], self.ww[:k], size=(h, w), hu=self.hu, want_level=self.level)
                computed = torch.cuda.Event()
                computed.record(cur)
                drain(slot)                          # the chunk that used this slot last: its D2H started two chunks ago
                done = torch.cuda.Event()
                with torch.cuda.stream(self.d2h):
                    self.d2h.wait_event(computed)
                    self._pix[slot][:k].copy_(pix, non_blocking=True)
                    pix.record_stream(self.d2h)
                    if lvl is not None:
                        self._lvl[slot][:k].copy_(lvl, non_blocking=True)
                        lvl.record_stream(self.d2h)
                    done.record()
                pending[slot] = (done, s, e)
            for slot in sorted(range(SLOTS), key=lambda q: pending[q][1] if pending[q] else -1):
                drain(slot)
        # the forwards above ran fused conv + InstanceNorm launches: none may have given up (raises)
        ops.nie_check("series inference")
        stats["total"] = clock() - t_call
        return self._result(out_pix, out_lvl, is_np)

    @staticmethod
    def _result(pix, lvl, is_np):
        if is_np:
            return {"pix": pix.numpy(), "level": None if lvl is None else lvl.numpy()}
        return {"pix": pix, "level": lvl}
