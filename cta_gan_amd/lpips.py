"""LPIPS (AlexNet, lpips 0.1) on the device: the fifth metric of the trainers' test() loops.

The reference builds `loss_fn_alex = lpips.LPIPS(net='alex')` (trainer/HdTrainer.py:26-28) and calls
`loss_fn_alex.forward(torch.tensor(x), torch.tensor(y))` on two 2-D arrays in [-1, 1] per pair (:504-513, 531-536).  Neither
`lpips` nor `torchvision` is a dependency here; only the weight FILE is pretrained, the arithmetic is

  1. scaling layer  (x - shift) / scale, the grey plane broadcast to three channels;
  2. AlexNet features: conv 3->64 k11 s4 p2, [pool 3/2] conv 64->192 k5 p2, [pool 3/2] conv 192->384 k3 p1, conv 384->256 k3 p1,
     conv 256->256 k3 p1, each + bias + ReLU, zero padding;
  3. per layer  l_k = mean_pixels sum_c lin_k[c] (n(f_k(x)) - n(f_k(y)))^2,  n(f) = f / (sqrt(sum_c f^2) + 1e-10);
  4. LPIPS = l_1 + ... + l_5.

All of it runs in fp32 on the library's kernels: the stem as a two-plane im2col (the scaling layer and the channel broadcast are
folded into the weights on the host in float64: plane 0 the image, plane 1 a plane of ones that carries the shift and vanishes in
the zero-padded border exactly as the shifted image does) + a 1-tap GEMM, conv2 .. conv5 on `ops.conv_igemm`, the pools on
`ops.maxpool3s2_fwd`, the distances on `ops.lpips_layer` (fp64 sums, bit-reproducible).  No backward pass: a metric, not a loss.

PARITY UNPINNED (like SSIM): the arithmetic above is pinned by tests against a float64 torch-CPU restatement
(tests/lpips_ref.py); no fixture of the real package exists here, and the state-dict key names below are written from the
packages' sources from memory -- KEYS is the one place to fix a wrong name.
"""
from __future__ import annotations

import torch

# (Cout, Cin, k, stride, pad) of AlexNet's five feature convs
CONVS = ((64, 3, 11, 4, 2), (192, 64, 5, 1, 2), (384, 192, 3, 1, 1), (256, 384, 3, 1, 1), (256, 256, 3, 1, 1))
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
MIN_SIZE = 31      # smaller inputs leave the second pool without a window

# ---- the key table: every state-dict name this module reads -------------------------------------------------------------------
_FEATURE_INDEX = (0, 3, 6, 8, 10)      # positions of the convs in torchvision's alexnet().features
KEYS = {
    # lpips.LPIPS(net='alex').state_dict(): conv k lives in net.slice{k+1} under its torchvision index
    "full_conv": tuple("net.slice%d.%d" % (k + 1, i) for k, i in enumerate(_FEATURE_INDEX)),
    # torchvision.models.alexnet().state_dict()
    "alexnet_conv": tuple("features.%d" % i for i in _FEATURE_INDEX),
    # both lpips' full state dict and its weights/v0.1/alex.pth
    "lin": tuple("lin%d.model.1.weight" % k for k in range(5)),
    "lin_duplicate": tuple("lins.%d.model.1.weight" % k for k in range(5)),      # optional; must agree with "lin"
    "shift": "scaling_layer.shift",      # optional; override SHIFT / SCALE
    "scale": "scaling_layer.scale",
}


def _take(sd, key, shape):
    if key not in sd:
        raise ValueError("LPIPS weights: missing key %r (expected shape %s)" % (key, tuple(shape)))
    t = torch.as_tensor(sd[key]).detach().cpu()
    if tuple(t.shape) != tuple(shape):
        raise ValueError("LPIPS weights: key %r has shape %s, expected %s" % (key, tuple(t.shape), tuple(shape)))
    return t.double()


def fold_stem(w1, shift=SHIFT, scale=SCALE):
    """conv1 weights [64, 3, 11, 11] -> float64 [64, 2 * 121] of the two-plane stem: columns 0 .. 120 multiply the image
    (sum_c w[:, c] / scale_c), columns 121 .. 241 a plane of ones (-sum_c w[:, c] shift_c / scale_c).  conv1 of the scaled,
    zero-padded 3-channel input equals this conv of the zero-padded (image, ones) planes: the padding is applied after the scaling
    layer, so the shift term is absent in the border -- where the padded ones plane is zero too."""
    w = torch.as_tensor(w1).double()
    sh = torch.as_tensor(shift, dtype=torch.float64).reshape(1, 3, 1, 1)
    sc = torch.as_tensor(scale, dtype=torch.float64).reshape(1, 3, 1, 1)
    w_img = (w / sc).sum(1)
    w_one = -(w * sh / sc).sum(1)
    return torch.cat([w_img.reshape(w.shape[0], -1), w_one.reshape(w.shape[0], -1)], dim=1)


def _host_params(conv_sd, conv_keys, lin_sd):
    """Validated fp32 host tensors: stem_w [64, 242], w2 .. w5, b1 .. b5, lin0 .. lin4 [C]."""
    out = {}
    # (the package registers the constants as float32 buffers: its own state dict holds them rounded to float32)
    shift, scale = torch.tensor(SHIFT, dtype=torch.float32).double(), torch.tensor(SCALE, dtype=torch.float32).double()
    if KEYS["shift"] in lin_sd or KEYS["scale"] in lin_sd:
        shift = _take(lin_sd, KEYS["shift"], (1, 3, 1, 1)).reshape(3)
        scale = _take(lin_sd, KEYS["scale"], (1, 3, 1, 1)).reshape(3)
    for k, (cout, cin, ks, _, _) in enumerate(CONVS):
        w = _take(conv_sd, conv_keys[k] + ".weight", (cout, cin, ks, ks))
        b = _take(conv_sd, conv_keys[k] + ".bias", (cout,))
        if k == 0:
            out["stem_w"] = fold_stem(w, shift, scale).float().contiguous()
        else:
            out["w%d" % (k + 1)] = w.float().contiguous()
        out["b%d" % (k + 1)] = b.float().contiguous()
        lin = _take(lin_sd, KEYS["lin"][k], (1, cout, 1, 1))
        dup = KEYS["lin_duplicate"][k]
        if dup in lin_sd and not torch.equal(_take(lin_sd, dup, (1, cout, 1, 1)), lin):
            raise ValueError("LPIPS weights: key %r disagrees with %r" % (dup, KEYS["lin"][k]))
        out["lin%d" % k] = lin.reshape(cout).float().contiguous()
    return out


def _round_up(v, m):
    return (v + m - 1) // m * m


def feature_sizes(h, w):
    """[(h, w)] of f1 .. f5 for an H x W input."""
    h1, w1 = (h + 4 - 11) // 4 + 1, (w + 4 - 11) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    return [(h1, w1), (h2, w2), (h3, w3), (h3, w3), (h3, w3)]


class LPIPS:
    """`lpips.LPIPS(net='alex')` for inference on the GPU.  Weights come from `load_state_dict` / `from_files`; none ship."""

    def __init__(self, net="alex", spatial=False, **unsupported):
        if net != "alex":
            raise ValueError("LPIPS: only net='alex' is built (got %r)" % (net,))
        if spatial:
            raise ValueError("LPIPS: spatial=True is not built")
        if unsupported:
            raise ValueError("LPIPS: unsupported arguments %s" % sorted(unsupported))
        self.params = None      # host tensors (`_host_params`)
        self._packs = {}        # device -> packed weights
        self._ws = {}           # (device, B, H, W) -> workspace

    # ---- weights
    def load_state_dict(self, state_dict):
        """The full `lpips.LPIPS(net='alex').state_dict()` (KEYS: full_conv, lin, lin_duplicate, shift, scale)."""
        self.params = _host_params(state_dict, KEYS["full_conv"], state_dict)
        self._packs.clear()
        return self

    def load_two(self, alexnet, lins):
        """A torchvision alexnet state dict (`classifier.*` ignored) + lpips' weights/v0.1/alex.pth."""
        self.params = _host_params(alexnet, KEYS["alexnet_conv"], lins)
        self._packs.clear()
        return self

    @classmethod
    def from_files(cls, path=None, alexnet=None, lins=None, net="alex"):
        """`path`: a file holding the full state dict; or `alexnet=` and `lins=`: the two-file form."""
        self = cls(net=net)
        if path is not None:
            if alexnet is not None or lins is not None:
                raise ValueError("LPIPS.from_files: one file, or alexnet= and lins=")
            return self.load_state_dict(torch.load(path, map_location="cpu"))
        if alexnet is None or lins is None:
            raise ValueError("LPIPS.from_files: the two-file form needs both alexnet= and lins=")
        return self.load_two(torch.load(alexnet, map_location="cpu"), torch.load(lins, map_location="cpu"))

    @classmethod
    def from_config(cls, spec):
        """config['lpips_weights']: one path, or {'alexnet': path, 'lins': path}."""
        if isinstance(spec, dict):
            extra = set(spec) - {"alexnet", "lins"}
            if extra:
                raise ValueError("lpips_weights: unknown entries %s" % sorted(extra))
            return cls.from_files(alexnet=spec.get("alexnet"), lins=spec.get("lins"))
        return cls.from_files(spec)

    # ---- device state
    def _device_packs(self, dev):
        hit = self._packs.get(dev)
        if hit is not None:
            return hit
        from . import ops
        p = self.params
        packs = {"w": [], "npad": [], "b": [], "lin": []}
        # the stem: one slice, K = 2 * 121 zero-padded to 256
        packs["w"].append(ops.weight_pack(p["stem_w"].to(dev), torch.float32, 1, 64, 242, 64, 256, 242, 1, 0))
        packs["npad"].append(64)
        for k in range(1, 5):
            cout, cin, ks, _, _ = CONVS[k]
            kk = ks * ks
            npad = _round_up(cout, 128)
            packs["w"].append(ops.weight_pack(p["w%d" % (k + 1)].to(dev), torch.float32, kk, cout, cin, npad, cin, cin * kk, kk, 1))
            packs["npad"].append(npad)
        for k in range(5):
            packs["b"].append(p["b%d" % (k + 1)].to(dev))
            packs["lin"].append(p["lin%d" % k].to(dev))
        self._packs[dev] = packs
        return packs

    def _workspace(self, dev, b, h, w):
        key = (dev, b, h, w)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        from . import ops
        n = 2 * b
        sizes = feature_sizes(h, w)
        e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        ws = {
            "img": e(n, h, w),
            "ones": torch.ones((n, h, w), dtype=torch.float32, device=dev),
            "col": e(n, sizes[0][0], sizes[0][1], 256),
            "f": [e(n, sh, sw, CONVS[k][0]) for k, (sh, sw) in enumerate(sizes)],
            "pool": [e(n, sizes[1][0], sizes[1][1], 64), e(n, sizes[2][0], sizes[2][1], 192)],
            "part": torch.empty(b * ops.LPIPS_PART, dtype=torch.float64, device=dev),
        }
        self._ws[key] = ws
        return ws

    # ---- the metric
    @torch.no_grad()
    def forward(self, x, y, ret_per_layer=False, normalize=False):
        """x, y: [B, H, W] or [B, 1, H, W] GPU tensors in [-1, 1] -> float64 [B] on the GPU (no sync), or [B, 5] = l_1 .. l_5 with
        ret_per_layer.  The 2B planes run as one batch."""
        from . import ops
        if normalize:
            raise ValueError("LPIPS: normalize=True is not built (inputs are in [-1, 1])")
        if self.params is None:
            raise RuntimeError("LPIPS: no weights loaded (load_state_dict / from_files)")
        if not (x.is_cuda and y.is_cuda):
            raise RuntimeError("LPIPS: CPU tensors are not supported (no CPU fallback)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("LPIPS: not capturable into a graph (cached workspaces, lazily packed weights)")
        if x.shape != y.shape or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1):
            raise ValueError("LPIPS: two tensors [B, H, W] or [B, 1, H, W] of one shape, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
        b, h, w = x.shape[0], x.shape[-2], x.shape[-1]
        if h < MIN_SIZE or w < MIN_SIZE:
            raise ValueError("LPIPS: H and W must be at least %d (got %d x %d): AlexNet's second pool would be empty" % (MIN_SIZE, h, w))
        dev = x.device
        pk = self._device_packs(dev)
        ws = self._workspace(dev, b, h, w)
        img = ws["img"]
        img[:b].copy_(x.reshape(b, h, w))
        img[b:].copy_(y.reshape(b, h, w))
        out = torch.empty((b, 5), dtype=torch.float64, device=dev)
        sizes = feature_sizes(h, w)
        one_tap = [ops.pack_tap(0, 0, 0)]
        # conv1 (+ scaling layer): two-plane im2col, then a 1-tap GEMM over K = 256 with bias + ReLU
        col = ops.im2col_pack(img, ws["ones"], 11, 4, 2, ops.PAD_ZERO, torch.float32, 256, out=ws["col"])
        f = ws["f"][0]
        ops.conv_igemm(col, pk["w"][0], pk["npad"][0], f, pk["b"][0], 64, sizes[0][0], sizes[0][1], 0, 0, 1, 1, ops.PAD_ZERO,
                       ops.ACT_RELU, one_tap)
        ops.lpips_layer(f, pk["lin"][0], 0, out, ws["part"])
        for k in range(1, 5):
            cout, _, ks, _, pad = CONVS[k]
            src = ops.maxpool3s2_fwd(f, ws["pool"][k - 1]) if k <= 2 else f
            f = ws["f"][k]
            taps = [ops.pack_tap(ky - pad, kx - pad, ky * ks + kx) for ky in range(ks) for kx in range(ks)]
            ops.conv_igemm(src, pk["w"][k], pk["npad"][k], f, pk["b"][k], cout, sizes[k][0], sizes[k][1], 0, 0, 1, 1, ops.PAD_ZERO,
                           ops.ACT_RELU, taps)
            ops.lpips_layer(f, pk["lin"][k], k, out, ws["part"])
        return out if ret_per_layer else out.sum(1)

    __call__ = forward
