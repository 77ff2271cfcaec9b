"""Step bodies of the reference's CTA-GAN trainers on the HIP path.

`Hd_Trainer_x1` = stage 1 (trainer/HdTrainer.py:94-240: `Discriminator` + plain MSE),
`Hd_Trainer_x2` = stage 2 (:605-763: `Discriminator_m` + `GANLoss` + masked L1); `Hd_Trainer_x` is the
alias train.py:42-43 asks the user to create by hand.  Constructor takes the same yaml dict.  Only the
per-batch body (`train_step`) and a minimal `train()` loop are provided; data loading from DICOM lists,
validation metrics, Visdom logging and DICOM export are out of scope.
"""
from __future__ import annotations

import torch

from ..Model.HdGan import DataPrefetcher
from .. import dp, ops, optim, synth
from ..Model.HdGan import Discriminator, Discriminator_m, GANLoss, Generator
from ..nets import add_scalars, l1_loss, masked_l1_loss
from .augment import NoiseAugmenter
from .reg import Reg
from .transformer import Transformer_2D
from .utils import smooothing_loss


class _frozen:
    """Context manager: parameters of `module` do not require grad inside (their gradient would be thrown away)."""

    def __init__(self, module):
        self.params = [p for p in module.parameters() if p.requires_grad]

    def __enter__(self):
        for p in self.params:
            p.requires_grad_(False)

    def __exit__(self, *exc):
        for p in self.params:
            p.requires_grad_(True)
        return False


_NO_D_BATCH = bool(__import__("os").environ.get("CTG_NO_D_BATCH"))   # A/B switch (scripts/ab.sh)
_SIDE_STREAM = not __import__("os").environ.get("CTG_NO_SIDE_STREAM")   # adversarial branch of the G step on a second HIP stream


def run_epoch_steps(trainer, it):
    """The step loop of one epoch.  Every `config['nie_check_every']` steps (default 50; 0: never) the failure flag of the fused
    conv + InstanceNorm launches is read -- one device synchronisation per 50 steps -- so that a bounded wait that ran out stops the
    run within 50 optimiser steps instead of at the end of the epoch (ops.nie_check raises on every rank)."""
    every = int(trainer.config.get("nie_check_every", 50))
    for i, batch in enumerate(it):
        trainer.train_step({k: v for k, v in batch.items() if torch.is_tensor(v)})
        if every > 0 and (i + 1) % every == 0:
            ops.nie_check("step %d of the epoch" % (i + 1))


class side_branch:
    """`with side_branch(trainer) as br: ...` runs the enclosed forward launches on the trainer's second HIP stream (autograd
    later replays their backward there too); `br.join()` makes the main stream wait before it consumes the results.
    For branches that only share an input with what the main stream does meanwhile -- the frozen-discriminator
    (adversarial) branches of the generator steps.  A no-op under stream capture or with CTG_NO_SIDE_STREAM."""

    def __init__(self, trainer):
        self.on = _SIDE_STREAM and not torch.cuda.is_current_stream_capturing()   # module switch read per use (tests flip it)
        if self.on:
            if getattr(trainer, "_side", None) is None:
                trainer._side = torch.cuda.Stream()
            self.side = trainer._side

    def __enter__(self):
        if self.on:
            self.cur = torch.cuda.current_stream()
            self.side.wait_stream(self.cur)
            torch.cuda.set_stream(self.side)
        return self

    def __exit__(self, *exc):
        if self.on:
            torch.cuda.set_stream(self.cur)
        return False

    def join(self):
        if self.on:
            self.cur.wait_stream(self.side)


def synced_losses(last):
    """The `sync_losses=True` return of every trainer's train_step: the scalar loss terms as floats (this synchronises with the
    device), after the check that no fused conv + InstanceNorm launch of the step gave up waiting (ops.nie_check raises)."""
    out = {k: float(v.detach()) for k, v in last.items() if v is not None and v.dim() == 0}
    ops.nie_check("train_step")
    return out


def to_windowdata(image, WC, WW):
    """trainer/HdTrainer.py:41-64 on device tensors: (B, ..., H, W) in [-1, 1] -> CT window (WC, WW) -> [-1, 1]."""
    return ops.to_windowdata(image, WC, WW)


VAL_EVERY = 5      # `if epoch%5==0` (HdTrainer.py:242, 765; CycTrainer.py:203; p2pTrainer.py:153; RegTrainer.py:206)


def run_validation(trainer, val_iter, keys):
    """The in-training validation pass (HdTrainer.py:765-783 and its siblings): the generator over the validation batches without
    gradients, `PSNR(fake_B, real_B)` (:566-580) and `measure.compare_ssim(fake_B, real_B)` per slice -- both on the device
    (`ops.val_psnr`, `ops.ssim`: csrc/metrics.hip; the reference pulls every slice to the host) --, their means printed as the
    reference prints them.  Returns (PSNR, SSIM, slices); the reference's loader yields one slice per batch, here every slice of
    a batch counts once."""
    tot = torch.zeros(2, dtype=torch.float64, device=trainer.device)
    num = 0
    with torch.no_grad():
        for batch in val_iter:
            real_A = batch[keys[0]].to(trainer.device, non_blocking=True)
            real_B = batch[keys[1]].to(trainer.device, non_blocking=True)
            fake_B = trainer.netG_A2B(real_A).float()
            tot[0] += ops.val_psnr(fake_B, real_B).sum()
            tot[1] += ops.ssim(fake_B, real_B).sum()
            num += real_A.shape[0]
    if num == 0:
        return None
    res = (tot / num).cpu().numpy()
    ops.nie_check("validation pass")
    print("PSNR:", res[0])
    print("SSIM:", res[1])
    return float(res[0]), float(res[1]), num


def validate_if_due(trainer, epoch, dataloader, val_dataloader, keys):
    """Every fifth epoch: `run_validation` over `val_dataloader` (the reference's `self.val_data`, built from config['val_list']);
    a synthetic run (no training dataloader) validates on `config.get('synthetic_val_steps', 2)` synthetic batches.  A run with a
    training dataloader but no validation one skips the pass (plain checkpoint names)."""
    if epoch % VAL_EVERY:
        return None
    if val_dataloader is None:
        if dataloader is not None:
            return None
        val_dataloader = (trainer.synthetic_batch(100000 + i) for i in range(trainer.config.get("synthetic_val_steps", 2)))
    return run_validation(trainer, val_dataloader, keys)


def save_epoch(trainer, epoch, files, optimizers, val=None, val_suffix=".pth"):
    """End-of-epoch checkpoints with the reference's file names (HdTrainer.py:785-803, CycTrainer.py:222-236,
    p2pTrainer.py:169-184, RegTrainer.py:225-240): `files` maps a file stem to a module; `save_root + stem + str(epoch) +
    ".pth"` holds its state_dict (same keys and shapes as the reference's, so either side loads the other's files).  With
    `val` = (PSNR, SSIM, ...) of `run_validation` -- every fifth epoch -- the name is the reference's
    `str(epoch) + '_' + str(round(PSNR, 4)) + '_' + str(round(SSIM, 4))` + `val_suffix` ("b.pth" in HdTrainer.py:785-790, ".pth"
    in the other trainers).  The FORM of the name is the reference's; its digits are not bit-comparable with a reference run on
    the same weights: the PSNR mean is accumulated in float64 on the device (the reference: np.mean over float32 arrays), the SSIM is
    a restatement of skimage with no reference fixture to pin it ("parity unpinned", tests/test_metrics.py), and under data
    parallelism rank 0 names the files from ITS validation batches.  Rank 0 writes.  Extra (the reference cannot resume): `train_state_<epoch>.pth` holds the optimisers'
    state, the learning rates and the weight files' names for `resume()`.  Skipped without `config['save_root']`."""
    import os
    # end of an epoch (and so of train()): the one place every trainer stops anyway -- a fused conv + InstanceNorm launch whose
    # bounded wait ran out must not go unnoticed (raises; see ops.nie_check)
    ops.nie_check("end of epoch %s" % epoch)
    root = trainer.config.get("save_root")
    if not root or not trainer.config.get("save_checkpoints", True):
        return
    if dp.world_size() > 1 and torch.distributed.get_rank() != 0:
        return
    os.makedirs(root, exist_ok=True)
    st, suffix = str(epoch), ".pth"
    if val is not None:
        st, suffix = str(epoch) + "_" + str(round(val[0], 4)) + "_" + str(round(val[1], 4)), val_suffix
    names = {}
    for stem, module in files.items():
        names[stem] = stem + st + suffix
        torch.save(module.state_dict(), root + names[stem])
    torch.save({"epoch": epoch, "lr": trainer.config.get("lr"), "lrd": trainer.config.get("lrd"), "files": names,
                "val": None if val is None else {"PSNR": val[0], "SSIM": val[1], "slices": val[2]},
                "optimizers": {k: o.state_dict() for k, o in optimizers.items()}}, root + "train_state_" + str(epoch) + ".pth")


def resume_epoch(trainer, epoch, files, optimizers):
    """Load what `save_epoch(trainer, epoch, ...)` wrote (weights + optimiser state) and set config['epoch'] = epoch."""
    root = trainer.config["save_root"]
    st = str(epoch)
    state = torch.load(root + "train_state_" + st + ".pth", map_location=trainer.device)
    names = state.get("files") or {}       # (validated epochs carry PSNR / SSIM in their names)
    for stem, module in files.items():
        module.load_state_dict(torch.load(root + names.get(stem, stem + st + ".pth"), map_location=trainer.device))
    for k, o in optimizers.items():
        o.load_state_dict(state["optimizers"][k])
    for k in ("lr", "lrd"):
        if state.get(k) is not None:
            trainer.config[k] = state[k]
    trainer.config["epoch"] = epoch


def _export_batch(fake_B, wc, ww, paths, first, root, png):
    """One batch of the test() loop's export: `<root>/<stem>.npy` (int16) per slice, and `<stem>.png` (uint8 level) with `png`."""
    import os
    import numpy as np
    pix, level = ops.export_slices(fake_B, wc, ww, want_level=png)
    pix = pix.cpu().numpy()
    level = level.cpu().numpy() if png else None
    if isinstance(paths, str):
        paths = [paths]
    os.makedirs(root, exist_ok=True)
    for i in range(pix.shape[0]):
        stem = "%06d" % (first + i)
        if paths is not None and i < len(paths):
            stem = os.path.splitext(os.path.basename(str(paths[i])))[0]
        np.save(os.path.join(root, stem + ".npy"), pix[i])
        if png:
            from PIL import Image
            Image.fromarray(level[i]).save(os.path.join(root, stem + ".png"))      # uint8 [H, W]: mode "L"


def run_test_loop(trainer, dataloader, keys, ckpt_name, aliased, uqiw_label="UQIW:"):
    """The inference + metrics loop shared by the trainers' `test()` (HdTrainer.py:951-1087, CycTrainer.py:238-398,
    p2pTrainer.py:186-312, RegTrainer.py:242-380): load `save_root/ckpt_name` into the generator if it exists, run the
    generator over the batches (dicts holding `keys` = (input, target), optionally per-slice 'WC' / 'WW') and average the
    windowed and raw MAE / PSNR / SSIM / UQI on the device.  `aliased`: the reference's `bb = b` / `cc = c` aliasing (Cyc, P2p).
    With `config['lpips_weights']` (one path: the full `lpips.LPIPS(net='alex')` state dict; or {'alexnet': path, 'lins': path}: a
    torchvision AlexNet state dict + lpips' weights/v0.1/alex.pth) the loop also reports `LPIPSw` / `LPIPS`, the reference's
    `loss_fn_alex.forward` on the windowed and on the raw masked pair (HdTrainer.py:504-513, 531-536), from `cta_gan_amd.lpips` on
    the planes `ops.window_pairs` writes; with `aliased` the windowed pair is the two +-1 masks, as in the reference.  Without the
    key nothing of it is imported, computed or printed.
    The DICOM container of the same loop's export is not part of this build; the export's
    pixels are, behind `config['export_root']` (absent: nothing is written): every slice's `newimg.astype(np.int16)`
    (HdTrainer.py:539-543) is saved as `<export_root>/<stem>.npy`, <stem> = the basename of `batch['A_path'][i]` without its
    extension or a running %06d index, plus `<stem>.png` (the 8-bit window level) with `config['export_png']`; rank 0 writes."""
    import os
    cfg = trainer.config
    ckpt = os.path.join(cfg.get("save_root", ""), ckpt_name)
    if cfg.get("save_root") and os.path.exists(ckpt):
        trainer.netG_A2B.load_state_dict(torch.load(ckpt, map_location=trainer.device))
    it = dataloader if dataloader is not None else (
        trainer.synthetic_batch(i) for i in range(cfg.get("synthetic_steps", 4)))
    total = torch.zeros(2, 3, dtype=torch.float64, device=trainer.device)
    total_ssim = torch.zeros(2, dtype=torch.float64, device=trainer.device)
    lp = total_lpips = None
    if cfg.get("lpips_weights"):
        from ..lpips import LPIPS
        lp = LPIPS.from_config(cfg["lpips_weights"])
        total_lpips = torch.zeros(2, dtype=torch.float64, device=trainer.device)
    num = 0
    export_root = cfg.get("export_root")
    if export_root and dp.world_size() > 1 and torch.distributed.get_rank() != 0:
        export_root = None
    with torch.no_grad():
        for batch in it:
            real_A = batch[keys[0]].to(trainer.device, non_blocking=True)
            real_B = batch[keys[1]].to(trainer.device, non_blocking=True)
            wc = batch.get("WC", cfg.get("WC", 40.0))
            ww = batch.get("WW", cfg.get("WW", 400.0))
            fake_B = trainer.netG_A2B(real_A)
            total += ops.window_metrics(fake_B, real_B, wc, ww, aliased=aliased).sum(0)
            total_ssim += ops.window_ssim(fake_B, real_B, wc, ww, aliased=aliased).sum(0)      # HdTrainer.py:1028, 1053
            if lp is not None:
                pairs = ops.window_pairs(fake_B, real_B, wc, ww, aliased=aliased)      # [c, fake_m, b, real_m]
                n, (h, w) = pairs.shape[1], pairs.shape[2:]
                total_lpips += lp(pairs[:2].reshape(2 * n, h, w), pairs[2:].reshape(2 * n, h, w)).reshape(2, n).sum(1)
            if export_root:
                _export_batch(fake_B, wc, ww, batch.get("A_path"), num, export_root, bool(cfg.get("export_png")))
            num += real_A.shape[0]
    res = (total / max(num, 1)).cpu().numpy()
    res_ssim = (total_ssim / max(num, 1)).cpu().numpy()
    ops.nie_check("test loop")      # the generator forwards above ran fused conv + InstanceNorm launches: none may have given up
    out = {"MAEw": res[0, 0], "PSNRw": res[0, 1], "UQIw": res[0, 2], "MAE": res[1, 0], "PSNR": res[1, 1],
           "UQI": res[1, 2], "SSIMw": res_ssim[0], "SSIM": res_ssim[1], "num": num}
    if lp is not None:
        res_lpips = (total_lpips / max(num, 1)).cpu().numpy()
        out["LPIPSw"], out["LPIPS"] = res_lpips[0], res_lpips[1]
    print("MAEw", out["MAEw"]); print("PSNRw:", out["PSNRw"]); print("SSIMw:", out["SSIMw"])
    if lp is not None:
        print("LPIPSw:", out["LPIPSw"])
    print(uqiw_label, out["UQIw"]); print("\n")
    print("MAE:", out["MAE"]); print("PSNR:", out["PSNR"]); print("SSIM:", out["SSIM"])
    if lp is not None:
        print("LPIPS:", out["LPIPS"])
    print("UQI:", out["UQI"])
    return out


class _HdBase:
    stage = 2

    def __init__(self, config):
        self.config = config
        dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.netG_A2B = Generator(config["input_nc"], config["output_nc"]).to(dev)
        self.netD_B = (Discriminator_m if self.stage == 2 else Discriminator)(config["input_nc"]).to(dev)
        if self.stage == 2:
            self.netD_B.patch_only = True      # GANLoss reads feats[-1] only (Model/HdGan.py:276-290)
        self.R_A = Reg(config["size"], config["size"], config["input_nc"], config["input_nc"]).to(dev)
        self.spatial_transform = Transformer_2D().to(dev)
        dp.broadcast_params(self.netG_A2B, self.netD_B, self.R_A)
        cap = bool(config.get("hip_graph", False))
        self.optimizer_D_B = optim.Adam(self.netD_B.parameters(), lr=config["lrd"], betas=(0.5, 0.999), capturable=cap)
        self.optimizer_R_A = optim.Adam(self.R_A.parameters(), lr=config["lr"], betas=(0.5, 0.999), capturable=cap)
        self.optimizer_G = optim.Adam(self.netG_A2B.parameters(), lr=config["lr"], betas=(0.5, 0.999), capturable=cap)
        self.criterionGAN = GANLoss()
        self.last = {}
        # the loaders' RandomAffine (`noise_level`; absent or 0: none), applied by train() to host batches only
        self.augment = NoiseAugmenter(config.get("noise_level", 0), config["size"], seed=config.get("seed", 0))
        self._graph = None      # (CUDAGraph, static batch) once captured (config['hip_graph'])
        import weakref
        ops.NIE_ON_FAILURE.append(weakref.WeakMethod(self._drop_graph))

    # -- reference: update_learning_rate (HdTrainer.py:670-684), reproduced with its quirks: the decrement is
    #    recomputed from the already-decayed lr, and D's group gets a key ('lrd') Adam never reads.
    def update_learning_rate(self):
        lrd = self.config["lr"] / self.config["decay_epoch"]
        lr = self.config["lr"] - lrd
        lr2 = self.config["lrd"] - lrd
        for g in self.optimizer_D_B.param_groups:
            g["lrd"] = lr2
        for g in self.optimizer_R_A.param_groups:
            g["lr"] = lr
        for g in self.optimizer_G.param_groups:
            g["lr"] = lr
        self.config["lr"] = lr

    def train_step(self, batch, sync_losses: bool = False):
        """One G+R step and one D step on a dict batch of device tensors A2, B1, B2 (each (B,1,S,S) fp32).

        With `config['hip_graph']` the whole step (~1500 kernel launches, Adam included) is captured ONCE into a
        hipGraph after three eager warm-up steps and replayed afterwards: at the reference's batchSize of 1-4 the
        eager step is bound by host launch overhead, not by the GPU."""
        if self.config.get("hip_graph", False) and not dp.enabled():
            return self._graph_step(batch, sync_losses)
        return self._eager_step(batch, sync_losses)

    def _graph_step(self, batch, sync_losses):
        from .. import nets
        opts = (self.optimizer_G, self.optimizer_R_A, self.optimizer_D_B)
        # what a captured step bakes in: the rates (launch constants of the captured Adam) and the compute dtype;
        # update_learning_rate() or set_default_compute_dtype() make the next step re-capture
        lrs = tuple(g["lr"] for o in opts for g in o.param_groups) + (nets.compute_mode(),)
        if self._graph is not None and self._graph[2] != lrs:
            self._graph = None
        if self._graph is not None and any(tuple(batch[k].shape) != tuple(v.shape) or batch[k].dtype != v.dtype
                                           for k, v in self._graph[1].items()):
            # another batch shape (the trailing batch of an epoch): `copy_` would broadcast it into the captured tensors
            # and train on duplicated slices -- this batch runs eagerly, the graph stays for the regular ones
            return self._eager_step(batch, sync_losses)
        if self._graph is None:
            self._warm = getattr(self, "_warm", 0) + 1
            if self._warm <= 3:
                return self._eager_step(batch, sync_losses)
            static = {k: v.clone() for k, v in batch.items() if k in ("A2", "B1", "B2")}
            for m in (self.netG_A2B, self.netD_B, self.R_A):
                for sub in [m] + list(getattr(m, "_scales", [])):
                    sub._cache.store.clear()
            # drop the warm-up step's result handles (and the tapes they keep alive) BEFORE capture: releasing them in
            # the middle of the capture while the captured step's own handles survive it crashed hipStreamEndCapture
            self.last = None
            for o in opts:
                o.prepare_capture()
            from .. import ops
            ops.nie_prepare_capture(static["A2"].device)      # the fused conv + InstanceNorm launches' counters: not graph-pool memory
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._eager_step(static, False)
            # the captured step's result handles: every replay rewrites THESE tensors, so `self.last` is pointed back at
            # them after a replay (an eager detour for a batch of another shape rebinds it to eager tensors meanwhile)
            self._graph = (g, static, lrs, self.last)
            # packed weights cached during capture live in the graph's private pool: never reuse them eagerly
            for m in (self.netG_A2B, self.netD_B, self.R_A):
                m._cache.store.clear()
        g, static, _, captured_last = self._graph
        for k, v in static.items():
            v.copy_(batch[k], non_blocking=True)
        g.replay()
        self.last = captured_last
        for o in opts:
            o.note_replayed()
        if sync_losses:
            return synced_losses(self.last)
        return None

    def _eager_step(self, batch, sync_losses: bool = False):
        cfg = self.config
        real_A2, real_B2 = batch["A2"], batch["B2"]
        real_BB2 = real_B2  # the reference deep-copies because it later rebinds real_B2; nothing here mutates it
        self.optimizer_R_A.zero_grad()
        self.optimizer_G.zero_grad()
        fake_B = self.netG_A2B(real_A2)
        # D's own weight gradients of this pass are discarded by optimizer_D_B.zero_grad() below (HdTrainer.py:741)
        # before anything reads them, so they are not computed: only d(adv)/d(fake_B) flows through D here
        # the adversarial branch only shares fake_B with the registration branch: second stream, beside Reg's many small
        # low-resolution launches (interleaved A/B in one box: 54.67 -> 53.60 ms/step)
        with side_branch(self) as adv_branch:
            with _frozen(self.netD_B):
                pred_fake0 = self.netD_B(fake_B)
            # the loss weights of Yaml/HdGan.yaml:10-15 ride the fused reductions (no scalar-multiply launches around them)
            if self.stage == 1:
                adv_loss = cfg["Adv_lamda1"] * ((pred_fake0 - 1.0) ** 2).mean()
            else:
                adv_loss = self.criterionGAN(pred_fake0, True, weight=cfg["Adv_lamda1"])
        trans = self.R_A(fake_B, real_B2)
        sys_regist = self.spatial_transform(fake_B, trans)
        sm_loss = smooothing_loss(trans, weight=cfg["Smooth_lamda"])
        sr_loss = l1_loss(sys_regist, real_B2, weight=cfg["Corr_lamda1"])
        adv_branch.join()      # adv_loss joins the sum on the main stream
        if self.stage == 1:
            total = add_scalars(sm_loss, adv_loss, sr_loss)
            sr_loss2 = None
        else:
            # HdTrainer.py:726-735 fused: bb = (B1 >= 0.3); both operands masked, zeros -> -1, L1
            sr_loss2 = masked_l1_loss(sys_regist, real_B2, batch["B1"], weight=cfg["Corr_lamda2"])
            total = add_scalars(sm_loss, adv_loss, sr_loss, sr_loss2)      # HdTrainer.py:736, one launch
        sync = self._grad_sync()
        if sync is not None:
            sync["G"].begin()      # the weight-gradient kernels write into the exchange buckets from here on
        total.backward()
        if sync is not None:
            sync["G"].finish()     # {Reg}, {G late half}, {G early half} were launched from inside the backward
        self.optimizer_R_A.step()
        self.optimizer_G.step()

        self.optimizer_D_B.zero_grad()
        with torch.no_grad():
            fake_B = self.netG_A2B(real_A2)
        # D(fake) and D(real) as ONE pass over the concatenated batch: every layer of D is per-sample (InstanceNorm,
        # no BatchNorm), so the two halves are exactly the reference's two separate calls (HdTrainer.py:744-745)
        nb = fake_B.shape[0]
        pred_both = None
        if _NO_D_BATCH:
            pred_fake0, pred_real = self.netD_B(fake_B), self.netD_B(real_BB2)
        else:
            pred_both = self.netD_B(torch.cat([fake_B, real_BB2.to(fake_B.dtype)], 0))
            if self.stage == 1:
                pred_fake0, pred_real = pred_both[:nb], pred_both[nb:]
        if self.stage == 1:
            loss_D_B = cfg["Adv_lamda1"] * (pred_fake0 ** 2).mean() + cfg["Adv_lamda1"] * ((pred_real - 1.0) ** 2).mean()
        elif pred_both is not None:
            # Adv * (GANLoss(fake, False) + GANLoss(real, True)) / 2 over the two halves of the batched pass: one fused reduction
            loss_D_B = self.criterionGAN.pair(pred_both, nb, weight=cfg["Adv_lamda1"] / 2)
        else:
            loss_D_B = add_scalars(self.criterionGAN(pred_fake0, False, weight=cfg["Adv_lamda1"] / 2),
                                   self.criterionGAN(pred_real, True, weight=cfg["Adv_lamda1"] / 2))
        if sync is not None:
            sync["D"].begin()
        loss_D_B.backward()
        if sync is not None:
            sync["D"].finish()
        self.optimizer_D_B.step()
        self.last = dict(SM=sm_loss, SR=sr_loss, adv=adv_loss, SR2=sr_loss2, total=total, loss_D=loss_D_B,
                         fake_B=fake_B, flow=trans, warped=sys_regist)
        if sync_losses:
            return synced_losses(self.last)
        return None

    def _grad_sync(self):
        """Data-parallel gradient exchange of the two optimiser steps (None in a single-process run): persistent flat
        buckets in backward order -- {Reg} completes when Reg's backward ends (before the generator's starts), the
        generator's two halves at its "mid" mark and at its end; {D} is reduced after the D step's backward."""
        if not dp.enabled() or __import__("os").environ.get("CTG_DP_NO_SYNC"):     # (A/B knob: process group without exchange)
            return None
        if getattr(self, "_sync", None) is None:
            g = self.netG_A2B
            buckets = [(list(self.R_A.parameters()), (self.R_A, "done"))]
            if __import__("os").environ.get("CTG_DP_ONE_G_BUCKET"):      # A/B knob: the generator as ONE bucket, launched at its end
                buckets += [(list(g.parameters()), (g, "done"))]
            else:
                buckets += [(ps, (g, tag)) for ps, tag in g.grad_buckets()]
            self._sync = {"G": dp.GradSync(buckets), "D": dp.GradSync([(list(self.netD_B.parameters()), None)])}
        return self._sync

    def synthetic_batch(self, seed=1234):
        b, s = self.config["batchSize"], self.config["size"]
        tag = "_r%d" % dp.rank() if dp.world_size() > 1 else ""      # replicas train on different slices
        return {k: synth.synth_images("hd_%s_%d%s" % (k, seed, tag), b, s).to(self.device) for k in ("A2", "B1", "B2")}

    def _drop_graph(self):
        self._graph = None

    def train(self, dataloader=None, val_dataloader=None):
        """Epoch loop of HdTrainer.py:695-803 over `dataloader` (an iterable of dict batches); without one, runs
        `config.get('synthetic_steps', 4)` steps on synthetic pairs per epoch (no DICOM reader on this path).  Stage 2 starts
        from the stage-1 generator / registration weights when `save_root` holds them (HdTrainer.py:697-699); every fifth epoch
        runs the validation pass (:765-783, `validate_if_due`) and every epoch ends with the reference's checkpoint files
        (`save_epoch`: PSNR / SSIM spliced into the validated epochs' names, :785-790)."""
        import os
        if self.config.get("hip_graph") is None and self.config.get("batchSize", 16) <= 2 and not dp.enabled():
            # the reference's shipped batch sizes (Yaml/HdGan.yaml:19: batchSize 1) leave the GPU waiting for launches:
            # replay the step as a hipGraph (B=1: 15.6 -> 13.1 ms/step, B=2: 15.9 -> 14.7; 300-step soak:
            # scripts/graph_soak.py).  `hip_graph: false` in the yaml keeps it eager.
            self.config["hip_graph"] = True
            for o in (self.optimizer_G, self.optimizer_R_A, self.optimizer_D_B):
                o.capturable = True
        root = self.config.get("save_root")
        if self.stage == 2 and root and self.config["epoch"] == 0 and os.path.exists(root + "netG_A2B_x_45.pth") and os.path.exists(root + "R_A_x_45.pth"):
            self.netG_A2B.load_state_dict(torch.load(root + "netG_A2B_x_45.pth", map_location=self.device))
            self.R_A.load_state_dict(torch.load(root + "R_A_x_45.pth", map_location=self.device))
        for epoch in range(self.config["epoch"] + 1, self.config["n_epochs"] + 1 + self.config["decay_epoch"]):
            if epoch > self.config["n_epochs"]:
                self.update_learning_rate()
            it = dataloader if dataloader is not None else (
                self.synthetic_batch(i) for i in range(self.config.get("synthetic_steps", 4)))
            if dataloader is not None:
                # host batches: pinned, double-buffered H2D on a copy stream, one batch ahead of the step that trains
                # ... and, at noise_level > 0, the loaders' RandomAffine behind each copy on that stream (trainer/augment.py)
                it = DataPrefetcher(it, device=self.device, transform=self.augment if self.augment.level > 0 else None)
            run_epoch_steps(self, it)
            val = validate_if_due(self, epoch, dataloader, val_dataloader, self._val_keys)
            save_epoch(self, epoch, self._ckpt_files(), self._ckpt_optimizers(), val=val, val_suffix=self._val_suffix)

    _val_keys = ("A2", "B2")       # HdTrainer.py:771-774
    _val_suffix = "b.pth"          # HdTrainer.py:785-790

    def _ckpt_files(self):
        return {"netG_A2B_x_": self.netG_A2B, "R_A_x_": self.R_A, "netD_B_x_": self.netD_B}

    def _ckpt_optimizers(self):
        return {"G": self.optimizer_G, "R_A": self.optimizer_R_A, "D_B": self.optimizer_D_B}

    def resume(self, epoch):
        """Continue from the files `train()` wrote at the end of `epoch` (weights, Adam moments and step counts, rates)."""
        resume_epoch(self, epoch, self._ckpt_files(), self._ckpt_optimizers())

    def test(self, dataloader=None):
        """Inference + metrics loop of HdTrainer.py:951-1087 with everything after the generator kept on the device:
        windowing (`to_windowdata`), the 0.3-threshold masks and MAE / PSNR / UQI (both the windowed and the raw pair)
        are one reduction launch per batch instead of a D2H copy + numpy per slice.  Batches are dicts with 'A2', 'B2'
        (B,1,S,S) and optionally per-slice 'WC' / 'WW' (the reference reads them from the DICOM header; default:
        config['WC'], config['WW'] or 40 / 400).  Without a dataloader, `config.get('synthetic_steps', 4)` synthetic
        batches; SSIM / SSIMw (`measure.compare_ssim`, :1028, 1053) come from `ops.window_ssim`, LPIPS / LPIPSw (:1029-1031, 1054-1056) from
        `cta_gan_amd.lpips` when `config['lpips_weights']` names the weight file(s).  The DICOM export is not part of this build.
        If `config['save_root']` holds netG_A2B_x_3.pth it is loaded first, as in the reference."""
        return run_test_loop(self, dataloader, ("A2", "B2"), "netG_A2B_x_3.pth", aliased=False, uqiw_label="UQIw:")


class Hd_Trainer_x1(_HdBase):
    stage = 1


class Hd_Trainer_x2(_HdBase):
    stage = 2


Hd_Trainer_x = Hd_Trainer_x2
