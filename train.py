#!/usr/bin/python3
"""Entry point with the reference's CLI: `python train.py --config Yaml/HdGan.yaml` (reference train.py:31-50).

Picks the trainer by `config['name']`, seeds like the reference's `seed_everything(42)` and runs `train()`
on the MI355X path.  Extra flags (not in the reference): --stage {1,2} selects Hd_Trainer_x1/x2 (the reference
asks the user to rename the class by hand, train.py:42); --steps N limits the synthetic run; --bf16 / --dtype select the
compute mode (default bf16x3: the fastest one inside the reference's fp32 tolerance on outputs and gradients; bf16x3f: the same
forward with a bf16 backward); --test runs `trainer.test()` (generator
inference + device-side windowed / raw MAE, PSNR, SSIM, UQI, and LPIPS when the config names `lpips_weights`; the reference's
train.py:45 calls test()) instead of train() -- the DICOM container of its export is not part of this build; with `export_root` in the config test() saves every slice's int16
pixels as .npy (`export_png`: + the 8-bit window as .png), and predict.py translates a whole HU series from the command line.  train() validates every fifth epoch (PSNR / SSIM, on synthetic pairs here) and puts
both numbers into that epoch's checkpoint names, as the reference does.
"""
import argparse
import os
import random

import numpy as np
import torch
import yaml


def get_config(path):
    with open(path, "r") as stream:
        return yaml.safe_load(stream)   # the reference's bare yaml.load(stream) raises on PyYAML >= 6


def seed_everything(seed):
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, default="Yaml/HdGan.yaml", help="Path to the config file.")
    parser.add_argument("--stage", type=int, default=2, choices=[1, 2])
    parser.add_argument("--steps", type=int, default=None, help="synthetic steps per epoch (no DICOM reader here)")
    parser.add_argument("--epochs", type=int, default=None, help="override n_epochs (+0 decay epochs)")
    parser.add_argument("--bf16", action="store_true")
    parser.add_argument("--dtype", choices=["fp32", "bf16", "bf16x3", "bf16x3f"], default=None,
                        help="compute mode.  Default bf16x3: split-pair storage with split-bf16 contractions -- the fastest mode whose "
                             "generator output AND gradients stay at the reference's fp32 arithmetic (output 4e-5 rel-L2, gradients as "
                             "close as the fp32 mode's); bf16x3f: the same forward (same output, same losses) with a plain bf16 "
                             "backward -- gradients 1.5e-2 rel-L2 from the reference's, 1.4x faster; fp32: exact-f32 MFMA; "
                             "bf16: bf16 storage + MFMA (2.2x faster than bf16x3, output 2e-2 from the reference)")
    parser.add_argument("--test", action="store_true", help="run trainer.test() instead of train()")
    opts = parser.parse_args()
    config = get_config(opts.config)
    from cta_gan_amd import _lib, dp, nets
    from trainer import Cyc_Trainer, Hd_Trainer_x1, Hd_Trainer_x2, P2p_Trainer, Reg_Trainer
    _lib.load()           # builds a stale kernel library BEFORE the process group exists (ranks serialise on a file lock)
    dp.init_from_env()
    mode = opts.dtype or ("bf16" if opts.bf16 else "bf16x3")
    nets.set_default_compute_dtype({"fp32": torch.float32, "bf16": torch.bfloat16}.get(mode, mode))
    if dp.rank() == 0:
        # (the reference computes in fp32; what a run without --dtype computes in is said out loud -- ADVICE r5)
        print("compute mode: %s%s" % (nets.compute_mode(), "" if opts.dtype or opts.bf16 else " (default; --dtype fp32 is the reference's own "
                                                                                              "arithmetic)"), flush=True)
    if opts.steps is not None:
        config["synthetic_steps"] = opts.steps
    if opts.epochs is not None:
        config["n_epochs"], config["decay_epoch"] = opts.epochs, 0
    if config["name"] == "CycleGan":
        trainer = Cyc_Trainer(config)
    elif config["name"] == "HdGan":
        trainer = (Hd_Trainer_x2 if opts.stage == 2 else Hd_Trainer_x1)(config)
    elif config["name"] == "P2p":
        trainer = P2p_Trainer(config)
    elif config["name"] in ("Reg", "RegGan"):   # the reference ships no yaml (and no train.py branch) for this trainer
        trainer = Reg_Trainer(config)
    else:
        raise SystemExit("config name %r: expected HdGan, CycleGan, P2p or Reg" % config["name"])
    if opts.test:
        trainer.test()
        return
    if dp.rank() == 0:
        # train.py has no DICOM loader: it trains on synthetic batches, which are never augmented (only host batches handed to
        # trainer.train(dataloader) are)
        print("noise_level: %s (RandomAffine of the training loaders; the synthetic batches of this run are not augmented)"
              % trainer.augment.level, flush=True)
    trainer.train()
    torch.cuda.synchronize()
    print("done:", {k: float(v.detach()) for k, v in trainer.last.items() if v is not None and v.dim() == 0})


if __name__ == "__main__":
    seed_everything(seed=42)
    main()
