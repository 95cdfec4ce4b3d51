"""Cost of the device-side view augmentation (csrc/augment2d.hip, csrc/augment2d3d.hip, csrc/augment3d.hip), one JSON line:

    python tools/bench_augment.py [--task simsiam3d|simsiam2d3d|aug3d] [--batch 256] [--bbox 36] [--rounds 5] [--small]

  launches_us     the four launches of one batch (two mi_aug2d_params + two mi_aug2d_apply) alone: HIP events around
                  `ViewAugmenter.views`, median of 200 calls after a warm-up (includes the four output allocations)
  apply_us        one mi_aug2d_apply launch per quarter turn k (records k = 0..3 otherwise alike): the k = 1 / 3 LDS reads
                  run down a column of the byte image
  iteration_ms    the SimSiam-2D training iteration as the entry point runs it (`trainer.train(epoch, dataset)`: loader,
                  batch copy, hipGraph replay, meters) with `--augment mirror` and with `--augment reference`, same
                  process, same synthetic tomograms, alternating epochs, --rounds epochs each; `mirror_spread` is the
                  spread between the repeated mirror epochs, the yardstick for the difference

--task simsiam2d3d: the same for the 2d3d mode (simsiam2d3d_18 on tilt + tomogram patch pairs).  `launches_us` is then the
two launches of a batch (mi_aug2d3d_params + mi_aug2d3d_apply, all four tensors) around `PairViewAugmenter.views`,
`params_us` / `apply_us` each launch alone, and `mirror` stands for the unaugmented pairs (the step without the flag).

--task aug3d: the random 3-D views of the MoCo training, a batch of 64 at crop 32 (--batch / --bbox are not used).  `aug3d_ms` is
both views of a batch (mi_aug3d_params + mi_aug3d_apply: three launches, HIP events around `VolumeAugmenter.views`), `cut_ms` the
two `CropTable.cut` launches that make the mirror views of the same samples on the same table, `params_ms` / `apply_ms` the
parts alone, and `iteration_ms` the MoCo-3D training iteration (`trainer.train(epoch, loader)` on the synthetic loader, which
cuts on the training stream) with `--augment mirror` and with `--augment reference`.  A record, not a gate.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _build(augment, batch, bbox, small):
    from cet_pick_amd.datasets.synthetic_datasets import SyntheticSimSiamDataset
    from cet_pick_amd.models.model import create_model
    from cet_pick_amd.opts import opts
    from cet_pick_amd.trains.train_factory import train_factory
    opt = opts().parse(["simsiam3d", "--arch", "simsiam2d_18", "--dataset", "synthetic", "--bbox", str(bbox), "--batch_size", str(batch),
                        "--lr", "0.001", "--debug", "0", "--augment", augment, "--exp_id", "bench_augment"])
    opt = opts().update_dataset_info_and_set_heads(opt, SyntheticSimSiamDataset)
    torch.manual_seed(opt.seed)
    model = create_model(opt.arch, opt.heads, opt.head_conv)
    trainer = train_factory[opt.task](opt, model, torch.optim.SGD(model.parameters(), opt.lr))
    trainer.set_device(opt.gpus, opt.chunk_sizes, torch.device("cuda"))
    shape, n_tomos, cap = ((24, 256, 256), 2, 512) if small else ((48, 512, 512), 4, 2048)
    ds = SyntheticSimSiamDataset(opt, "train", (3, bbox, bbox), sigma1=opt.dog, shape=shape, n_tomos=n_tomos, max_per_tomo=cap)
    return trainer, ds


def _build_2d3d(augment, batch, bbox, small):
    from cet_pick_amd.datasets.simsiam2d3d import SyntheticSimSiam2D3DDataset
    from cet_pick_amd.models.model import create_model
    from cet_pick_amd.opts import opts
    from cet_pick_amd.trains.train_factory import train_factory
    opt = opts().parse(["simsiam2d3d", "--arch", "simsiam2d3d_18", "--dataset", "simsiam2d3d", "--bbox", str(bbox), "--batch_size",
                        str(batch), "--lr", "0.001", "--debug", "0", "--augment", augment, "--exp_id", "bench_augment2d3d"])
    opt = opts().update_dataset_info_and_set_heads(opt, SyntheticSimSiam2D3DDataset)
    torch.manual_seed(opt.seed)
    model = create_model(opt.arch, opt.heads, opt.head_conv)
    trainer = train_factory[opt.task](opt, model, torch.optim.SGD(model.parameters(), opt.lr))
    trainer.set_device(opt.gpus, opt.chunk_sizes, torch.device("cuda"))
    shape, n_tomos = ((32, 256, 256), 2) if small else ((48, 384, 384), 4)
    ds = SyntheticSimSiam2D3DDataset(opt, "train", (3, bbox, bbox), sigma1=opt.dog, shape=shape, n_tomos=n_tomos)
    if len(ds) == 0:
        raise SystemExit("the synthetic 2d3d dataset has %d samples, fewer than one batch of %d" % (ds.num_samples, batch))
    return trainer, ds


def _build_moco(augment):
    from cet_pick_amd import moco_main
    from cet_pick_amd.opts import opts
    opt = opts().parse(["moco", "--arch", "moco3d_18", "--dataset", "synthetic", "--batch_size", "64", "--lr", "0.001", "--debug", "0",
                        "--augment", augment, "--exp_id", "bench_augment3d"])
    _, _, _, trainer, loader, _, _, _ = moco_main.build(opt)
    return trainer, loader


def _main_aug3d(a):
    from cet_pick_amd.datasets import augment as A
    runs = {m: _build_moco(m) for m in ("mirror", "reference")}
    loader = runs["reference"][1]
    B, c = loader.batch_size, loader.crop
    out = {"task": "aug3d", "batch": B, "crop": c, "samples": len(loader.centres), "iterations_per_epoch": len(loader)}
    order = loader.table.epoch_order(np.random.default_rng(1).permutation(len(loader.centres)))
    ids = order[:B]
    aug = loader.augmenter
    cut = lambda: (loader.table.cut(order, 0, B, (c,) * 3), loader.table.cut(order, 0, B, (c,) * 3, shifted=True, flip_x=True))
    for _ in range(20):
        aug.views(ids, 0)
        cut()
    torch.cuda.synchronize()
    out["aug3d_ms"] = _events_us(lambda: aug.views(ids, 0), 200) / 1e3
    out["cut_ms"] = _events_us(cut, 200) / 1e3
    t = A._draw_3d(ids, 317, 0, 0, 2, c, None)
    out["params_ms"] = _events_us(lambda: A._draw_3d(ids, 317, 0, 0, 2, c, None), 200) / 1e3
    out["apply_ms"] = _events_us(lambda: A.apply_3d(loader.table, ids, t, c), 200) / 1e3
    ms = {m: [] for m in runs}
    for m, (trainer, d) in runs.items():                      # warm-up: workspaces, the hipGraph capture
        d.set_epoch(0)
        trainer.train(0, d)
    torch.cuda.synchronize()
    for r in range(1, a.rounds + 1):
        for m, (trainer, d) in runs.items():
            d.set_epoch(r)
            t0 = time.perf_counter()
            trainer.train(r, d)
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) / len(d) * 1e3)
    med = {m: float(np.median(v)) for m, v in ms.items()}
    out["iteration_ms"] = {m: [round(v, 4) for v in ms[m]] for m in ms}
    out["iteration_ms_median"] = med
    out["mirror_spread_ms"] = float(max(ms["mirror"]) - min(ms["mirror"]))
    out["reference_minus_mirror_ms"] = med["reference"] - med["mirror"]
    for trainer, _ in runs.values():
        if trainer.engine is not None:
            trainer.engine.close()
    print(json.dumps(out))


def _events_us(fn, reps):
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="simsiam3d", choices=["simsiam3d", "simsiam2d3d", "aug3d"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bbox", type=int, default=36)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    if a.task == "aug3d":
        return _main_aug3d(a)
    from cet_pick_amd.datasets import augment as A
    build = _build_2d3d if a.task == "simsiam2d3d" else _build
    runs = {m: build(m, a.batch, a.bbox, a.small) for m in ("mirror", "reference")}
    ds = runs["reference"][1]
    out = {"task": a.task, "batch": a.batch, "bbox": a.bbox, "samples": int(ds.num_samples), "iterations_per_epoch": len(ds)}

    # (a) the launches alone
    ids = torch.randperm(ds.num_samples, device="cuda")[:a.batch].contiguous()
    if a.task == "simsiam2d3d":
        aug = ds.augmenter
        var = torch.as_tensor(ds.epoch_views()[1], device="cuda")[ids].contiguous()
        for _ in range(20):
            aug.views(ids, var, 0)
        torch.cuda.synchronize()
        out["launches_us"] = _events_us(lambda: aug.views(ids, var, 0), 200)
        t = A.draw_params_2d3d(ids, 317, 0, a.bbox)
        out["params_us"] = _events_us(lambda: A.draw_params_2d3d(ids, 317, 0, a.bbox), 200)
        out["apply_us"] = _events_us(lambda: A.apply_2d3d(aug.patches_2d, aug.patches_3d, ids, var, t, aug.means, aug.stds), 200)
    else:
        for _ in range(20):
            ds.augmenter.views(ids, 0)
        torch.cuda.synchronize()
        out["launches_us"] = _events_us(lambda: ds.augmenter.views(ids, 0), 200)
        t = A.draw_params(ids, 317, 0, A.STRONG, a.bbox)
        out["params_us"] = _events_us(lambda: A.draw_params(ids, 317, 0, A.STRONG, a.bbox), 200)
        out["apply_us"] = {}
        for k in range(4):
            tk = t.clone()
            tk[:, 6] = k
            out["apply_us"]["k%d" % k] = _events_us(lambda: A.apply(ds.sub_vols_3d, ids, tk, ds.mean_subvols3d, ds.std_subvols3d), 200)

    # (b) the training iteration, alternating
    ms = {m: [] for m in runs}
    for m, (trainer, d) in runs.items():                      # warm-up: workspaces, the hipGraph capture
        d.set_epoch(0)
        trainer.train(0, d)
    torch.cuda.synchronize()
    for r in range(1, a.rounds + 1):
        for m, (trainer, d) in runs.items():
            d.set_epoch(r)
            t0 = time.perf_counter()
            trainer.train(r, d)
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) / len(d) * 1e3)
    med = {m: float(np.median(v)) for m, v in ms.items()}
    out["iteration_ms"] = {m: [round(v, 4) for v in ms[m]] for m in ms}
    out["iteration_ms_median"] = med
    out["mirror_spread_ms"] = float(max(ms["mirror"]) - min(ms["mirror"]))
    out["reference_minus_mirror_ms"] = med["reference"] - med["mirror"]
    for trainer, _ in runs.values():
        trainer.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
