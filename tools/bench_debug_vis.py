"""Cost of the validation pictures of one tomogram (csrc/debug_vis.hip, utils/debug_vis.py), one JSON line and
profiles/debug_vis_bench.json:

    python tools/bench_debug_vis.py [--out profiles/debug_vis_bench.json] [--shape 110x700x700] [--reps 10] [--val_reps 3]
                                    [--parent_debug0_ms MS]
    python tools/bench_debug_vis.py --val_only [--repo DIR]     # only the --debug 0 validation time, of the package under DIR

  minmax_us, render_us       device time (events) of mi_dbgvis_minmax and mi_dbgvis_render over the slices [20, D - 20) of the
                             validation window of the tomogram (110 x 500 x 500 for the default shape), one launch each
  *_bytes, *_tbs             the bytes the kernels must move and the rate that gives
  copy_ms                    the rendered pictures device -> pinned host, one copy
  val_debug4_ms, val_debug0_ms   wall time of TomoCRSemiTrainer.val over one sample (unet_4, untrained) with --debug 4 / --debug 0
  encode_thread_s, pool      seconds inside the PNG encoders summed over the pool's threads during one --debug 4 validation
  encode_share               encode_thread_s / pool over the extra wall time of --debug 4
  bound                      which of render, copy and encode is the longest
  parent_debug0_ms           the --debug 0 validation time of the parent commit on the same machine (measured with --val_only
                             on a checkout of it and passed in)
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--shape", default="110x700x700")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--val_reps", type=int, default=3)
ap.add_argument("--val_only", action="store_true")
ap.add_argument("--parent_debug0_ms", type=float, default=None)
ARGS = ap.parse_args()
REPO = os.path.abspath(ARGS.repo)
sys.path.insert(0, REPO)

HBM_CEILING = 8e12
PREDICTED = {"minmax_us": 25.0, "render_us": 80.0, "copy_ms": 4.2, "encode_ms": 260.0}


def _events_us(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(times)), [round(t, 1) for t in times]


def _trainer_and_sample(vol, coords, work):
    from cet_pick_amd.datasets.semi_files import TomoFileDetectorDataset
    from cet_pick_amd.models.model import create_model
    from cet_pick_amd.opts import opts
    from cet_pick_amd.trains.train_factory import train_factory
    os.chdir(work)
    opt = opts().parse(["semi", "--arch", "unet_4", "--dataset", "semi", "--exp_id", "bench_debug_vis", "--debug", "0",
                        "--print_iter", "0"])
    opt = opts().update_dataset_info_and_set_heads(opt, TomoFileDetectorDataset)
    opt.device = torch.device("cuda", 0)
    torch.manual_seed(opt.seed)
    model = create_model(opt.arch, opt.heads, opt.head_conv, last_k=opt.last_k)
    trainer = train_factory[opt.task](opt, model, None)
    trainer.set_device(opt.gpus, opt.chunk_sizes, opt.device)
    ds = TomoFileDetectorDataset.from_arrays(opt, "val", {"bench": vol}, {"bench": coords}, device=opt.device)
    return opt, trainer, ds


def _val_ms(trainer, ds, reps):
    times = []
    for _ in range(reps + 1):                                  # the first one warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            trainer.val(0, ds)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times[1:])), [round(t, 1) for t in times]


def main():
    a = ARGS
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    D, H, W = (int(v) for v in a.shape.split("x"))
    rng = np.random.RandomState(0)
    vol = torch.from_numpy((rng.standard_normal((D, H, W)) * 30 + 10).astype(np.float32)).cuda()
    coords = np.stack([rng.randint(40, W - 40, 400), rng.randint(40, H - 40, 400), rng.randint(4, D - 4, 400)], 1)
    work = tempfile.mkdtemp(prefix="bench_debug_vis_")
    opt, trainer, ds = _trainer_and_sample(vol, coords, work)
    out = {"device": torch.cuda.get_device_name(0), "tomogram": [D, H, W], "val_reps": a.val_reps}
    out["val_debug0_ms"], out["val_debug0_ms_all"] = _val_ms(trainer, ds, a.val_reps)
    if a.val_only:
        print(json.dumps(out))
        shutil.rmtree(work, ignore_errors=True)
        return

    from cet_pick_amd.build import source_sha16
    from cet_pick_amd.utils import debug_vis as V
    batch = next(iter(ds))
    tomo, hm_gt = batch["input"][0], batch["hm"][0, 0]
    d, hh, ww = tomo.shape
    z_lo, z_hi = V.Z_MARGIN, d - V.Z_MARGIN
    nz = z_hi - z_lo
    hm_pred = torch.rand_like(hm_gt)
    gt = np.array(batch["meta"]["gt_det"], dtype=np.float32)
    gt[:, :2] *= 2
    pred = np.concatenate([gt[:200], np.full((min(len(gt), 200), 2), 0.9, np.float32)], 1)
    out.update({"kernels_sha16": source_sha16(["debug_vis"]), "window": [d, hh, ww], "slices": nz, "reps": a.reps,
                "picks": len(pred), "gt_centres": len(gt), "ceilings": {"hbm_tbs": HBM_CEILING / 1e12},
                "predicted": PREDICTED})
    mm = V.slice_minmax(tomo, z_lo, nz)
    dev_out = torch.empty((12 * nz * hh * ww,), dtype=torch.uint8, device=tomo.device)
    out["minmax_us"], out["minmax_us_all"] = _events_us(lambda: V.slice_minmax(tomo, z_lo, nz), a.reps)
    out["render_us"], out["render_us_all"] = _events_us(
        lambda: V.render(tomo, hm_pred, hm_gt, z_lo, nz, pred, gt, minmax=mm, out=dev_out), a.reps)
    px = nz * hh * ww
    out["minmax_bytes"] = 4 * px
    out["render_bytes"] = 4 * px + 2 * 4 * (px // 4) + 12 * px        # the tomogram, two heat-maps, four RGB pictures
    for k in ("minmax", "render"):
        out[k + "_tbs"] = out[k + "_bytes"] / (out[k + "_us"] * 1e-6) / 1e12
        out[k + "_frac_hbm"] = out[k + "_bytes"] / (out[k + "_us"] * 1e-6) / HBM_CEILING
    pinned = torch.empty((dev_out.numel(),), dtype=torch.uint8, pin_memory=True)
    us, _ = _events_us(lambda: pinned.copy_(dev_out, non_blocking=True), max(3, a.reps // 2), warm=1)
    out["copy_ms"], out["copy_bytes"] = us / 1e3, dev_out.numel()
    out["copy_gbs"] = dev_out.numel() / (us * 1e-6) / 1e9
    del pinned, dev_out

    opt.debug = 4
    opt.debug_dir = os.path.join(work, "debug")
    with torch.no_grad():
        trainer.val(0, ds)                                      # warm-up: staging buffers, pool, code objects
    V.encode_stats(reset=True)
    out["val_debug4_ms"], out["val_debug4_ms_all"] = _val_ms(trainer, ds, a.val_reps)
    sec, files = V.encode_stats(reset=True)
    runs = a.val_reps + 1
    out["pool"], out["files"] = V.pool_size(), files // runs
    out["png_bytes"] = sum(os.path.getsize(os.path.join(opt.debug_dir, f)) for f in os.listdir(opt.debug_dir)
                           if f.endswith(".png"))
    out["encode_thread_s"] = sec / runs
    extra = max(out["val_debug4_ms"] - out["val_debug0_ms"], 1e-3)
    out["debug4_extra_ms"] = extra
    out["encode_share"] = min(1.0, out["encode_thread_s"] * 1e3 / out["pool"] / extra)
    parts = {"render": (out["render_us"] + out["minmax_us"]) / 1e3, "copy": out["copy_ms"],
             "encode": out["encode_thread_s"] * 1e3 / out["pool"]}
    out["parts_ms"] = parts
    out["bound"] = max(parts, key=parts.get)
    out["parent_debug0_ms"] = a.parent_debug0_ms
    os.chdir(REPO)
    shutil.rmtree(work, ignore_errors=True)
    path = a.out or os.path.join(REPO, "profiles", "debug_vis_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if not k.endswith("_all")}))


if __name__ == "__main__":
    main()
