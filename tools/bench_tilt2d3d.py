"""The 2d3d tilt-patch kernel (csrc/tilt_patch.hip) and the 2d3d dataset build, one JSON line:

    python tools/bench_tilt2d3d.py [--picks 8192] [--bbox 36] [--iters 20]

  kernel_ms       one mi_tilt_patches launch: picks x 5 variants x 13 tilts of a 1024^2 stack (median of --iters, events)
  gather_gbs      the gathered bytes (n * T * bbox^2 * 4 + the n * bbox^2 * 4 written) over kernel_ms
  dataset_build_s the train split of ArraySimSiam2D3DDataset on a synthetic (48, 384, 384) tomogram and its 41-tilt series
                  (DoG picks, both patch launches, compaction, statistics, normalisation), after one warm-up build
  cpu_ms_per_pick the numpy restatement of the reference loop (tests/test_oracle_tilt2d3d.py) on --cpu_picks picks x 5
                  variants of the same stack; cpu_s_all_picks scales it to --picks
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SHIFTS = np.array([(0, 0, 0), (0, 0, 1), (0, 0, -1), (-1, 0, -1), (0, 1, -1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--picks", type=int, default=8192)
    ap.add_argument("--bbox", type=int, default=36)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu_picks", type=int, default=128)
    a = ap.parse_args()
    from cet_pick_amd.datasets import subvols as S
    from cet_pick_amd.datasets.simsiam2d3d import ArraySimSiam2D3DDataset
    from cet_pick_amd.synthetic import make_tilt_series, make_tomo
    from test_oracle_tilt2d3d import ref_extract_patches

    T, H, W, Z, b = 13, 1024, 1024, 256, a.bbox
    rng = np.random.default_rng(5)
    tilts_h = rng.random((T, H, W), dtype=np.float32)
    angles = np.linspace(-18, 18, T)
    picks = np.stack([rng.integers(b, W - b, a.picks), rng.integers(b, H - b, a.picks), rng.integers(10, Z - 10, a.picks)], 1)
    cents = (picks[:, None, :] + SHIFTS[None]).reshape(-1, 3).astype(np.int32)
    stacks = S.TiltStacks([(torch.as_tensor(tilts_h).cuda(), angles, Z)])
    c_dev = torch.as_tensor(cents).cuda()
    for _ in range(3):
        p, v = stacks.patches(c_dev, b, b)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        stacks.patches(c_dev, b, b)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    kernel_ms = float(np.median(times))
    n = len(cents)
    gathered = n * T * b * b * 4 + n * b * b * 4

    # CPU: the reference's loop, restated in numpy, on a subset
    sub = cents[:a.cpu_picks * len(SHIFTS)]
    t0 = time.perf_counter()
    for c in sub:
        ref_extract_patches(tilts_h, c, angles, [W, H, Z], b)
    cpu_ms_per_pick = (time.perf_counter() - t0) * 1e3 / a.cpu_picks
    # bit-level spot check of the timed launch against the restatement
    p_h, v_h = p.cpu().numpy(), v.cpu().numpy()
    mismatch = 0
    for i in range(0, len(sub), 7):
        r = ref_extract_patches(tilts_h, sub[i], angles, [W, H, Z], b)
        mismatch += int((r is not None) != bool(v_h[i]) or (r is not None and np.abs(r - p_h[i, 0]).max() > 2e-6))

    # dataset build
    vol, _ = make_tomo((48, 384, 384), seed=9, margin_xy=40, margin_z=12)
    ang41 = np.arange(-60, 61, 3).astype(np.float64)
    items = [("bench", make_tilt_series(vol, ang41), vol, ang41)]
    opt = type("O", (), {"compress": False, "batch_size": 8, "seed": 1})()
    ArraySimSiam2D3DDataset(opt, "train", (3, b, b), items)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = ArraySimSiam2D3DDataset(opt, "train", (3, b, b), items)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    print(json.dumps({"metric": "tilt2d3d", "picks": a.picks, "variants": len(SHIFTS), "tilts": T, "stack": [H, W], "bbox": b,
                      "kernel_ms": round(kernel_ms, 4), "gather_gbs": round(gathered / kernel_ms / 1e6, 1),
                      "valid_fraction": round(float(v_h.mean()), 4), "spot_check_mismatches": mismatch,
                      "dataset_build_s": round(build_s, 4), "dataset_samples": ds.num_samples,
                      "cpu_ms_per_pick": round(cpu_ms_per_pick, 3),
                      "cpu_s_all_picks": round(cpu_ms_per_pick * a.picks / 1e3, 2)}))


if __name__ == "__main__":
    main()
