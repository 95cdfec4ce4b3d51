"""Cost of the pose-pooled MoCo-3D exploration inference (cet_pick_amd/moco_test_3d.py `embed_picks`, csrc/crop_pose.hip), one
JSON line and profiles/moco_infer_bench.json:

    python tools/bench_moco_infer.py [--out profiles/moco_infer_bench.json] [--picks 1024] [--bbox 32] [--reps 5]

The input is a synthetic (64, 256, 256) tomogram, `--picks` seeded centres with a whole box inside it, and a moco3d_18 encoder
with seeded weights in eval mode.  A record, not a gate.  Per --tta in (1, 8):
  embed_ms          one embed_picks over all picks (crops, forward_test, pooling; nothing goes to the host), host clock around
                    the call and a device synchronise, median after a warm-up
  us_per_pick       embed_ms / picks
  batch_picks       picks per batch (moco_test_3d.picks_per_batch: the stem's output stays within 512 MiB)
  crop_ms, pool_ms  the batch's mi_crop_znorm_poses and mi_embed_pool launches alone, HIP events, median
  new_kernels_share (crop_ms + pool_ms) x batches / embed_ms
  crop_gbs          bytes the crop launch must move (the window read once, P crops written) over crop_ms
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


def _events_ms(fn, reps, warm=2):
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
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), [round(t, 4) for t in times]


def _host_ms(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), [round(t, 4) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "moco_infer_bench.json"))
    ap.add_argument("--picks", type=int, default=1024)
    ap.add_argument("--bbox", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    from cet_pick_amd import hipops as H
    from cet_pick_amd import moco_test_3d as M
    from cet_pick_amd.build import source_sha16
    from cet_pick_amd.datasets import subvols as S
    from cet_pick_amd.models.model import create_model
    from cet_pick_amd.synthetic import make_tomo, seeded_state_dict

    shape, s = (64, 256, 256), a.bbox
    vol, _ = make_tomo(shape, seed=317)
    rec = torch.as_tensor(vol).cuda()
    rng = np.random.default_rng(5)
    bd = s // 2 + 1
    cen = np.stack([rng.integers(bd, shape[2] - bd, a.picks), rng.integers(bd, shape[1] - bd, a.picks),
                    rng.integers(bd, shape[0] - bd, a.picks)], 1).astype(np.int32)
    enc = create_model("moco3d_18", {"proj": 256, "pred": 256}, -1)
    enc.load_state_dict(seeded_state_dict(enc, seed=317))
    enc = enc.cuda().eval()
    r = {"kernels_sha16": source_sha16(["crop_pose"]), "device": torch.cuda.get_device_name(0), "picks": a.picks, "bbox": s,
         "tta": {}}
    with torch.no_grad():
        for tta in (1, 8):
            poses = M.pose_set(tta)
            p = len(poses)
            b = min(M.picks_per_batch(s, p), a.picks)
            e = {"batch_picks": b}
            e["embed_ms"], e["embed_ms_all"] = _host_ms(lambda: M.embed_picks(enc, rec, cen, s, tta=tta), a.reps)
            e["us_per_pick"] = 1e3 * e["embed_ms"] / a.picks
            table = S.CropTable([rec], np.zeros(a.picks, np.int32), cen)
            out = torch.empty((b, p, 1, s, s, s), device="cuda")
            e["crop_ms"], _ = _events_ms(lambda: table.cut_poses(0, b, (s, s, s), poses, out=out), a.reps)
            z = torch.randn(b, p, 128, device="cuda")
            pooled = torch.empty(b, 128, device="cuda")
            e["pool_ms"], _ = _events_ms(lambda: H.embed_pool(z, out=pooled), a.reps)
            batches = -(-a.picks // b)
            e["new_kernels_share"] = (e["crop_ms"] + e["pool_ms"]) * batches / e["embed_ms"]
            e["crop_gbs"] = b * (1 + p) * s ** 3 * 4 / (e["crop_ms"] * 1e-3) / 1e9
            r["tta"][str(tta)] = e
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print(json.dumps(r))


if __name__ == "__main__":
    main()
