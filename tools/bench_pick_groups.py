"""Cost of grouping and tracing the picks (csrc/pick_groups.hip), one JSON line and profiles/pick_groups_bench.json:

    python tools/bench_pick_groups.py [--out profiles/pick_groups_bench.json] [--sizes 900 4096] [--reps 9]

The input is the long case for label propagation: n integer points on a line, 10 apart (only consecutive ones are within the
cutoff of 15), in a shuffled index order - one component of n members whose graph has diameter n - 1.  A record, not a gate:
the work is small, and one workgroup merges the labels.  Per size:
  components_ms    one hipops.pick_components (two launches), points already on the device; HIP events, median after a warm-up
  fiber_fit_ms     one hipops.pick_fiber_fit on its labels (one launch and the entry's wait for the row count); host clock
                   around the call and a device synchronise, median
  host_group_ms    utils.post_process.tomo_group_postprocess on the same points, host clock, median (for information)
  host_fiber_ms    utils.post_process.tomo_fiber_postprocess on the same points
  equal            the device forms return what the host functions return
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


def chain(n, seed=3):
    order = np.random.default_rng(seed).permutation(n)
    pts = np.zeros((n, 3))
    pts[:, 0], pts[:, 1], pts[:, 2] = 10.0 * order, 7.0 + (order % 3 == 0), 3.0 + (order % 2)
    return pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pick_groups_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[900, 4096])
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    from cet_pick_amd import hipops as H
    from cet_pick_amd.build import source_sha16
    from cet_pick_amd.utils import post_process as PP

    r = {"kernels_sha16": source_sha16(["pick_groups"]), "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in a.sizes:
        pts = chain(n)
        d = torch.from_numpy(pts).cuda()
        cap = int((pts[:, 0].max() - pts[:, 0].min()) // 2)
        label, size = H.pick_components(d, 15)
        e = {}
        e["components_ms"], e["components_ms_all"] = _events_ms(lambda: H.pick_components(d, 15), a.reps)
        e["fiber_fit_ms"], e["fiber_fit_ms_all"] = _host_ms(lambda: H.pick_fiber_fit(d, label, size, 30, 0.03, 2, cap), a.reps)
        scored = np.concatenate([pts, np.full((n, 1), 0.5)], 1)
        e["host_group_ms"], _ = _host_ms(lambda: PP.tomo_group_postprocess(scored, 15, 5), 3)
        e["host_fiber_ms"], _ = _host_ms(lambda: PP.tomo_fiber_postprocess(pts, 15, 30, 0.03, 2), 3)
        e["equal"] = bool(np.array_equal(np.array(PP.tomo_group_postprocess_device(scored, 15, 5)),
                                         np.array(PP.tomo_group_postprocess(scored, 15, 5))) and
                          PP.tomo_fiber_postprocess_device(pts, 15, 30, 0.03, 2) == PP.tomo_fiber_postprocess(pts, 15, 30, 0.03, 2))
        r["sizes"][str(n)] = e
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print(json.dumps(r))


if __name__ == "__main__":
    main()
