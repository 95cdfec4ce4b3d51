"""Cost of the pick-to-target matching (csrc/match.hip, hipops.match_coordinates), one JSON line and profiles/match_bench.json:

    python tools/bench_match.py [--out profiles/match_bench.json] [--images 16] [--picks 900] [--targets 600] [--radius 10]

A made-up test split: per image `--targets` integer centres in a 512 x 512 x 128 box; min(5/6 of the picks, the targets)
picks are a jittered centre each and the rest false positives anywhere in the box.  A record, not a gate: one workgroup
solves one image serially, so a single small image may well lose to the host.
  batch_ms         one hipops.match_coordinates over all images (the offset copies, ONE launch), coordinates already on the
                   device; HIP events, median after a warm-up
  single_ms        the same call on the first image alone
  scipy_ms         scipy.optimize.linear_sum_assignment over the same images' dense float64 matrices, one after the other, on
                   the host (the matrices built outside the timed region); host clock, median
  scipy_build_ms   building those matrices with numpy, which the reference also pays
  cost_equal       the device's total costs equal scipy's (integer costs: exactly)
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


def _host_ms(fn, reps):
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), [round(t, 4) for t in times]


def split(n_img, P, T, seed=3):
    rng = np.random.default_rng(seed)
    box = np.array([512, 512, 128])
    images = []
    for _ in range(n_img):
        targets = rng.integers(0, box, (T, 3))
        near = min(P * 5 // 6, T)
        picks = np.concatenate([targets[rng.permutation(T)[:near]] + rng.integers(-4, 5, (near, 3)),
                                rng.integers(0, box, (P - near, 3))])
        images.append((picks[rng.permutation(P)].astype(np.float64), targets.astype(np.float64)))
    return images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "match_bench.json"))
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--picks", type=int, default=900)
    ap.add_argument("--targets", type=int, default=600)
    ap.add_argument("--radius", type=float, default=10)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    from scipy.optimize import linear_sum_assignment
    from cet_pick_amd import hipops as H
    from cet_pick_amd.build import source_sha16

    images = split(a.images, a.picks, a.targets)
    po = np.arange(a.images + 1) * a.picks
    to = np.arange(a.images + 1) * a.targets
    preds = torch.as_tensor(np.concatenate([p for p, _ in images])).cuda()
    targets = torch.as_tensor(np.concatenate([t for _, t in images])).cuda()
    r = {"kernels_sha16": source_sha16(["match"]), "device": torch.cuda.get_device_name(0), "images": a.images,
         "picks": a.picks, "targets": a.targets, "radius": a.radius}
    r["batch_ms"], r["batch_ms_all"] = _events_ms(lambda: H.match_coordinates(preds, targets, po, to, a.radius), a.reps)
    r["single_ms"], r["single_ms_all"] = _events_ms(
        lambda: H.match_coordinates(preds[:a.picks], targets[:a.targets], po[:2], to[:2], a.radius), a.reps)

    def build():
        return [np.minimum(np.sum((p[:, None] - t[None]) ** 2, 2) - a.radius ** 3, 0) for p, t in images]
    costs = build()
    r["scipy_build_ms"], _ = _host_ms(build, 3)
    r["scipy_ms"], r["scipy_ms_all"] = _host_ms(lambda: [linear_sum_assignment(c) for c in costs], a.reps)
    r["scipy_single_ms"], _ = _host_ms(lambda: linear_sum_assignment(costs[0]), a.reps)
    want = [float(c[linear_sum_assignment(c)].sum()) for c in costs]
    p2t, _, total = H.match_coordinates(preds, targets, po, to, a.radius)
    r["cost_equal"] = bool(np.array_equal(total.cpu().numpy(), np.array(want)))
    r["matched_per_image"] = float((p2t >= 0).sum().item()) / a.images
    r["batch_over_scipy"] = r["batch_ms"] / r["scipy_ms"]
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print(json.dumps(r))


if __name__ == "__main__":
    main()
