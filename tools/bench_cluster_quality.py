"""Cost of the exact silhouette (csrc/cluster_quality.hip), one JSON line and profiles/cluster_quality_bench.json:

    python tools/bench_cluster_quality.py [--out profiles/cluster_quality_bench.json] [--n 200000] [--d 128] [--k 256] [--reps 5]

Two inputs of --n picks in --d dimensions with --k fine clusters: "random" (normal rows, labels drawn uniformly: no structure, even
cluster sizes) and "blobs" (rows around --k normal centres, spread 0.15, the label the blob; cluster sizes drawn from a
Dirichlet(1) so they are uneven).  A record, not a gate.  Per input, HIP events around the launches alone, median of --reps after
two warm-ups, synchronised:
  sums_ms           mi_silhouette_sums (count, scan, prep, pairs, sum: the one pass over the n x n pairs); the stable sort of the
                    labels that the wrapper does with torch is outside it (sort_ms)
  score_ms          one SilhouetteSums.score (mi_silhouette_finalise on the kept sums, a merge into 16 classes, its results
                    brought to the host), host clock
  mfma_flop         6 x 2 x n^2 x d: the bf16x3 matrix-core work the pass stands for; mfma_tflops = mfma_flop / sums_ms
  workspace_mib, sums_mib
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


def _host_ms(fn, reps, warm=2):
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


def inputs(kind, n, d, k, seed=7):
    rs = np.random.RandomState(seed)
    if kind == "random":
        return rs.randn(n, d).astype(np.float32), rs.randint(0, k, n).astype(np.int32)
    labels = rs.choice(k, n, p=rs.dirichlet(np.ones(k))).astype(np.int32)
    return (rs.randn(k, d).astype(np.float32)[labels] + np.float32(0.15) * rs.randn(n, d).astype(np.float32)), labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cluster_quality_bench.json"))
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    from cet_pick_amd import _lib as L
    from cet_pick_amd.build import source_sha16
    from cet_pick_amd.utils.cluster_quality import SilhouetteSums

    n, d, k = a.n, a.d, a.k
    r = {"kernels_sha16": source_sha16(["cluster_quality", "rowdot", "bf16x3"]), "device": torch.cuda.get_device_name(0), "n": n, "d": d,
         "k": k, "mfma_flop": 6 * 2 * n * n * d, "inputs": {}}
    nbytes = L.lib().mi_silhouette_workspace_bytes(n, d, k)
    assert nbytes > 0
    r["workspace_mib"], r["sums_mib"] = nbytes / 2 ** 20, n * k * 8 / 2 ** 20
    class_of = (np.arange(k) % 16).astype(np.int32)
    for kind in ("random", "blobs"):
        x, labels = inputs(kind, n, d, k)
        xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
        e = {"largest_cluster": int(np.bincount(labels, minlength=k).max()), "smallest_cluster": int(np.bincount(labels, minlength=k).min())}
        e["sort_ms"], _ = _events_ms(lambda: torch.sort(ld, stable=True)[1].to(torch.int32), a.reps)
        order = torch.sort(ld, stable=True)[1].to(torch.int32)
        sums = torch.empty((n, k), dtype=torch.float64, device="cuda")
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        e["sums_ms"], e["sums_ms_all"] = _events_ms(lambda: L.call("mi_silhouette_sums", xd, ld, order, n, d, k, sums, ws, ws.numel()), a.reps)
        e["mfma_tflops"] = r["mfma_flop"] / (e["sums_ms"] * 1e-3) / 1e12
        del sums, ws
        kept = SilhouetteSums(xd, ld, k)
        e["score_ms"], e["score_ms_all"] = _host_ms(lambda: kept.score(class_of), a.reps)
        e["mean_silhouette_16"] = kept.score(class_of).mean
        del kept
        r["inputs"][kind] = e
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print(json.dumps(r))


if __name__ == "__main__":
    main()
