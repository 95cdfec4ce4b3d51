"""Cost of the exact k-nearest-neighbour search (csrc/knn.hip, hipops.knn_search), one JSON line and profiles/knn_bench.json:

    python tools/bench_knn.py [--out profiles/knn_bench.json] [--sizes 100000x128x16,...] [--metric l2] [--chunk 8192]

Per size N x d x k, one self-search (queries = database, exclude_self), HIP events, median after a warm-up:
  knn_ms           one hipops.knn_search (the cut of the database, the fused product + selection, the merge; the workspace
                   allocation included);  knn_tflops = 2 N N d / t, the f32-equivalent rate;  knn_frac_bf16x3 of the 416.7 TFLOP/s
                   bf16x3 ceiling (2.5 PFLOP/s / 6)
  torch_ms         the same result from torch on the same device: per chunk of --chunk queries a matmul against the whole
                   database (fp32), the diagonal masked, torch.topk;  torch_tflops likewise
  assign_k1024_ms  for scale: one mi_kmeans_assign of the same N x d points against 1024 centroids (the same product with a
                   best-of-1024 selection);  assign_k1024_tflops = 2 N 1024 d / t
  index_agreement  share of the (row, rank) pairs on which the two results name the same row (they differ on near-ties and
                   where torch's fp32 matmul and bf16x3 round differently)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BF16X3_CEILING = 416.7e12


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


def torch_knn(x, k, metric, chunk):
    """The chunked matmul + topk baseline: (index (N, k) int64, value (N, k))."""
    n = x.shape[0]
    xn = (x * x).sum(1)
    index = torch.empty(n, k, dtype=torch.int64, device=x.device)
    value = torch.empty(n, k, dtype=torch.float32, device=x.device)
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        sim = x[s:e] @ x.t()
        if metric == "l2":
            sim = xn[s:e, None] + (xn[None, :] - 2.0 * sim)
        rows = torch.arange(e - s, device=x.device)
        sim[rows, rows + s] = float("inf") if metric == "l2" else float("-inf")
        v, i = sim.topk(k, dim=1, largest=metric == "ip", sorted=True)
        index[s:e], value[s:e] = i, v.clamp_(min=0) if metric == "l2" else v
    return index, value


def one(N, d, k, metric, chunk, reps):
    from cet_pick_amd import hipops as H
    g = torch.Generator(device="cuda").manual_seed(7)
    mu = torch.nn.functional.normalize(torch.randn(48, d, device="cuda", generator=g), dim=1)
    x = mu[torch.randint(48, (N,), device="cuda", generator=g)] + 0.15 * torch.randn(N, d, device="cuda", generator=g)
    r = {"N": N, "d": d, "k": k, "metric": metric, "exclude_self": True, "torch_chunk": chunk}
    r["knn_ms"], r["knn_ms_all"] = _events_ms(lambda: H.knn_search(x, x, k, metric=metric, exclude_self=True), reps)
    r["torch_ms"], r["torch_ms_all"] = _events_ms(lambda: torch_knn(x, k, metric, chunk), reps)
    flop = 2.0 * N * N * d
    r["knn_tflops"] = flop / (r["knn_ms"] * 1e-3) / 1e12
    r["knn_frac_bf16x3"] = r["knn_tflops"] * 1e12 / BF16X3_CEILING
    r["torch_tflops"] = flop / (r["torch_ms"] * 1e-3) / 1e12
    r["knn_over_torch"] = r["knn_ms"] / r["torch_ms"]
    r["image_bytes"] = int(H.L.lib().mi_knn_image_bytes(N, d))
    r["workspace_bytes"] = int(H.L.lib().mi_knn_workspace_bytes(N, N, d, k, 1, 0))
    gi, _ = H.knn_search(x, x, k, metric=metric, exclude_self=True)
    ti, _ = torch_knn(x, k, metric, chunk)
    r["index_agreement"] = float((gi.long() == ti).float().mean())
    cent = x[torch.from_numpy(np.random.RandomState(1234).permutation(N)[:1024]).cuda()].clone()
    ws = H.kmeans_workspace(N, d, 1024, x.device)
    image, xnorm = H.kmeans_prep(cent), H.kmeans_xnorm(x)
    labels, dist = H.kmeans_assign(x, xnorm, image, 1024, ws=ws)
    r["assign_k1024_ms"], _ = _events_ms(lambda: H.kmeans_assign(x, xnorm, image, 1024, labels, dist, ws), reps)
    r["assign_k1024_tflops"] = 2.0 * N * 1024 * d / (r["assign_k1024_ms"] * 1e-3) / 1e12
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "knn_bench.json"))
    ap.add_argument("--sizes", default="100000x128x16", help="N x d x k, comma separated")
    ap.add_argument("--metric", default="l2", choices=["ip", "l2"])
    ap.add_argument("--chunk", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    from cet_pick_amd.build import source_sha16
    out = {"kernels_sha16": source_sha16(["knn", "rowdot", "bf16x3"]), "device": torch.cuda.get_device_name(0),
           "ceilings": {"bf16x3_tflops": BF16X3_CEILING / 1e12}, "sizes": []}
    for s in a.sizes.split(","):
        N, d, k = (int(v) for v in s.split("x"))
        out["sizes"].append(one(N, d, k, a.metric, a.chunk, a.reps))
        print(json.dumps(out["sizes"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
