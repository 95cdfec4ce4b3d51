"""Cost of the k-means of the exploration embeddings (csrc/kmeans.hip, utils/kmeans.py), one JSON line and
profiles/kmeans_bench.json:

    python tools/bench_kmeans.py [--out profiles/kmeans_bench.json] [--sklearn_iters 3] [--sizes 10000x128x256,...]

Per (N, d, k): HIP events around repeated launches after a warm-up (median)
  assign_us        one mi_kmeans_assign;  assign_frac_bf16x3 = (2 N k d / t) / 416.7 TFLOP/s (the bf16x3 ceiling: 2.5 PFLOP/s / 6)
  update_us        one mi_kmeans_update (six launches);  update_frac_hbm = (N d 4 bytes / t) / 8 TB/s
  prep_us          one mi_kmeans_prep
  iteration_us     one iteration as Kmeans.train enqueues it (a fit of `--iters` iterations / iters, host launches included)
  fit300_ms        a 300-iteration Kmeans.train (xnorm, the loop, the read-back of the objective), wall clock
  sklearn_*        sklearn.cluster.KMeans(init=<same rows>, n_init=1, algorithm='lloyd', tol=0, max_iter=--sklearn_iters) on
                   this host's CPU (threads as the environment sets them), per iteration and scaled to 300
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

BF16X3_CEILING, HBM_CEILING = 416.7e12, 8e12


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
    return float(np.median(times))


def one(N, d, k, iters, sk_iters):
    from cet_pick_amd import hipops as H
    from cet_pick_amd.utils.kmeans import Kmeans
    g = torch.Generator(device="cuda").manual_seed(7)
    mu = torch.nn.functional.normalize(torch.randn(48, d, device="cuda", generator=g), dim=1)
    x = mu[torch.randint(48, (N,), device="cuda", generator=g)] + 0.15 * torch.randn(N, d, device="cuda", generator=g)
    rows = np.random.RandomState(1234).permutation(N)[:k]
    cent = x[torch.from_numpy(rows).cuda()].clone()
    ws = H.kmeans_workspace(N, d, k, x.device)
    image, xnorm = H.kmeans_prep(cent), H.kmeans_xnorm(x)
    labels, dist = H.kmeans_assign(x, xnorm, image, k, ws=ws)
    counts = torch.empty(k, dtype=torch.int32, device="cuda")
    c2 = cent.clone()
    reps = 30 if N <= 100000 else 10
    r = {"N": N, "d": d, "k": k}
    r["prep_us"] = _events_us(lambda: H.kmeans_prep(cent, image), reps)
    r["xnorm_us"] = _events_us(lambda: H.kmeans_xnorm(x, xnorm), reps)
    r["assign_us"] = _events_us(lambda: H.kmeans_assign(x, xnorm, image, k, labels, dist, ws), reps)
    r["update_us"] = _events_us(lambda: H.kmeans_update(x, labels, c2, counts, ws=ws), reps)
    r["assign_tflops"] = 2.0 * N * k * d / (r["assign_us"] * 1e-6) / 1e12
    r["assign_frac_bf16x3"] = r["assign_tflops"] * 1e12 / BF16X3_CEILING
    r["update_gbs"] = N * d * 4.0 / (r["update_us"] * 1e-6) / 1e9
    r["update_frac_hbm"] = r["update_gbs"] * 1e9 / HBM_CEILING

    def fit(n):
        km = Kmeans(d, k, niter=n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        km.train(x)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, km
    fit(3)
    r["iteration_us"] = float(np.median([fit(iters)[0] for _ in range(3)])) / iters * 1e3
    ms, km = fit(300)
    r["fit300_ms"] = ms
    r["objective"] = [float(km.obj[0]), float(km.obj[-1])]
    r["empty_clusters_served"] = km.n_split
    try:
        from sklearn.cluster import KMeans
        xh = x.cpu().numpy()
        t0 = time.perf_counter()
        sk = KMeans(n_clusters=k, init=xh[rows].copy(), n_init=1, algorithm="lloyd", tol=0, max_iter=sk_iters).fit(xh)
        dt = time.perf_counter() - t0
        r["sklearn_iters"] = int(sk.n_iter_)
        r["sklearn_iteration_ms"] = dt / max(int(sk.n_iter_), 1) * 1e3
        r["sklearn_fit300_ms_scaled"] = r["sklearn_iteration_ms"] * 300
        r["sklearn_threads"] = int(os.environ.get("OMP_NUM_THREADS", 0)) or None
    except ImportError:
        r["sklearn_iteration_ms"] = None
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kmeans_bench.json"))
    ap.add_argument("--sizes", default="10000x128x256,100000x128x256,1000000x128x256,1000000x32x256")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sklearn_iters", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    from cet_pick_amd.build import source_sha16
    out = {"kernels_sha16": source_sha16(["kmeans", "rowdot", "bf16x3"]), "device": torch.cuda.get_device_name(0),
           "ceilings": {"bf16x3_tflops": BF16X3_CEILING / 1e12, "hbm_tbs": HBM_CEILING / 1e12}, "sizes": []}
    for s in a.sizes.split(","):
        N, d, k = (int(v) for v in s.split("x"))
        out["sizes"].append(one(N, d, k, a.iters, a.sklearn_iters))
        print(json.dumps(out["sizes"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
