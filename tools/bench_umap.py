"""Cost of the UMAP kernels (csrc/umap.hip), one JSON line and profiles/umap_bench.json:

    python tools/bench_umap.py [--out profiles/umap_bench.json] [--n 100000] [--d 128] [--n_neighbors 40]

N points in d dimensions (48 blobs), the K - 1 = n_neighbors - 1 nearest other points of each, umap-learn's random start; HIP
events, the median of five runs after two warm-ups:
  smooth_knn_ms, union_ms  the two set-up kernels (union: one launch with the spacings)
  epoch_ms                 one mi_umap_epoch, at epochs 1, 100 and 200 of 200 (the firings differ a little from epoch to epoch)
  fit_ms                   the whole 200-epoch fit of utils/umap.UMAP from the graph (set-up, reverse lists, 200 launches, the copy
                           back), a host clock around a synchronise; fit_epochs_ms the 200 launches alone, by events
  firings, terms           incident pairs that fire at epoch 100 (counted by torch from the device's spacings) and the 6 terms each
                           adds; term_rate = terms / epoch_ms; incident = entries of all incident lists
  torch_epoch_ms           the same epoch written in torch on the same device in float64: the firing test over the incident list,
                           gathers, the attraction and 5 negatives per firing (torch.randint, not Philox), index_add_ per vertex
                           (the two forms draw different negatives, so their outputs are not compared here; the kernel is held
                           to float64 term by term in tests/test_umap_gpu.py)
Not measured here: the quality of the map at this N, hardware counters, other N / K.
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

F64_VECTOR_PEAK = 78.6e12
TERMS_PER_FIRING = 6


def _events_ms(fn, reps=5, warm=2):
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


def incident_lists(index, mutual, eps):
    """(vertex, other, eps) of every incident entry, on the device: the forward edges, then the reverse edges without an
    opposite edge (their order does not matter to the torch form)."""
    n, k = index.shape
    src = torch.arange(n, device=index.device).repeat_interleave(k)
    dst = index.reshape(-1).long()
    lone = mutual.reshape(-1) == 0
    e = eps.reshape(-1)
    return torch.cat([src, dst[lone]]), torch.cat([dst, src[lone]]), torch.cat([e, e[lone]])


def torch_epoch(y, vert, other, eps, n, n_epochs, a, b, generator):
    N = y.shape[0]
    Y = y.double()
    fire = torch.floor(n / eps) > torch.floor((n - 1) / eps)
    v, o = vert[fire], other[fire]
    acc = torch.zeros_like(Y)
    diff = Y[v] - Y[o]
    d2 = (diff * diff).sum(1, keepdim=True)
    c = torch.where(d2 > 0, -2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0), torch.zeros_like(d2))
    acc.index_add_(0, v, 2.0 * (c * diff).clamp(-4.0, 4.0))
    neg = torch.randint(N, (len(v), 5), device=y.device, generator=generator)
    diff = Y[v][:, None, :] - Y[neg]
    d2 = (diff * diff).sum(2, keepdim=True)
    t = (2.0 * b / ((0.001 + d2) * (a * d2 ** b + 1.0)) * diff).clamp(-4.0, 4.0)
    t = torch.where(d2 > 0, t, torch.full_like(t, 4.0))
    t = torch.where((neg == v[:, None])[:, :, None], torch.zeros_like(t), t)
    acc.index_add_(0, v, t.sum(1))
    return (Y + (1.0 - (n - 1.0) / n_epochs) * acc).float(), int(fire.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "umap_bench.json"))
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--n_neighbors", type=int, default=40)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    from cet_pick_amd import hipops as H
    from cet_pick_amd.build import source_sha16
    from cet_pick_amd.utils.graph import reverse_graph
    from cet_pick_amd.utils.umap import UMAP, find_ab_params
    N, K = a_.n, a_.n_neighbors
    k = K - 1
    g = torch.Generator(device="cuda").manual_seed(7)
    mu = 4.0 * torch.randn(48, a_.d, device="cuda", generator=g)
    x = mu[torch.randint(48, (N,), device="cuda", generator=g)] + torch.randn(N, a_.d, device="cuda", generator=g)
    um = UMAP(K, min_dist=0.5, seed=42)
    n_epochs = 500 if N <= 10000 else 200
    a, b = find_ab_params(0.5)
    index, dist = um.graph(x)
    index, dist = index[:, :k].contiguous(), dist[:, :k].contiguous()
    mean_all = float(torch.sqrt(dist).sum(dtype=torch.float64).item()) / (N * K)
    w = H.umap_smooth_knn(dist, mean_all)[2]
    rev_ptr, rev_edge = reverse_graph(index)
    out = H.umap_union(index, w, rev_ptr, rev_edge, n_epochs)
    wmax = out[0].max().reshape(1)
    _, mutual, eps = H.umap_union(index, w, rev_ptr, rev_edge, n_epochs, wmax=wmax, out=out)
    y = torch.from_numpy(np.random.RandomState(42).uniform(-10, 10, (N, 2)).astype(np.float32)).cuda()
    y2 = torch.empty_like(y)
    r = {"kernels_sha16": source_sha16(["umap", "knn_graph"]), "device": torch.cuda.get_device_name(0), "N": N, "d": a_.d, "n_neighbors": K,
         "columns": k, "n_epochs": n_epochs, "a": a, "b": b, "f64_vector_peak_tflops": F64_VECTOR_PEAK / 1e12}
    r["smooth_knn_ms"], r["smooth_knn_ms_all"] = _events_ms(lambda: H.umap_smooth_knn(dist, mean_all))
    r["union_ms"], r["union_ms_all"] = _events_ms(lambda: H.umap_union(index, w, rev_ptr, rev_edge, n_epochs, wmax=wmax, out=out))
    for n in (1, 100, n_epochs):
        key = "epoch_ms" if n == 100 else "epoch_%d_ms" % n
        r[key], r[key + "_all"] = _events_ms(lambda: H.umap_epoch(y, y2, index, rev_ptr, rev_edge, mutual, eps, n, n_epochs, a, b, 42))
    vert, other, eps_inc = incident_lists(index, mutual, eps)
    r["incident"] = int(len(vert))
    _, r["firings"] = torch_epoch(y, vert, other, eps_inc, 100, n_epochs, a, b, g)
    r["terms"] = TERMS_PER_FIRING * r["firings"]
    r["term_rate"] = r["terms"] / (r["epoch_ms"] * 1e-3)
    r["torch_epoch_ms"], r["torch_epoch_ms_all"] = _events_ms(lambda: torch_epoch(y, vert, other, eps_inc, 100, n_epochs, a, b, g))
    r["epoch_over_torch"] = r["epoch_ms"] / r["torch_epoch_ms"]

    def epochs():
        p, q = y.clone(), y2
        for n in range(1, n_epochs + 1):
            H.umap_epoch(p, q, index, rev_ptr, rev_edge, mutual, eps, n, n_epochs, a, b, 42)
            p, q = q, p

    r["fit_epochs_ms"], r["fit_epochs_ms_all"] = _events_ms(epochs, reps=3, warm=1)
    fits = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        emb = um.fit_transform(x, graph=(index, dist))
        torch.cuda.synchronize()
        fits.append((time.perf_counter() - t0) * 1e3)
    r["fit_ms"], r["fit_ms_all"] = float(np.median(fits)), [round(t, 3) for t in fits]
    r["fit_finite"], r["fit_extent"] = bool(np.isfinite(emb).all()), [float(v) for v in np.ptp(emb, axis=0)]
    with open(a_.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print(json.dumps(r))


if __name__ == "__main__":
    main()
