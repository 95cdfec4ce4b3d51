"""Cost of the exact t-SNE kernels (csrc/tsne.hip), one JSON line and profiles/tsne_bench.json:

    python tools/bench_tsne.py [--out profiles/tsne_bench.json] [--n 100000] [--perplexity 30] [--chunk 8192]

N points in 32 dimensions (48 blobs), K = 3 perplexity + 1 neighbours, an embedding of N(0, 10^2) points; HIP events, the
median of five runs after two warm-ups:
  gradient_ms          one mi_tsne_gradient without the divergence (repulsion, merge, finish)
  gradient_kl_ms       the same with the divergence (every 50th iteration of the descent)
  iteration_ms         one mi_tsne_gradient + one mi_tsne_update
  affinities_ms        one mi_tsne_affinities
  repulsion_tflops     13 N^2 / gradient_ms: per pair 2 subtractions, 2 fused multiply-adds for 1 + |d|^2, the reciprocal, q^2,
                       the sum of q and 2 fused multiply-adds for the force = 13 floating-point operations; pair_rate the
                       pairs per second;  repulsion_frac_f32_peak of the 157.3 TFLOP/s fp32 vector peak (the attraction's
                       2 N K edges ride along in gradient_ms)
  torch_repulsion_ms   the same three sums (sum q, sum q^2 dx, sum q^2 dy per point, self excluded) from torch on the same
                       device, in blocks of --chunk rows against all points
  z, torch_z           agreement of the two: Z = the sum of q over i != j from either, z_rel_diff their relative difference
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

F32_VECTOR_PEAK = 157.3e12
FLOP_PER_PAIR = 13


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


def torch_repulsion(y, chunk):
    """(sum q (N,), sum q^2 (y_i - y_j) (N, 2)) over j != i, in blocks of `chunk` rows."""
    n = y.shape[0]
    sq = torch.empty(n, device=y.device)
    f = torch.empty(n, 2, device=y.device)
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        dx = y[s:e, None, 0] - y[None, :, 0]
        dy = y[s:e, None, 1] - y[None, :, 1]
        q = 1.0 / (1.0 + dx * dx + dy * dy)
        rows = torch.arange(e - s, device=y.device)
        q[rows, rows + s] = 0.0
        sq[s:e] = q.sum(1)
        q = q * q
        f[s:e, 0] = (q * dx).sum(1)
        f[s:e, 1] = (q * dy).sum(1)
    return sq, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tsne_bench.json"))
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--perplexity", type=int, default=30)
    ap.add_argument("--chunk", type=int, default=8192)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    from cet_pick_amd import hipops as H
    from cet_pick_amd.build import source_sha16
    from cet_pick_amd.utils.graph import reverse_graph
    from cet_pick_amd.utils.tsne import n_neighbors
    N, P = a.n, a.perplexity
    K = n_neighbors(N, P)
    g = torch.Generator(device="cuda").manual_seed(7)
    mu = 4.0 * torch.randn(48, 32, device="cuda", generator=g)
    x = mu[torch.randint(48, (N,), device="cuda", generator=g)] + torch.randn(N, 32, device="cuda", generator=g)
    y = 10.0 * torch.randn(N, 2, device="cuda", generator=g)
    index, dist = H.knn_search(x, x, K, metric="l2", exclude_self=True)
    p, _ = H.tsne_affinities(dist, P)
    rev_ptr, rev_edge = reverse_graph(index)
    ws = H.tsne_workspace(N, K, 0, x.device)
    grad, z, kl = H.tsne_gradient(y, index, p, rev_ptr, rev_edge, 1.0, ws=ws)
    vel, gains, y2 = torch.zeros_like(y), torch.ones_like(y), y.clone()
    r = {"kernels_sha16": source_sha16(["tsne", "knn_graph"]), "device": torch.cuda.get_device_name(0), "N": N, "perplexity": P, "K": K,
         "torch_chunk": a.chunk, "workspace_bytes": int(ws.numel()), "f32_vector_peak_tflops": F32_VECTOR_PEAK / 1e12,
         "flop_per_pair": FLOP_PER_PAIR}

    def step():
        H.tsne_gradient(y2, index, p, rev_ptr, rev_edge, 1.0, kl=False, out=(grad, z, None), ws=ws)
        H.tsne_update(y2, grad, vel, gains, 0.8, 200.0)

    r["gradient_ms"], r["gradient_ms_all"] = _events_ms(
        lambda: H.tsne_gradient(y, index, p, rev_ptr, rev_edge, 1.0, kl=False, out=(grad, z, None), ws=ws))
    r["gradient_kl_ms"], _ = _events_ms(lambda: H.tsne_gradient(y, index, p, rev_ptr, rev_edge, 1.0, out=(grad, z, kl), ws=ws))
    r["iteration_ms"], r["iteration_ms_all"] = _events_ms(step)
    r["affinities_ms"], r["affinities_ms_all"] = _events_ms(lambda: H.tsne_affinities(dist, P))
    r["torch_repulsion_ms"], r["torch_repulsion_ms_all"] = _events_ms(lambda: torch_repulsion(y, a.chunk))
    r["pair_rate"] = float(N) * N / (r["gradient_ms"] * 1e-3)
    r["repulsion_tflops"] = FLOP_PER_PAIR * r["pair_rate"] / 1e12
    r["repulsion_frac_f32_peak"] = r["repulsion_tflops"] * 1e12 / F32_VECTOR_PEAK
    r["gradient_over_torch"] = r["gradient_ms"] / r["torch_repulsion_ms"]
    # the two agree: sum q per point from the library's partials (its Z) against torch's
    H.tsne_gradient(y, index, p, rev_ptr, rev_edge, 1.0, kl=False, out=(grad, z, None), ws=ws)
    sq, _ = torch_repulsion(y, a.chunk)
    r["z"], r["torch_z"] = float(z.item()), float(sq.double().sum().item())
    r["z_rel_diff"] = abs(r["z"] - r["torch_z"]) / r["torch_z"]
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print(json.dumps(r))


if __name__ == "__main__":
    main()
