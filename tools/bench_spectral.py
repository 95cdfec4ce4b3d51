"""Cost of the spectral start (csrc/spectral.hip, utils/spectral.py), one JSON line and profiles/spectral_bench.json:

    python tools/bench_spectral.py [--out profiles/spectral_bench.json] [--n 100000] [--d 128] [--n_neighbors 40] [--eigsh]

bench_umap.py's data and graph (N points in d dimensions in 48 blobs, the K - 1 nearest other points of each).  HIP events, the
median of five runs after two warm-ups:
  incident                 entries of all incident lists (forward edges and lone reverse edges with a finite spacing)
  components_ms, sweeps    the whole labelling (every sweep's launch and the flag read between them), and its sweeps
  degree_ms, spmv_ms       one mi_spectral_degree, one mi_spectral_spmv over all rows; spmv_stream_gbs = incident x 20 bytes (index or
                           reverse id, wsym, eps, and 4 for the reverse lists' skipped entries) / spmv_ms
  orth_ms                  one mi_spectral_orth at a basis of 316 vectors of length N; orth_gbs = 2 x 316 x N x 8 bytes / orth_ms
  start_ms, steps,         the whole spectral_layout to tol 1e-6 (components, renumbering, Lanczos, placement), a host clock around a
  restarts, converged      synchronise, the median of three; its Lanczos steps and restarts
  fit_spectral_ms,         the whole fit of utils/umap.UMAP from the graph with init="spectral" and with init="random", host clock,
  fit_random_ms            the median of three
  eigsh_s (--eigsh only)   on the host CPU, the call umap-learn makes on the same L: scipy.sparse.linalg.eigsh(L, 3, which="SM",
                           ncv=316, tol=1e-4, v0=ones, maxiter=5 N).  Recorded as what it is; no ratio is asked of it.
Not measured here: hardware counters, other N / K, the quality of the map at this N.
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
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_umap import _events_ms  # noqa: E402


def _host_ms(fn, reps=3):
    times, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), [round(t, 3) for t in times], out


def host_eigsh(index, wsym, eps, n):
    import scipy.sparse as sp
    from scipy.sparse.linalg import eigsh
    k = index.shape[1]
    live = np.isfinite(eps.reshape(-1))
    i, j, w = np.repeat(np.arange(n), k)[live], index.reshape(-1)[live], wsym.reshape(-1)[live].astype(np.float64)
    W = sp.coo_matrix((w, (i, j)), shape=(n, n)).tocsr()
    W = W.maximum(W.T)
    dis = 1.0 / np.sqrt(np.asarray(W.sum(1)).ravel())
    Lm = sp.identity(n) - sp.diags(dis) @ W @ sp.diags(dis)
    t0 = time.perf_counter()
    lam = eigsh(Lm, 3, which="SM", ncv=316, tol=1e-4, v0=np.ones(n), maxiter=5 * n)[0]
    return time.perf_counter() - t0, np.sort(lam).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spectral_bench.json"))
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--n_neighbors", type=int, default=40)
    ap.add_argument("--eigsh", action="store_true")
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    from cet_pick_amd import hipops as H
    from cet_pick_amd.build import source_sha16
    from cet_pick_amd.utils.spectral import spectral_layout
    from cet_pick_amd.utils.umap import UMAP
    N, K = a_.n, a_.n_neighbors
    k = K - 1
    gen = torch.Generator(device="cuda").manual_seed(7)
    mu = 4.0 * torch.randn(48, a_.d, device="cuda", generator=gen)
    x = mu[torch.randint(48, (N,), device="cuda", generator=gen)] + torch.randn(N, a_.d, device="cuda", generator=gen)
    um = UMAP(K, min_dist=0.5, seed=42)
    n_epochs = 500 if N <= 10000 else 200
    index, dist = um.graph(x)
    index, dist = index[:, :k].contiguous(), dist[:, :k].contiguous()
    rev_ptr, rev_edge, mutual, eps, wsym = um.setup(index, dist, n_epochs, with_wsym=True)
    g = (index, wsym, eps, mutual, rev_ptr, rev_edge)
    live = torch.isfinite(eps)
    r = {"kernels_sha16": source_sha16(["spectral", "knn_graph"]), "device": torch.cuda.get_device_name(0), "N": N, "d": a_.d, "n_neighbors": K,
         "columns": k, "n_epochs": n_epochs, "incident": int(live.sum()) + int((live & (mutual == 0)).sum())}
    r["components_ms"], r["components_ms_all"] = _events_ms(lambda: H.graph_components(index, eps, mutual, rev_ptr, rev_edge))
    label, r["sweeps"] = H.graph_components(index, eps, mutual, rev_ptr, rev_edge)
    r["n_components"] = int(torch.unique(label).numel())
    deg, dis = H.spectral_degree(*g)
    r["degree_ms"], r["degree_ms_all"] = _events_ms(lambda: H.spectral_degree(*g))
    v = torch.randn(N, dtype=torch.float64, device="cuda", generator=gen)
    y = torch.empty_like(v)
    r["spmv_ms"], r["spmv_ms_all"] = _events_ms(lambda: H.spectral_spmv(*g, dis, v, y))
    r["spmv_stream_gbs"] = r["incident"] * 20 / (r["spmv_ms"] * 1e-3) / 1e9
    m = 316
    Q = torch.randn(m, N, dtype=torch.float64, device="cuda", generator=gen) / np.sqrt(N)
    c = torch.empty(m, dtype=torch.float64, device="cuda")
    r["orth_basis"] = m
    r["orth_ms"], r["orth_ms_all"] = _events_ms(lambda: H.spectral_orth(Q, y, c))
    r["orth_gbs"] = 2.0 * m * N * 8 / (r["orth_ms"] * 1e-3) / 1e9
    del Q
    r["start_ms"], r["start_ms_all"], (Y, info) = _host_ms(lambda: spectral_layout(*g, dim=2, seed=42, tol=1e-6, x=x))
    r.update(steps=info["steps"], restarts=info["restarts"], converged=info["converged"], basis=info["basis"],
             eigenvalues=None if info["eigenvalues"] is None else [float(e) for e in info["eigenvalues"]],
             residuals=None if info["residuals"] is None else [float(e) for e in info["residuals"]])
    for init in ("spectral", "random"):
        fit = UMAP(K, min_dist=0.5, seed=42, init=init)
        r["fit_%s_ms" % init], r["fit_%s_ms_all" % init], emb = _host_ms(lambda: fit.fit_transform(x, graph=(index, dist)))
        r["fit_%s_init_used" % init], r["fit_%s_finite" % init] = fit.init_, bool(np.isfinite(emb).all())
    if a_.eigsh:
        r["eigsh_s"], r["eigsh_lam"] = host_eigsh(index.cpu().numpy(), wsym.cpu().numpy(), eps.cpu().numpy(), N)
    with open(a_.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print(json.dumps(r))


if __name__ == "__main__":
    main()
