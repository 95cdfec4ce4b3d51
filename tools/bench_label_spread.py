"""Cost of label spreading (csrc/label_spread.hip), one JSON line and profiles/label_spread_bench.json:

    python tools/bench_label_spread.py [--out profiles/label_spread_bench.json] [--n 1000000] [--d 128] [--k 15] [--c 4]
                                       [--reps 7] [--sweeps 50]

A synthetic blob bank of --n picks in --d dimensions around 64 normal centres (spread 0.15), its graph searched by mi_knn_search,
--c classes seeded on 8 picks each.  A record, not a gate.  HIP events around the launches alone, synchronised, two warm-ups:
  knn_ms            the search (once)
  graph_ms          spread_graph: weights, reverse graph (torch sort), count, scan, fill; median and all of --reps
  sweep_us          mi_spread_step without the residual word, one window = --sweeps ping-pong sweeps, per sweep; median, min, max
  sweep_track_us    the same with the residual word
  spmm_us           the baseline: torch.sparse.mm of the same CSR (int32 indices, float64) with F, nothing else - an independent
                    implementation; windows alternate with sweep_us in one loop
  spmm_axpy_us      the baseline with the alpha / (1 - alpha) Y combination, what a sweep computes in full
  ratio             sweep_us / spmm_us (medians); spread_pct of each = (max - min) / median
  hbm_bytes         per sweep, compulsory: col + val (12 nnz), row_ptr (8 n), Y and F_out (16 n c), F_in once (8 n c); the
                    gathered rows (8 nnz c) are expected from L2 / Infinity Cache (F is 8 n c bytes); hbm_tb_s = hbm_bytes / sweep
  max_rel_diff      the sweep against the baseline's result, elementwise relative
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _window_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(times_ms, per):
    us = np.asarray(times_ms) * 1e3 / per
    med = float(np.median(us))
    return {"median": med, "min": float(us.min()), "max": float(us.max()), "spread_pct": float(100 * (us.max() - us.min()) / med),
            "all": [round(float(t), 3) for t in us]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "label_spread_bench.json"))
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--c", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    from cet_pick_amd import hipops as H
    from cet_pick_amd.build import source_sha16
    from cet_pick_amd.utils import label_spread as LS

    n, d, k, c, alpha = a.n, a.d, a.k, a.c, 0.9
    rs = np.random.RandomState(7)
    blob = rs.randint(0, 64, n)
    x = torch.from_numpy(rs.randn(64, d).astype(np.float32)[blob] + np.float32(0.15) * rs.randn(n, d).astype(np.float32)).cuda()
    r = {"kernels_sha16": source_sha16(["label_spread", "knn_graph"]), "device": torch.cuda.get_device_name(0), "n": n, "d": d, "k": k,
         "c": c, "alpha": alpha, "sweeps_per_window": a.sweeps}
    index = dist = None

    def search():
        nonlocal index, dist
        index, dist = H.knn_search(x, x, k, metric="l2", exclude_self=True)
    r["knn_ms"] = _window_ms(search)
    del x
    graph = [None]

    def build():
        graph[0] = LS.spread_graph(index, dist, "gauss")
    for _ in range(2):
        build()
    r["graph_ms"] = _stats([_window_ms(build) for _ in range(a.reps)], 1e3)
    g = graph[0]
    nnz = int(g.col.shape[0])
    rows = np.diff(g.row_ptr.cpu().numpy())
    r.update(nnz=nnz, longest_row=int(rows.max()), median_row=float(np.median(rows)))
    seeds = rs.choice(n, 8 * c, replace=False)
    y = torch.from_numpy(LS.seed_matrix(n, seeds, np.arange(8 * c) % c, c)).cuda()
    f0, f1 = y.clone(), torch.empty_like(y)
    word = torch.zeros(1, dtype=torch.int64, device="cuda")

    def sweeps(track):
        def run():
            p, q = f0, f1
            for _ in range(a.sweeps):
                H.spread_step(g.row_ptr, g.col, g.val, alpha, p, y, q, word if track else None)
                p, q = q, p
        return run

    s_csr = torch.sparse_csr_tensor(g.row_ptr.to(torch.int32), g.col, g.val, size=(n, n))
    yb = (1.0 - alpha) * y

    def spmm():
        p = f0
        for _ in range(a.sweeps):
            p = torch.sparse.mm(s_csr, p)

    def spmm_axpy():
        p = f0
        for _ in range(a.sweeps):
            p = torch.add(yb, torch.sparse.mm(s_csr, p), alpha=alpha)

    for fn in (sweeps(False), sweeps(True), spmm, spmm_axpy):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {"sweep_us": [], "sweep_track_us": [], "spmm_us": [], "spmm_axpy_us": []}
    for _ in range(a.reps):                                # the four alternate inside one loop
        t["sweep_us"].append(_window_ms(sweeps(False)))
        t["spmm_us"].append(_window_ms(spmm))
        t["sweep_track_us"].append(_window_ms(sweeps(True)))
        t["spmm_axpy_us"].append(_window_ms(spmm_axpy))
    for key, v in t.items():
        r[key] = _stats(v, a.sweeps)
    r["ratio"] = r["sweep_us"]["median"] / r["spmm_us"]["median"]
    r["ratio_full"] = r["sweep_us"]["median"] / r["spmm_axpy_us"]["median"]
    r["hbm_bytes"] = 12 * nnz + 8 * n + 24 * n * c
    r["gathered_bytes"] = 8 * nnz * c
    r["hbm_tb_s"] = r["hbm_bytes"] / (r["sweep_us"]["median"] * 1e-6) / 1e12
    ours = H.spread_step(g.row_ptr, g.col, g.val, alpha, y, y, torch.empty_like(y))
    base = torch.add(yb, torch.sparse.mm(s_csr, y), alpha=alpha)
    r["max_rel_diff"] = float(((ours - base).abs() / base.abs().clamp_min(1e-300)).max())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print(json.dumps(r))


if __name__ == "__main__":
    main()
