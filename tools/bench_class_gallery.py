"""Cost of the class gallery (csrc/class_gallery.hip), one JSON line and profiles/class_gallery_bench.json:

    python tools/bench_class_gallery.py [--out profiles/class_gallery_bench.json] [--sizes 10000 100000] [--reps 9]

n picks of 36 x 36 patches in 48 classes of uneven size, 128-dimensional embeddings on 256 centroids, 8 exemplars per class: what
plot_2d --class_gallery runs on an exploration of that size.  A record, not a gate.  Per size, inputs already on the device:
  moments_ms       one hipops.gallery_moments (counting sort, two passes of partial sums: 7 launches); HIP events, median
  exemplars_ms     one hipops.gallery_exemplars (counting sort, one selection launch); HIP events, median.  Both wrappers first
                   look at the labels on a host copy, which is part of the call and of this time
  raster_ms        one hipops.gallery_raster (4 launches); HIP events, median
  host_*_ms        the float64 numpy restatements of tests/gallery_ref.py on the same inputs, host clock (for information: they
                   are written to be read, not to be fast)
  moments_gb_s     the bytes the two passes must read (2 n h w 4) over moments_ms
  within_bounds / equal   the device results against the restatements: the bounds of tests/test_class_gallery_gpu.py for the
                   moments, equality for the exemplars and the picture
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
sys.path.insert(0, os.path.join(REPO, "tests"))


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
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), out


def inputs(n, seed=7, h=36, w=36, k=48, kc=256, dim=128):
    rs = np.random.RandomState(seed)
    share = rs.dirichlet(np.full(k, 2.0))                   # uneven classes, none of them empty by design
    labels = rs.choice(k, n, p=share).astype(np.int32)
    assign = (labels + k * rs.randint(0, kc // k, n)).astype(np.int32)      # a class is the union of kc / k centroids
    centroids = (rs.standard_normal((kc, dim)) * 4).astype(np.float32)
    emb = centroids[assign] + rs.standard_normal((n, dim)).astype(np.float32)
    patches = rs.standard_normal((n, h, w)).astype(np.float32)
    patches *= (0.5 + labels % 5)[:, None, None].astype(np.float32)
    patches += (labels % 7)[:, None, None].astype(np.float32)
    return patches, labels, emb.astype(np.float32), centroids, assign, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "class_gallery_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--m", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    import gallery_ref as R
    from cet_pick_amd import hipops as H
    from cet_pick_amd.build import source_sha16
    from cet_pick_amd.utils.plot2d import DIGITS_5X7

    r = {"kernels_sha16": source_sha16(["class_gallery"]), "device": torch.cuda.get_device_name(0), "m": a.m, "sizes": {}}
    glyphs = torch.from_numpy(DIGITS_5X7).cuda()
    for n in a.sizes:
        patches, labels, emb, centroids, assign, k = inputs(n)
        x, lab, e_, c_, a_ = (torch.from_numpy(v).cuda() for v in (patches, labels, emb, centroids, assign))
        e = {"classes": k, "patch": list(patches.shape[1:]), "dim": emb.shape[1], "largest_class": int(np.bincount(labels).max())}
        mean, std, count = H.gallery_moments(x, lab, k)
        idx, d2 = H.gallery_exemplars(e_, c_, a_, lab, k, a.m)
        pic, order = H.gallery_raster(mean, std, count, idx, x, glyphs)
        e["moments_ms"], e["moments_ms_all"] = _events_ms(lambda: H.gallery_moments(x, lab, k), a.reps)
        e["exemplars_ms"], e["exemplars_ms_all"] = _events_ms(lambda: H.gallery_exemplars(e_, c_, a_, lab, k, a.m), a.reps)
        e["raster_ms"], e["raster_ms_all"] = _events_ms(lambda: H.gallery_raster(mean, std, count, idx, x, glyphs), a.reps)
        e["moments_gb_s"] = 2 * patches.nbytes / (e["moments_ms"] * 1e-3) / 1e9
        e["picture"] = list(pic.shape)
        host_reps = 3 if n <= 20000 else 1
        e["host_moments_ms"], (w_mean, w_std, w_count) = _host_ms(lambda: R.moments(patches, labels, k), host_reps)
        e["host_exemplars_ms"], (w_idx, w_d2) = _host_ms(lambda: R.exemplars(emb, centroids, assign, labels, k, a.m), host_reps)
        mean_h, std_h, count_h, idx_h = (t.cpu().numpy() for t in (mean, std, count, idx))
        e["host_raster_ms"], w_pic = _host_ms(lambda: R.raster(mean_h, std_h, count_h, idx_h, patches, a.m, 2), host_reps)
        top = float(np.abs(patches).max())
        e["mean_error_over_bound"] = float(np.abs(mean_h - w_mean).max() / (2.0 ** -23 * top))
        e["std_error_over_bound"] = float((np.abs(std_h - w_std) / (2.0 ** -24 * w_std + 2.0 ** -40 * (w_std + top) + 2.0 ** -149)).max())
        e["within_bounds"] = bool(np.array_equal(count_h, w_count) and e["mean_error_over_bound"] <= 1 and e["std_error_over_bound"] <= 1)
        e["equal"] = bool(np.array_equal(idx_h, w_idx) and d2.cpu().numpy().tobytes() == w_d2.tobytes()
                          and np.array_equal(pic.cpu().numpy(), w_pic) and order.cpu().numpy().tolist() == R.row_order(w_count).tolist())
        r["sizes"][str(n)] = e
        del x, patches
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print(json.dumps(r))


if __name__ == "__main__":
    main()
