"""Cost of the 3-D visualisation of one tomogram (csrc/vis3d.hip, utils/vis3d.py), one JSON line and profiles/vis3d_bench.json:

    python tools/bench_vis3d.py [--out profiles/vis3d_bench.json] [--shape 128x512x512] [--picks 5000] [--reps 20] [--no_host]

HIP events around one call, median of --reps calls after a warm-up of 3:
  gauss_us      mi_vis_gauss_u8 (three launches).  gauss_bytes = 8 per voxel as built (1 + 1, 1 + 1, 1 + 3: byte intermediates
                between the passes), gauss_min_bytes = 4 per voxel (read once, write three channels); *_frac_hbm = bytes / t / 8 TB/s
  paint_us      mi_vis_paint (memset, scatter, paint pass).  paint_bytes = index zeroed + index read + volume written
  chain_us      the normalisation chain in front of the filter (two statistics passes, two per-slice passes)
  tomogram_us   the whole device work of one tomogram: chain, filter and painter, from the reordered fp32 volume to both volumes
  host_*_ms     the numpy / scipy restatement of tests/vis3d_ref.py on this host's CPU (one core), and whether the device's
                bytes equal it at this size (`*_equal`; the chain by its rule: `chain_differ_clear` must be 0)
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

HBM_CEILING = 8e12


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
    return float(np.median(times)), [round(t, 1) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vis3d_bench.json"))
    ap.add_argument("--shape", default="128x512x512")
    ap.add_argument("--picks", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no_host", action="store_true", help="leave the host restatement (and the comparison with it) out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    from cet_pick_amd.build import source_sha16
    from cet_pick_amd.utils import vis3d as V
    z, r, c = (int(v) for v in a.shape.split("x"))
    vox = z * r * c
    rng = np.random.RandomState(0)
    vol_h = (rng.standard_normal((z, r, c)) * 30 + 10).astype(np.float32)
    coords = np.stack([rng.uniform(0, c, a.picks), rng.uniform(0, r, a.picks), rng.randint(0, z, a.picks)], 1)
    colours = rng.randint(1, 256, size=(a.picks, 3)).astype(np.uint8)
    names = np.array(["t"] * a.picks)
    rows, picks = V.tomogram_picks(coords, names, "t", z)
    n_slots = len(np.unique(picks[:, 2]))
    vol = torch.from_numpy(vol_h).cuda()
    u8 = V.volume_bytes(vol)

    out = {"kernels_sha16": source_sha16(["vis3d", "preproc"]), "device": torch.cuda.get_device_name(0),
           "ceilings": {"hbm_tbs": HBM_CEILING / 1e12}, "shape": [z, r, c], "picks": a.picks, "painted_slices": n_slots,
           "reps": a.reps}
    out["gauss_us"], out["gauss_us_all"] = _events_us(lambda: V.gaussian_u8(u8), a.reps)
    out["paint_us"], out["paint_us_all"] = _events_us(lambda: V.paint(picks, colours, (z, r, c)), a.reps)
    out["chain_us"], _ = _events_us(lambda: V.volume_bytes(vol), a.reps)
    out["tomogram_us"], out["tomogram_us_all"] = _events_us(lambda: (V.rec3d(vol), V.paint(picks, colours, (z, r, c))), a.reps)
    out["gauss_bytes"], out["gauss_min_bytes"] = 8 * vox, 4 * vox
    out["paint_bytes"] = 2 * 4 * n_slots * r * c + 3 * vox
    for k, b in (("gauss", out["gauss_bytes"]), ("gauss_min", out["gauss_min_bytes"]), ("paint", out["paint_bytes"])):
        t = out["gauss_us" if k.startswith("gauss") else "paint_us"] * 1e-6
        out[k + "_tbs"] = b / t / 1e12
        out[k + "_frac_hbm"] = b / t / HBM_CEILING
    print(json.dumps({k: v for k, v in out.items() if not k.endswith("_all")}), flush=True)

    if not a.no_host:
        import vis3d_ref as R
        u8_h = u8.cpu().numpy()
        t0 = time.perf_counter()
        want = R.gaussian_scipy(u8_h)
        out["host_gauss_ms"] = (time.perf_counter() - t0) * 1e3
        out["gauss_equal"] = bool(np.array_equal(V.gaussian_u8(u8).cpu().numpy(), want))
        del want
        print(json.dumps({"host_gauss_ms": out["host_gauss_ms"], "gauss_equal": out["gauss_equal"]}), flush=True)
        t0 = time.perf_counter()
        want, level = R.volume_chain(vol_h.astype(np.float64))
        out["host_chain_ms"] = (time.perf_counter() - t0) * 1e3
        clear = np.abs(level - np.floor(level) - 0.5) > 1e-3
        out["chain_differ"], out["chain_differ_clear"] = int((u8_h != want).sum()), int(((u8_h != want) & clear).sum())
        del want, level, clear
        print(json.dumps({"host_chain_ms": out["host_chain_ms"], "chain_differ_clear": out["chain_differ_clear"]}), flush=True)
        t0 = time.perf_counter()
        want = R.paint(picks.astype(np.int64), colours, (z, r, c))
        out["host_paint_ms"] = (time.perf_counter() - t0) * 1e3
        out["paint_equal"] = bool(np.array_equal(V.paint(picks, colours, (z, r, c)).cpu().numpy(), want))
        out["host_tomogram_ms"] = out["host_gauss_ms"] + out["host_chain_ms"] + out["host_paint_ms"]
        out["tomogram_speedup"] = out["host_tomogram_ms"] * 1e3 / out["tomogram_us"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if not k.endswith("_all")}))


if __name__ == "__main__":
    main()
