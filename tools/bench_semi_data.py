"""The detector's file-backed data path (csrc/semi_data.hip, datasets/semi_files.py), one JSON line per record:

    python tools/bench_semi_data.py [--iters 20] [--steps 50]

  semi_labels  one mi_semi_labels call (zero, scatter, -1 fill) on the label volume of a 256 x 512 x 512 tomogram
               (256 x 256 x 256), 1000 and 5000 centres, bbox 16 and 36: median device time of --iters (events), the bytes
               the three passes move at least (zero 4 B, fill 8 B per voxel) over it, and the numpy restatement
               (tests/test_oracle_semi_data.py `np_labels`) timed once; the result is compared bit for bit
  semi_pairs   one mi_semi_pairs launch at batch 1 and 16 (2B crops of 6 x 64 x 64 in, twice, 6 x 32 x 32 labels): median
               device time, bytes moved, and numpy slicing + flipping of the same table
  data_step    host time per training batch of the data path alone (iterate the dataset, synchronise), the file-backed
               dataset against SyntheticDetectorDataset (host crops, a host-to-device copy per batch), batch 1 and 16
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def _events(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def bench_labels(iters):
    from cet_pick_amd import _lib as L
    from cet_pick_amd.datasets import semi_files as SF
    from test_oracle_semi_data import np_labels
    shape = (256, 256, 256)
    rng = np.random.default_rng(3)
    for n in (1000, 5000):
        c = np.stack([rng.integers(0, shape[2], n), rng.integers(0, shape[1], n), rng.integers(0, shape[0], n)], 1).astype(np.int32)
        for bbox in (16, 36):
            r = SF.label_radius(bbox)
            st = SF.label_stencil(r)
            hm = torch.empty(shape, dtype=torch.float32, device="cuda")
            st_d, c_d = torch.as_tensor(st).cuda(), torch.as_tensor(c).cuda()

            def run():
                L.call("mi_semi_labels", hm, *shape, c_d, n, st_d, r, 1)
            ms = _events(run, iters)
            t0 = time.perf_counter()
            ref = np_labels(shape, c, st, True)
            cpu_s = time.perf_counter() - t0
            same = bool(np.array_equal(hm.cpu().numpy().view(np.uint32), ref.view(np.uint32)))
            vox = int(np.prod(shape))
            stamps = n * (2 * r + 1) ** 3
            nbytes = 12 * vox                     # zero (write) + fill (read + write)
            print(json.dumps({"metric": "semi_labels", "label": list(shape), "centres": n, "bbox": bbox, "radius": r,
                              "stamp_voxels": stamps, "device_ms": round(ms, 4), "min_bytes": nbytes,
                              "gbs": round(nbytes / ms / 1e6, 1), "numpy_s": round(cpu_s, 3), "bit_equal": same}))


def bench_pairs(iters):
    from cet_pick_amd.datasets import semi_files as SF
    shapes = np.array([(256, 512, 512), (128, 512, 512)], np.int64)
    rng = np.random.default_rng(4)
    tomos = [torch.rand(tuple(int(v) for v in s), device="cuda") for s in shapes]
    labels = [torch.rand((int(s[0]), int(s[1]) // 2, int(s[2]) // 2), device="cuda") for s in shapes]
    tdesc, ldesc = SF._descriptors(tomos, "cuda"), SF._descriptors(labels, "cuda")
    anns = np.concatenate([np.stack([rng.integers(0, s[2] // 2, 500), rng.integers(0, s[1] // 2, 500), rng.integers(0, s[0], 500),
                                     np.full(500, t)], 1) for t, s in enumerate(shapes)], 0)
    t_h = [t.cpu().numpy() for t in tomos]
    l_h = [t.cpu().numpy() for t in labels]
    for batch in (1, 16):
        owner, cen, _ = SF.draw_pairs(anns, shapes, 16, 0.5, seed=1, epoch=0, batch_size=batch)
        o_d, c_d = torch.as_tensor(owner).cuda(), torch.as_tensor(cen).cuda()
        out = SF.semi_pairs(tdesc, ldesc, 2, o_d, c_d, 0, 2 * batch, True)
        ms = _events(lambda: SF.semi_pairs(tdesc, ldesc, 2, o_d, c_d, 0, 2 * batch, True, out=out), iters)
        t0 = time.perf_counter()
        for _ in range(5):
            inp = np.stack([t_h[owner[s]][z - 3:z + 3, 2 * y - 32:2 * y + 32, 2 * x - 32:2 * x + 32]
                            for s, (x, y, z) in enumerate(cen[:2 * batch])])
            aug = np.ascontiguousarray(np.flip(inp, 2))
            hm = np.stack([l_h[owner[s]][z - 3:z + 3, y - 16:y + 16, x - 16:x + 16] for s, (x, y, z) in enumerate(cen[:2 * batch])])
        cpu_ms = (time.perf_counter() - t0) * 1e3 / 5
        same = bool(np.array_equal(out[0].cpu().numpy(), inp) and np.array_equal(out[1].cpu().numpy(), aug) and
                    np.array_equal(out[2].cpu().numpy()[:, 0], hm))
        nbytes = 2 * batch * (3 * 6 * 64 * 64 + 2 * 6 * 32 * 32) * 4      # read + 2 writes of the input, read + write of the label
        print(json.dumps({"metric": "semi_pairs", "batch": batch, "crops": 2 * batch, "device_ms": round(ms, 4),
                          "bytes": nbytes, "gbs": round(nbytes / ms / 1e6, 1), "numpy_ms": round(cpu_ms, 3), "bit_equal": same}))


def bench_data_step(steps):
    from cet_pick_amd.datasets.semi_files import TomoFileDetectorDataset
    from cet_pick_amd.datasets.synthetic_datasets import SyntheticDetectorDataset
    from cet_pick_amd.synthetic import make_tomo
    tomos, coords = {}, {}
    for i in range(2):
        vol, c = make_tomo((32, 256, 256), seed=70 + i, margin_xy=40, margin_z=6, blob_spacing=8)
        tomos["t%d" % i], coords["t%d" % i] = torch.as_tensor(vol).cuda(), c
    for batch in (1, 16):
        opt = SimpleNamespace(down_ratio=2, pn=False, bbox=16, translation_ratio=0.5, fiber=False, compress=False,
                              batch_size=batch, seed=1)
        # enough annotations for --steps batches: the same centres repeated (the timing does not depend on them)
        reps = max(1, -(-steps * batch // sum(len(c) for c in coords.values())))
        files = TomoFileDetectorDataset.from_arrays(opt, "train", tomos, {k: np.tile(v, (reps, 1)) for k, v in coords.items()})
        syn = SyntheticDetectorDataset(opt, "train", per_epoch=steps * batch, device="cuda")
        res = {}
        for name, ds in (("files", files), ("synthetic", syn)):
            ds.set_epoch(0)
            for _ in ds:                           # (warm-up epoch)
                pass
            ds.set_epoch(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = 0
            for b in ds:
                torch.cuda.synchronize()
                k += 1
                if k == steps:
                    break
            res[name] = (time.perf_counter() - t0) * 1e3 / k
        print(json.dumps({"metric": "semi_data_step", "batch": batch, "steps": steps, "files_ms": round(res["files"], 4),
                          "synthetic_ms": round(res["synthetic"], 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_semi_data.py needs the MI355X")
    bench_labels(a.iters)
    bench_pairs(a.iters)
    bench_data_step(a.steps)


if __name__ == "__main__":
    main()
