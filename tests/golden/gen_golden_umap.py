"""Writes tests/golden/umap_small.npz (CPU only; needs scipy and sklearn):  python tests/golden/gen_golden_umap.py

x, label and the neighbour graph of tsne_small.npz (600 x 32 in six blobs), n_neighbors K = 15 (the first 14 columns of the
recorded search), min_dist 0.5, 500 epochs.  Recorded, as results only:
  ab                        tests/umap_ref.find_ab(0.5)
  seq_seeds, seq_agree,     for every seed of umap_ref.sequential_fit64 (umap-learn's in-place loop, in plain Python: minutes
  seq_trust                 per seed, run side by side): tsne_ref.neighbour_agreement with the blob labels and
                            sklearn.manifold.trustworthiness(x, Y, n_neighbors=5)
  sync_seed, sync_agree,    the same two figures of umap_ref.fit64, the epoch-synchronous form the device runs, at seed 42
  sync_trust
  trust_margin              max - min of seq_trust
The synchronous form has to meet the caps the GPU test applies to the device (agreement >= min seq_agree, trustworthiness >=
min seq_trust - trust_margin); if it does not, nothing is written.
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import tsne_ref as T  # noqa: E402
import umap_ref as U  # noqa: E402

K, MIN_DIST, SEQ_SEEDS, SYNC_SEED = 15, 0.5, (0, 1, 2, 3, 4), 42


def run(job):
    from sklearn.manifold import trustworthiness
    form, seed = job
    z = np.load(os.path.join(HERE, "tsne_small.npz"))
    x, label = z["x"], z["label"].astype(np.int64)
    index, dist2 = z["index"].astype(np.int64)[:, :K - 1], z["dist"][:, :K - 1]
    a, b = U.find_ab(MIN_DIST)
    Y = (U.sequential_fit64 if form == "sequential" else U.fit64)(index, dist2, a, b, seed)
    return form, seed, T.neighbour_agreement(Y, label), float(trustworthiness(x, Y, n_neighbors=5))


def main():
    jobs = [("sequential", s) for s in SEQ_SEEDS] + [("synchronous", SYNC_SEED)]
    with ProcessPoolExecutor(len(jobs)) as ex:
        res = list(ex.map(run, jobs))
    for form, seed, agree, trust in res:
        print("%s seed %d: agreement %.4f, trustworthiness %.4f" % (form, seed, agree, trust))
    seq = [r for r in res if r[0] == "sequential"]
    seq_agree, seq_trust = np.array([r[2] for r in seq]), np.array([r[3] for r in seq])
    _, _, sync_agree, sync_trust = res[-1]
    margin = float(seq_trust.max() - seq_trust.min())
    print("caps: agreement >= %.4f, trustworthiness >= %.4f - %.4f" % (seq_agree.min(), seq_trust.min(), margin))
    assert sync_agree >= seq_agree.min() and sync_trust >= seq_trust.min() - margin, "the synchronous form misses its own caps"
    out = os.path.join(HERE, "umap_small.npz")
    np.savez_compressed(out, n_neighbors=np.int32(K), min_dist=np.float64(MIN_DIST), ab=np.array(U.find_ab(MIN_DIST)),
                        seq_seeds=np.array(SEQ_SEEDS, np.int32), seq_agree=seq_agree, seq_trust=seq_trust,
                        sync_seed=np.int32(SYNC_SEED), sync_agree=np.float64(sync_agree), sync_trust=np.float64(sync_trust),
                        trust_margin=np.float64(margin))
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
