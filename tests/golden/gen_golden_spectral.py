"""Writes tests/golden/spectral_small.npz (CPU only; needs scipy and sklearn):  python tests/golden/gen_golden_spectral.py

Two fixtures of tests/spectral_ref.strip (points uniform on a 3 x 1 strip behind a random 2 -> 32 linear map, 0.01 noise), their
graphs by spectral_ref.knn and spectral_ref.graph_tables (the float64 smooth distances and union, wsym as fp32), 500 epochs:
  strip   600 points, seed STRIP_SEED, n_neighbors K = 15 (14 columns)
  small    96 points, seed SMALL_SEED, n_neighbors K = 8 (7 columns)
Recorded, as results only: the generating seeds and sizes; lam, the seven smallest eigenvalues of L = I - D^-1/2 W D^-1/2 by the
dense float64 solve; gap, the distance of lam_1 and lam_2 to the rest of the spectrum; and for the strip at min_dist 0.5, seed 42
  trust_spectral   sklearn.manifold.trustworthiness(x, Y, n_neighbors=5) of umap_ref's float64 fit run from spectral_ref's start
  trust_random     the same figure of the fit from umap-learn's random start (recorded, never asserted on)
Both graphs must have one component and gaps above GAP_FLOOR, or nothing is written: a changed seed cannot pass with a
degenerate spectrum.
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import spectral_ref as R  # noqa: E402
import umap_ref as U  # noqa: E402

STRIP_N, STRIP_K, STRIP_SEED = 600, 15, 1
SMALL_N, SMALL_K, SMALL_SEED = 96, 8, 1
N_EPOCHS, MIN_DIST, SEED, GAP_FLOOR = 500, 0.5, 42, 1e-3


def graph(n, K, seed):
    x, _ = R.strip(n, seed)
    index, dist2 = R.knn(x, K - 1)
    wsym, mutual, eps = R.graph_tables(index, dist2, N_EPOCHS)
    return x, index, dist2, R.dense_w(index, wsym, eps)


def spectrum(n, K, seed):
    x, index, dist2, W = graph(n, K, seed)
    assert len(np.unique(R.components(W))) == 1, "the graph has more than one component"
    lam, v, gap = R.eigenpairs(W, 2)
    assert gap.min() >= GAP_FLOOR, "gaps %s below the floor %g" % (gap, GAP_FLOOR)
    res = np.abs((np.eye(n) - R.normalised(W)[0]) @ v - v * lam[1:3]).max()
    print("N=%d K=%d seed %d: lam %s, gaps %s, residual %.2e" % (n, K, seed, np.array2string(lam[:7], precision=4), gap, res))
    return lam[:7], gap


def fit(form):
    from sklearn.manifold import trustworthiness
    x, index, dist2, W = graph(STRIP_N, STRIP_K, STRIP_SEED)
    a, b = U.find_ab(MIN_DIST)
    y0 = R.start(R.layout(W, 2, SEED)[0], SEED) if form == "spectral" else U.start(STRIP_N, SEED)
    Y = R.fit64_from(index, dist2, a, b, SEED, y0, N_EPOCHS)
    return float(trustworthiness(x, Y, n_neighbors=5))


def main():
    with ProcessPoolExecutor(2) as ex:
        trust = list(ex.map(fit, ("spectral", "random")))
    print("trustworthiness of the float64 fit: spectral start %.4f, random start %.4f" % tuple(trust))
    strip_lam, strip_gap = spectrum(STRIP_N, STRIP_K, STRIP_SEED)
    small_lam, small_gap = spectrum(SMALL_N, SMALL_K, SMALL_SEED)
    out = os.path.join(HERE, "spectral_small.npz")
    np.savez_compressed(out, strip=np.array([STRIP_N, STRIP_K, STRIP_SEED], np.int32), small=np.array([SMALL_N, SMALL_K, SMALL_SEED], np.int32),
                        n_epochs=np.int32(N_EPOCHS), min_dist=np.float64(MIN_DIST), seed=np.int32(SEED), gap_floor=np.float64(GAP_FLOOR),
                        strip_lam=strip_lam, strip_gap=strip_gap, small_lam=small_lam, small_gap=small_gap,
                        trust_spectral=np.float64(trust[0]), trust_random=np.float64(trust[1]))
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
