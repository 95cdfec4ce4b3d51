"""Writes tests/golden/tsne_small.npz (CPU only; needs sklearn):  python tests/golden/gen_golden_tsne.py

x = 600 x 32 in six blobs (tsne_ref.make_blobs, seed 11), perplexity 5, K = 16 neighbours from the float64 arbiter of the
neighbour search.  Recorded from sklearn, as results only:
  sk_row, sk_col, sk_val   the joint affinities sklearn.manifold._t_sne._joint_probabilities_nn makes from that graph
  sk_kl                    for five seeds of sklearn.manifold.TSNE(perplexity=5, init="random", max_iter=1000): the float64
                           divergence tsne_ref.kl64 of sklearn's embedding against the arbiter's joint affinities
  sk_agree                 for the same embeddings: tsne_ref.neighbour_agreement with the blob labels
  kl_margin                twice the relative spread (max - min) / min of sk_kl
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import knn_ref  # noqa: E402
import tsne_ref as T  # noqa: E402

N, D, BLOBS, DATA_SEED, PERPLEXITY, SEEDS = 600, 32, 6, 11, 5, (0, 1, 2, 3, 4)


def main():
    from scipy.sparse import csr_matrix
    from sklearn.manifold import TSNE
    from sklearn.manifold._t_sne import _joint_probabilities_nn
    x, label = T.make_blobs(N, D, BLOBS, DATA_SEED)
    K = min(N - 1, 3 * PERPLEXITY + 1)
    index, dist = knn_ref.topk64(x, x, K, "l2", exclude_self=True)
    dist = dist.astype(np.float32)
    graph = csr_matrix((dist.reshape(-1).copy(), index.reshape(-1).copy(), np.arange(0, N * K + 1, K)), shape=(N, N))   # sorted in place
    sk = _joint_probabilities_nn(graph, PERPLEXITY, 0).tocoo()
    P = T.joint_P(index, T.affinities64(dist, PERPLEXITY)[0])
    kls, agree = [], []
    for seed in SEEDS:
        try:
            ts = TSNE(n_components=2, perplexity=PERPLEXITY, init="random", random_state=seed, max_iter=1000)
        except TypeError:                                           # sklearn before 1.5
            ts = TSNE(n_components=2, perplexity=PERPLEXITY, init="random", random_state=seed, n_iter=1000)
        Y = ts.fit_transform(x)
        kls.append(T.kl64(Y, P))
        agree.append(T.neighbour_agreement(Y, label))
        print("seed %d: sklearn's own KL %.6f, KL64 %.6f, agreement %.4f" % (seed, ts.kl_divergence_, kls[-1], agree[-1]))
    kls = np.array(kls)
    spread = (kls.max() - kls.min()) / kls.min()
    print("relative spread of KL64 %.4f -> margin %.4f" % (spread, 2 * spread))
    assert spread <= 0.25, "sklearn's own runs spread by more than 25 %: choose better separated blobs"
    out = os.path.join(HERE, "tsne_small.npz")
    np.savez_compressed(out, x=x, label=label.astype(np.int16), index=index.astype(np.int16), dist=dist, perplexity=np.int32(PERPLEXITY),
                        sk_row=sk.row.astype(np.int16), sk_col=sk.col.astype(np.int16), sk_val=sk.data.astype(np.float64),
                        sk_kl=kls, sk_agree=np.array(agree), kl_margin=np.float64(2 * spread), seeds=np.array(SEEDS, np.int32))
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
