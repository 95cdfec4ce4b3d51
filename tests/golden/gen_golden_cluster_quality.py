"""Golden values of the cluster-quality tests -> cluster_quality/small.npz, from scikit-learn in float64.  Run on the host:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_cluster_quality.py
The fixture holds results only; the inputs are tests/cluster_quality_ref.py::make(name) and second_labeling(labels).
  sil_{name} (N,) float64: sklearn.metrics.silhouette_samples(x as float64, labels) for every name of VARIANTS
  ari_{name}, nmi_{name}: adjusted_rand_score and normalized_mutual_info_score (arithmetic mean) of labels against
      second_labeling(labels)
The conditions the device tests rely on are asserted here, from float64 alone: at most 1 % of a case's picks have the two
nearest other classes closer together than twice the bound on b (the share is 0 on these inputs), and the largest bound on s is
small against the silhouettes themselves."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score, silhouette_samples  # noqa: E402
import cluster_quality_ref as R  # noqa: E402


def main():
    out = {}
    for name in R.VARIANTS:
        x, labels = R.make(name)
        out["sil_" + name] = silhouette_samples(x.astype(np.float64), labels)
        other = R.second_labeling(labels)
        out["ari_" + name] = np.float64(adjusted_rand_score(labels, other))
        out["nmi_" + name] = np.float64(normalized_mutual_info_score(labels, other))
        S, E, fin = R.silhouette64(x, labels)
        ea, eb, es, decided = R.bounds(E, fin)
        assert (~decided).mean() <= 0.01, name
        print("%-7s N=%d mean silhouette %.4f  restatement - sklearn %.2e  largest bound on s %.2e  undecided nearest %.3f %%  "
              "ARI %.4f NMI %.4f" % (name, len(x), out["sil_" + name].mean(), np.abs(fin["s"] - out["sil_" + name]).max(),
                                     es.max(), 100 * (~decided).mean(), out["ari_" + name], out["nmi_" + name]))
    os.makedirs(os.path.dirname(R.GOLDEN), exist_ok=True)
    np.savez(R.GOLDEN, **out)


if __name__ == "__main__":
    main()
