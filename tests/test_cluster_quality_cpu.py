"""The host side of the cluster-quality step: the float64 restatement against scikit-learn's stored values, ARI
and NMI from a table, the flags' parsing and refusals, and the entries that need no device."""
import argparse

import numpy as np
import pytest

import cluster_quality_ref as R


@pytest.mark.parametrize("name", R.VARIANTS)
def test_restatement_equals_sklearn_golden(name):
    gold = np.load(R.GOLDEN)
    x, labels = R.make(name)
    S, E, fin = R.silhouette64(x, labels)
    err = np.abs(fin["s"] - gold["sil_" + name]).max()
    print("%s: restatement - sklearn %.2e" % (name, err))
    assert err <= 1e-12
    ea, eb, es, decided = R.bounds(E, fin)
    assert (~decided).mean() <= 0.01 and 0 < es.max() < 1e-3 < abs(fin["s"].mean())      # the bound says something


@pytest.mark.parametrize("name", R.VARIANTS)
def test_ari_nmi_from_a_table(name):
    from cet_pick_amd.utils.cluster_quality import ari_nmi
    gold = np.load(R.GOLDEN)
    labels = R.make(name)[1]
    table = R.contingency(labels, R.second_labeling(labels))[0]
    ari, nmi = ari_nmi(table)
    assert abs(ari - float(gold["ari_" + name])) <= 1e-12 and abs(nmi - float(gold["nmi_" + name])) <= 1e-12
    same = R.contingency(labels, labels * 2 + 5)[0]
    assert ari_nmi(same) == (1.0, pytest.approx(1.0, abs=1e-12))
    assert ari_nmi(np.array([[5, 0]]).T) == (1.0, 1.0)     # one class each: sklearn's 1.0
    assert ari_nmi(np.array([[3, 3], [3, 3]]))[1] == 0.0


def test_flag_parsing_and_refusals(tmp_path):
    from cet_pick_amd import plot_2d as P
    from cet_pick_amd import scan_main as M
    from cet_pick_amd.utils.cluster_quality import parse_sweep
    assert parse_sweep("4,8,16") == [4, 8, 16] and parse_sweep(" 3 , 2,") == [3, 2]
    for bad in ("", ",", "4,x", "4,1", "0", "4,4"):
        with pytest.raises(ValueError):
            parse_sweep(bad)

    def parse(*flags):
        return P.add_arguments(argparse.ArgumentParser()).parse_args(["--input", "i.npz", "--path", "o", "--k", "8"] + list(flags))

    assert P.quality_plan(parse(), 10) is None
    assert P.quality_plan(parse("--quality"), 10) == (None, None)
    assert P.quality_plan(parse("--sweep_n_cluster", "2,7"), 10) == ([2, 7], None)
    with pytest.raises(ValueError, match="into fewer"):
        P.quality_plan(parse("--sweep_n_cluster", "2,8"), 10)
    np.savez(tmp_path / "l.npz", label=np.arange(10) % 3, name=np.arange(10))
    np.savez(tmp_path / "nolabel.npz", labels=np.arange(10))
    sweep, other = P.quality_plan(parse("--compare_labels", str(tmp_path / "l.npz")), 10)
    assert sweep is None and np.array_equal(other, np.arange(10) % 3)
    with pytest.raises(ValueError, match="labels 10 picks, the input has 11"):
        P.quality_plan(parse("--compare_labels", str(tmp_path / "l.npz")), 11)
    with pytest.raises(ValueError, match="holds no 'label'"):
        P.quality_plan(parse("--compare_labels", str(tmp_path / "nolabel.npz")), 10)
    args = M.add_arguments(argparse.ArgumentParser()).parse_args(["--input", "i.npz", "--path", "o", "--nclusters", "3", "--quality"])
    assert args.quality is True


def test_wrappers_have_no_cpu_path():
    import torch
    from cet_pick_amd import hipops as H
    from cet_pick_amd._lib import HipExtensionError
    from cet_pick_amd.utils import cluster_quality as Q
    x, lab = torch.zeros(8, 4), torch.zeros(8, dtype=torch.int32)
    with pytest.raises(HipExtensionError):
        H.silhouette_sums(x, lab, 2)
    with pytest.raises(HipExtensionError):
        H.silhouette_finalise(torch.zeros(8, 2, dtype=torch.float64), lab)
    with pytest.raises(HipExtensionError):
        H.label_contingency(lab, lab, 1, 1)
    with pytest.raises(HipExtensionError):
        Q.silhouette(x.numpy(), lab.numpy())
    with pytest.raises(HipExtensionError):
        Q.silhouette(x, lab)
    with pytest.raises(HipExtensionError):
        Q.SilhouetteSums(x.numpy(), lab.numpy(), 2, device="cpu")
    with pytest.raises(HipExtensionError):
        Q.compare_labelings(lab.numpy(), lab.numpy(), device="cpu")


def test_workspace_sizes_need_no_device():
    import __graft_entry__ as ge
    ge.build()
    from cet_pick_amd import _lib
    L = _lib.lib()
    sil, fin = L.mi_silhouette_workspace_bytes, L.mi_silhouette_finalise_workspace_bytes
    assert sil(1003, 17, 7) > 0 and sil(200000, 128, 256) > 200000 * 256 * 8 and sil(2, 1, 1) > 0 and sil(1000, 512, 1024) > 0
    assert sil(1000, 513, 7) == 0 and sil(1000, 0, 7) == 0 and sil(1000, 16, 1025) == 0 and sil(1000, 16, 0) == 0
    assert sil(1, 16, 2) == 0 and sil(1 << 31, 16, 2) == 0 and sil((1 << 31) - 1, 16, 2) > (1 << 35)
    assert fin(1000, 7, 7) > 0 and fin(1000, 1024, 1024) > 0 and fin(1000, 8, 2) > 0
    assert fin(1000, 7, 1) == 0 and fin(1000, 1025, 4) == 0 and fin(1000, 7, 1025) == 0 and fin(1, 7, 7) == 0 and fin(1 << 31, 7, 7) == 0
