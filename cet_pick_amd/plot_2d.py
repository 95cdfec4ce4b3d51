"""Cluster the exploration embeddings, write the per-pick class table and the 2-D UMAP or t-SNE map (the reference's
plot_2d.py; its pictures and thumbnails with --min_dist_vis):

    python -m cet_pick_amd.plot_2d --input exp/.../all_output_info.npz --path OUT --n_cluster 48 [--k 256] [--niter 300]
                                   [--seed 1234] [--gpus 0] [--host 7000] [--num_neighbor K] [--mode umap | --mode tsne]
                                   [--min_dist_umap 0.5] [--map_seed 42] [--colormap FILE.npy] [--umap_init random | spectral]
                                   [--label_map] [--target_weight 0.5] [--min_dist_vis 1.3e-3] [--save_out_img 1]
                                   [--plot_size 1500] [--class_gallery [--gallery_exemplars 8]]
                                   [--quality] [--sweep_n_cluster 4,8,16] [--compare_labels FILE.npz]

`pred` of the input is over-clustered by k-means on the MI355X (utils/kmeans.py: k = 256 centroids, 300 iterations, as the
reference runs faiss), the centroids are merged into --n_cluster classes on the host (sklearn's SpectralClustering with the
reference's arguments; --n_cluster 0 keeps the k-means assignment as the class), and every pick gets the class of its centroid.

    OUT/kmeans_labels.npz                 centroids (k, d) f32, assign (N,) i32, dist (N,) f32, label (N,) i32, obj (niter,) f32,
                                          name, coords: numpy only, always written
    OUT/interactive_info_parquet.gzip     the reference's table (name, coord, embeddings, label, image) where pandas with a
                                          parquet engine imports
    OUT/knn_graph.npz                     with --num_neighbor K only: index (N, K) i32 and dist (N, K) f32, the K nearest other
                                          picks of every pick by squared L2 distance over `pred`, ascending (utils: csrc/knn.hip,
                                          lowest index on ties), and k - the graph a UMAP / t-SNE map starts from
    OUT/embeddings_2d.npz                 with --mode tsne --num_neighbor P only: the exact t-SNE map of `pred` at perplexity P
                                          (utils/tsne.py, csrc/tsne.hip: sklearn's schedule, 1000 iterations, its init="random"
                                          from --map_seed, the reference's --seed): y (N, 2) f32, y01 = (y - min) / (max - min)
                                          per axis as the reference normalises, kl, n_iter, perplexity, seed.  One search with
                                          min(N - 1, 3 P + 1) neighbours serves the map and, by its first P columns, the graph.
                                          With --mode umap --num_neighbor K, given EXPLICITLY: the UMAP map of `pred` with
                                          n_neighbors K and min_dist --min_dist_umap (utils/umap.py, csrc/umap.hip: umap-learn's
                                          constants in an epoch-synchronous form, its init="random" from --map_seed): y, y01,
                                          n_epochs, n_neighbors, min_dist, a, b, seed.  One search with K neighbours serves the
                                          graph and, by its first K - 1 columns (UMAP counts the pick itself), the map.
                                          --umap_init spectral starts the map as umap-learn does by default, from the eigenvectors
                                          of the graph's normalised Laplacian (utils/spectral.py, csrc/spectral.hip), and adds
                                          init (the start that was used: "random" where the eigen-solver did not converge),
                                          n_graph_components and eigenvalues (those of the largest component) to the file.
    OUT/embeddings_2d_labels.npz          with --label_map --num_neighbor K only, under any --mode: the label-supervised UMAP map,
                                          the reference's umap.UMAP(K, min_dist, random_state).fit_transform(projs, y=final_lbs)
                                          (DESIGN.md 4.16): the UMAP map steered by `label` of kmeans_labels.npz, from the first
                                          K - 1 columns of the search already made (no second search), with --min_dist_umap,
                                          --map_seed, --umap_init and --target_weight (umap-learn's 0.5): y, y01, label,
                                          n_epochs, n_neighbors, min_dist, a, b, seed, target_weight, far_dist, and with
                                          --umap_init spectral init, n_graph_components, eigenvalues of the supervised graph.
    OUT/all_colors.npy                    with the map: (N, 3) uint8, the colour of every pick at its y01 place on a 2-D colour
                                          table, in pick order (utils/vis3d.py, csrc/vis3d.hip: the reference's
                                          BaseColorMap2D._sample - round half to even, clamp) - the input of visualize_3dhm.
                                          --colormap FILE.npy takes any (W, H, 3) uint8 table, e.g. the Ziegler table of a
                                          reference installation.  The default table is NOT the reference's (its colour tables
                                          are its own data files): it is table[i, j] = (i, j, 255 - (i + j) // 2), 256 x 256.

Only an explicit `--mode umap` makes the UMAP map.  The reference's default mode is umap too, but a command line without
--mode has always run here without a map (with --num_neighbor: the graph alone), and scripts and tests rely on its output and on
the files it does not write; the parser therefore tells the given value from the default one (DefaultMode), and making the bare
default draw the map is a one-line change in main.

With --min_dist_vis D, GIVEN (the reference's documented value is 1.3e-3; without it nothing below is written), the input must
also hold `subvol` (N, C, b, b), and utils/plot2d.py with csrc/plot2d.hip make on the MI355X:

    OUT/imgs/{i}.png                      with --save_out_img 1 (the default): channel 0 of every pick's patch as the reference's
                                          plt.imsave(cmap='gray') writes it (RGBA, R = G = B, A = 255) - the files the `image`
                                          column of the parquet table points to.  The bytes come from the device; the PNG
                                          encoding is host work on OMP_NUM_THREADS threads (4 where it is not set).
    OUT/2d_visualization_out.png          with a map: --plot_size P (1500) pixels square.  The reference's filter picks the
                                          thumbnails (in input order, a pick is shown unless one shown before it, or pick 0, lies
                                          at a float32 squared y01 distance below D); every shown pick gets a disc of radius 0.03
                                          map units in its colour of all_colors.npy and over it its 32 x 32 thumbnail (z-score,
                                          quantize(-3, 3), torchvision's resize), later picks over earlier ones.
    OUT/2d_visualization_labels.png       with --label_map: the same selection on the y01 of embeddings_2d_labels.npz, every
                                          thumbnail tagged with its class number in a blue-framed box.
    OUT/plot_2d_shown.npz                 shown_idx and / or shown_idx_labels (int32, ascending), min_dist_vis (f32), plot_size,
                                          thumb: enough to rebuild or restyle a picture from the embeddings files.
    OUT/2d_visualization_*.webp           the same pictures, lossless, under the reference's own file names, where PIL with WebP
                                          support imports (one log line otherwise).

Without a map --min_dist_vis writes the imgs/ only.  Not made here: the Phoenix interactive session, and
matplotlib's own figure layout - the pictures have no axes, ticks, fonts or tight bounding box; their layout is fixed in
utils/plot2d.py.

With --class_gallery (this project's own; it stands in for looking at the classes in the Phoenix session) the
input must hold `subvol` (N, C, h, w), and utils/plot2d.class_gallery with csrc/class_gallery.hip make on the MI355X, for the
final classes (`label` of kmeans_labels.npz: the merged classes where --n_cluster merges, the centroids otherwise):

    OUT/class_gallery.npz                 mean, std (k, h, w) f32: per pixel the mean and population deviation of channel 0 of the
                                          class's patches; count (k,) i32; exemplar_index (k, m) i32: the m = --gallery_exemplars
                                          members nearest to their own k-means centroid (squared L2 over `pred`, ties by pick
                                          index), -1 where a class has fewer; exemplar_d2 (k, m) f64, +inf there; order (k,) i32:
                                          the class of every row of the picture, by descending count, then ascending class
    OUT/class_gallery.png (.webp)         one row per class: its number over its count, the mean patch, the deviation patch (one
                                          grey scale for all classes) and the exemplars - what --labels of
                                          interactive_to_training_coords is chosen from

With --quality (this project's own: the file that says how good a clustering is) utils/cluster_quality.py with
csrc/cluster_quality.hip make on the MI355X, in ONE pass over the N x N pairs of picks (no N x N matrix is stored):

    OUT/cluster_quality.npz               the exact silhouette (scikit-learn's silhouette_samples, Euclidean over `pred`) under the
                                          final classes (`label`): s, a, b (N,) f64 in pick order (a: mean distance to the own
                                          class, b: to the nearest other class, s = (b - a) / max(a, b); a = s = 0 for the only
                                          member of a class), nearest (N,) i32 (the class attaining b), class_mean (C,) f64 (NaN
                                          for a class without members), class_count (C,) i32, confusion (C, C) i32
                                          [own][nearest], mean; and the same under the k-means assignment itself (`assign`):
                                          fine_s, fine_a, ... fine_mean.  One stdout line gives the two means.
                                          --sweep_n_cluster 4,8,16 (implies --quality; each value in 2..k-1) merges the centroids
                                          to every listed class count as --n_cluster does and scores each from the SAME pass:
                                          sweep_n_cluster, sweep_mean, sweep_min_class_mean (the worst class), sweep_smallest_class
                                          (its member count), and a printed table.  It does not change which --n_cluster the other
                                          outputs use.  Needs sklearn, as --n_cluster does.
                                          --compare_labels FILE.npz (implies --quality) reads `label` of another labeling of the
                                          same picks (scan_labels.npz; what interactive_to_training_coords reads; -1 is a class of
                                          its own) and adds compare_table (classes of `label` x classes of the file, i64),
                                          compare_ids, compare_ids_other (the class ids of its rows and columns), compare_ari
                                          (adjusted Rand index) and compare_nmi (normalised mutual information, arithmetic mean).
                                          Another number of picks is a ValueError.
"""
import argparse
import os

import numpy as np


class DefaultMode(str):
    """The value of --mode on a command line that does not give it: equal to "umap", and told from a given "umap" by its type."""


def add_arguments(parser):
    parser.add_argument("--input", required=True, help="all_output_info.npz of the exploration inference (pred, name, coords)")
    parser.add_argument("--path", required=True, help="output directory")
    parser.add_argument("--n_cluster", type=int, default=0, help="classes after merging the centroids; 0 (or >= k): no merge")
    parser.add_argument("--k", type=int, default=256, help="k-means centroids (the reference: 256)")
    parser.add_argument("--niter", type=int, default=300, help="k-means iterations (the reference: 300)")
    parser.add_argument("--seed", type=int, default=1234, help="seed of the initial centroids (the reference passes 1234 to faiss)")
    parser.add_argument("--host", type=int, default=7000, help="port in the image URLs of the parquet table")
    parser.add_argument("--gpus", default="0", help="GPU index; -1 (CPU) is refused")
    parser.add_argument("--num_neighbor", type=int, default=None,
                        help="also write knn_graph.npz: the K nearest other picks of every pick (squared L2 over pred)")
    parser.add_argument("--mode", default=DefaultMode("umap"), help="with --num_neighbor K also write embeddings_2d.npz: tsne, the "
                        "t-SNE map at perplexity K; umap, given explicitly, the UMAP map with n_neighbors K.  Without --mode no "
                        "map is made")
    parser.add_argument("--map_seed", type=int, default=42, help="seed of the map's random start (the reference's --seed)")
    parser.add_argument("--colormap", default=None, help="(W, H, 3) uint8 .npy colour table for all_colors.npy; the default is a "
                        "built-in 256 x 256 table, not one of the reference's")
    parser.add_argument("--min_dist_umap", type=float, default=0.5, help="min_dist of the UMAP map (the reference: 0.5)")
    parser.add_argument("--umap_init", choices=("random", "spectral"), default="random", help="start of the UMAP map: random, or "
                        "spectral as umap-learn's default (embeddings_2d.npz then also holds init, n_graph_components, eigenvalues)")
    parser.add_argument("--label_map", action="store_true", help="with --num_neighbor K, under any --mode: also write "
                        "embeddings_2d_labels.npz, the UMAP map steered by the class of every pick (the reference's second map)")
    parser.add_argument("--target_weight", type=float, default=0.5, help="weight of the classes in the label-supervised map, 0..1 "
                        "(umap-learn's default: 0.5)")
    parser.add_argument("--min_dist_vis", type=float, default=None, help="when given: write imgs/{i}.png and, with a map, the "
                        "pictures; a pick gets a thumbnail unless one shown before it lies at a SQUARED map distance below this "
                        "(the reference's documented value: 1.3e-3)")
    parser.add_argument("--save_out_img", type=int, default=1, help="with --min_dist_vis: 1 writes imgs/{i}.png, anything else "
                        "leaves them out")
    parser.add_argument("--plot_size", type=int, default=1500, help="side of the pictures in pixels, at least 128 (the "
                        "reference: 15 in at 100 dpi)")
    parser.add_argument("--class_gallery", action="store_true", help="also write class_gallery.npz and class_gallery.png: per "
                        "class the mean patch, the spread and number of its members and its most typical members (needs subvol)")
    parser.add_argument("--gallery_exemplars", type=int, default=8, help="with --class_gallery: members shown per class, 1..64, "
                        "the nearest to their centroid first")
    parser.add_argument("--quality", action="store_true", help="also write cluster_quality.npz: the exact silhouette of every pick "
                        "under the final classes and under the k-means assignment")
    parser.add_argument("--sweep_n_cluster", default=None, help="comma-separated class counts, each in 2..k-1: merge the centroids "
                        "to each and add its silhouette to cluster_quality.npz (implies --quality; --n_cluster still decides the outputs)")
    parser.add_argument("--compare_labels", default=None, help="FILE.npz with `label` of the same picks (scan_labels.npz): add the "
                        "contingency table, adjusted Rand index and normalised mutual information against the final classes to "
                        "cluster_quality.npz (implies --quality)")
    return parser


def merge_centroids(centroids, n_cluster):
    """The reference's host step on the k centroids: class of every centroid, (k,) int."""
    try:
        from sklearn.cluster import SpectralClustering
    except ImportError as e:
        raise RuntimeError("--n_cluster %d merges the centroids with sklearn.cluster.SpectralClustering, and sklearn does not "
                           "import (%s); use --n_cluster 0 to keep the k-means assignment as the class" % (n_cluster, e)) from None
    sc = SpectralClustering(n_clusters=n_cluster, assign_labels="discretize", random_state=0)
    sc.fit(centroids)
    return np.asarray(sc.labels_)


def write_parquet(path, names, coords, projs, labels, host):
    """The reference's table; False (one log line) where pandas or a parquet engine does not import."""
    try:
        import pandas as pd
        try:
            import pyarrow  # noqa: F401
        except ImportError:
            import fastparquet  # noqa: F401
    except ImportError as e:
        print("[cet_pick_amd] %s left out: pandas with a parquet engine does not import (%s)" % (path, e))
        return False
    rela = "http://localhost:{}/imgs/".format(host)
    table = {"name": list(names), "coord": [[str(j) for j in list(c)] for c in coords], "embeddings": [list(p) for p in projs],
             "label": list(labels), "image": [os.path.join(rela, str(i) + ".png") for i in range(len(names))]}
    pd.DataFrame.from_dict(table).to_parquet(path, compression="gzip")
    return True


def knn_graph(projs, k, device):
    """index (N, k) int32, dist (N, k) fp32: the k nearest other rows of every row of projs, squared L2, ascending."""
    import torch
    from . import hipops as H
    with torch.cuda.device(device):
        x = torch.from_numpy(projs).to(device)
        index, dist = H.knn_search(x, x, k, metric="l2", exclude_self=True)
        return index.cpu().numpy(), dist.cpu().numpy()


def tsne_map(projs, perplexity, seed, device):
    """One search with min(N - 1, 3 perplexity + 1) neighbours, then the map: (index, dist) cut to the first `perplexity`
    columns - the strict (distance, index) order makes them the search for that many - y (N, 2) fp32, kl, n_iter."""
    import torch
    from .utils.tsne import TSNE
    with torch.cuda.device(device):
        ts = TSNE(perplexity, seed=seed, device=device)
        x = torch.from_numpy(projs).to(device)
        index, dist = ts.graph(x)
        y = ts.fit_transform(x, graph=(index, dist))
        return (index[:, :perplexity].cpu().numpy(), dist[:, :perplexity].cpu().numpy(), y, ts.kl_divergence_, ts.n_iter_)


def umap_map(projs, n_neighbors, min_dist, seed, device, init="random"):
    """One search with n_neighbors other picks, then the map from its first n_neighbors - 1 columns: index, dist, y (N, 2)
    fp32, n_epochs and the curve parameters a, b; with init="spectral" also (init used, graph components, eigenvalues)."""
    import torch
    from .utils.umap import UMAP
    with torch.cuda.device(device):
        um = UMAP(n_neighbors, min_dist=min_dist, seed=seed, device=device, init=init)
        x = torch.from_numpy(projs).to(device)
        index, dist = um.graph(x)
        y = um.fit_transform(x, graph=(index, dist))
        out = index.cpu().numpy(), dist.cpu().numpy(), y, um.n_epochs_, um.a_, um.b_
        return out if init == "random" else out + ((um.init_, um.n_components_, um.eigenvalues_),)


def umap_label_map(projs, index, dist, label, n_neighbors, min_dist, seed, device, init="random", target_weight=0.5):
    """The label-supervised UMAP map (the reference's fit_transform(projs, y=final_lbs)) from the first n_neighbors - 1 columns
    of a search already made, index and dist (N, >= n_neighbors - 1) numpy: y (N, 2) fp32, n_epochs, a, b, far_dist and
    (init used, graph components, eigenvalues) - the last one None for init="random"."""
    import torch
    from .utils.umap import UMAP
    k = n_neighbors - 1
    with torch.cuda.device(device):
        um = UMAP(n_neighbors, min_dist=min_dist, seed=seed, device=device, init=init, target_weight=target_weight)
        graph = (torch.from_numpy(np.ascontiguousarray(index[:, :k], dtype=np.int32)).to(device),
                 torch.from_numpy(np.ascontiguousarray(dist[:, :k], dtype=np.float32)).to(device))
        y = um.fit_transform(torch.from_numpy(projs).to(device), graph=graph, y=label)
        return y, um.n_epochs_, um.a_, um.b_, um.far_dist_, \
            None if init == "random" else (um.init_, um.n_components_, um.eigenvalues_)


def map_colours(y01, table, device):
    """(N, 3) uint8: the colour of every row of y01 (N, 2) on the (W, H, 3) uint8 table, sampled on the device."""
    import torch
    from .utils.vis3d import sample_colours
    with torch.cuda.device(device):
        return sample_colours(torch.from_numpy(np.ascontiguousarray(y01, dtype=np.float32)).to(device), table).cpu().numpy()


def encoder_threads():
    """Threads of the host-side PNG encoding: OMP_NUM_THREADS where it is set (16 at most), 4 otherwise."""
    try:
        return max(1, min(16, int(os.environ["OMP_NUM_THREADS"])))
    except (KeyError, ValueError):
        return 4


def write_patch_images(subvol, out_dir, device):
    """imgs/{i}.png of every pick as the reference's plt.imsave(patch[0], cmap='gray') writes them: RGBA, R = G = B = the
    grey byte made on the device (utils/plot2d.patch_bytes), A = 255.  The encoding is host work, on a small thread pool."""
    from concurrent.futures import ThreadPoolExecutor
    from .utils import plot2d as P2
    grey = P2.patch_bytes(subvol, device=device)
    os.makedirs(out_dir, exist_ok=True)

    def one(i):
        rgba = np.repeat(grey[i][:, :, None], 4, 2)
        rgba[:, :, 3] = 255
        P2.write_png(os.path.join(out_dir, "%d.png" % i), rgba)

    with ThreadPoolExecutor(max_workers=encoder_threads()) as ex:
        list(ex.map(one, range(len(grey))))
    return len(grey)


def map_picture(y01, subvol, thr, plot_size, device, colours=None, labels=None):
    """The thumbnail selection on the map y01 and its picture, on the device: (shown_idx (n_shown,) int32, picture
    (plot_size, plot_size, 3) uint8), both numpy.  With `colours` (N, 3) the picture is 2d_visualization_out (discs under
    thumbnails), with `labels` (N,) it is 2d_visualization_labels (every thumbnail tagged with its class)."""
    import torch
    from .utils import plot2d as P2
    with torch.cuda.device(device):
        y = torch.from_numpy(np.ascontiguousarray(y01, dtype=np.float32)).to(device)
        idx = P2.select(y, thr)
        shown = idx.cpu().numpy()
        patches = torch.from_numpy(np.ascontiguousarray(subvol[shown], dtype=np.float32)).to(device)
        thumbs = P2.thumbnails(patches, torch.arange(len(shown), dtype=torch.int32, device=device))
        if colours is not None:
            pic = P2.draw_out(y, idx, thumbs, colours, plot_size)
        else:
            pic = P2.draw_labels(y, idx, thumbs, labels, plot_size)
        return shown, pic.cpu().numpy()


def write_picture(stem, pic):
    """stem.png always; stem.webp (lossless: the reference's own file name) where PIL with WebP support imports."""
    from .utils.plot2d import write_png
    write_png(stem + ".png", pic)
    try:
        from PIL import Image, features
        if not features.check("webp"):
            raise ImportError("PIL without WebP support")
        Image.fromarray(pic).save(stem + ".webp", lossless=True)
        return True
    except Exception as e:                                 # nothing may fail for lack of PIL: the PNG is written
        print("[cet_pick_amd] plot_2d: %s.webp left out (%s); %s.png holds the same picture" % (stem, e, stem))
        return False


def write_class_gallery(path, patches, projs, centroids, assign, label, n_classes, m, device):
    """class_gallery.npz (mean, std, count, exemplar_index, exemplar_d2, order) and class_gallery.png (.webp) under `path`: the
    classes of `label` as a gallery, made on the device (utils/plot2d.class_gallery)."""
    from .utils.plot2d import class_gallery
    g = class_gallery(patches, projs, np.asarray(centroids, np.float32), assign, label, n_classes, m=m, device=device)
    pic = g.pop("picture")
    np.savez(os.path.join(path, "class_gallery.npz"), **g)
    write_picture(os.path.join(path, "class_gallery"), pic)
    print("[cet_pick_amd] plot_2d: gallery of %d classes (%d with members), %d exemplars each, %d x %d -> %s and class_gallery.npz"
          % (n_classes, int((g["count"] > 0).sum()), m, pic.shape[1], pic.shape[0], os.path.join(path, "class_gallery.png")))


def quality_plan(args, n):
    """The checks of --quality, --sweep_n_cluster and --compare_labels that need no device: (sweep list or None, the labels to
    compare with or None), or None where none of the three flags is given."""
    if not (args.quality or args.sweep_n_cluster is not None or args.compare_labels is not None):
        return None
    from .utils.cluster_quality import parse_sweep
    sweep = None
    if args.sweep_n_cluster is not None:
        sweep = parse_sweep(args.sweep_n_cluster)
        if max(sweep) >= args.k:
            raise ValueError("--sweep_n_cluster merges the %d centroids into fewer classes, got %d" % (args.k, max(sweep)))
    other = None
    if args.compare_labels is not None:
        held = np.load(args.compare_labels)
        if "label" not in held.files:
            raise ValueError("--compare_labels %s holds no 'label' (it has %s)" % (args.compare_labels, ", ".join(held.files)))
        other = np.asarray(held["label"]).ravel()
        if len(other) != n:
            raise ValueError("--compare_labels %s labels %d picks, the input has %d" % (args.compare_labels, len(other), n))
    return sweep, other


def write_quality(path, projs, assign, label, class_of, centroids, k, plan, device):
    """cluster_quality.npz under `path` (the module docstring lists its keys) and its stdout lines: one pass over the pairs of
    picks on the device (utils/cluster_quality.SilhouetteSums) serves the final classes, the k-means assignment
    and every class count of the sweep."""
    import torch
    from .utils.cluster_quality import SilhouetteSums, compare_labelings
    sweep, other = plan
    with torch.cuda.device(device):
        sums = SilhouetteSums(projs, assign, k, device=device)
        fine = sums.score()
        final = fine if class_of is None else sums.score(class_of)
        out = dict(final.arrays(), **fine.arrays("fine_"))
        print("[cet_pick_amd] plot_2d: mean silhouette %.6f over the %d final classes, %.6f over the k-means assignment (%d "
              "clusters with members) -> %s" % (final.mean, int((final.class_count > 0).sum()), fine.mean,
                                                int((fine.class_count > 0).sum()), os.path.join(path, "cluster_quality.npz")))
        if sweep is not None:
            rows = []
            for v in sweep:
                r = sums.score(merge_centroids(centroids, v))
                rows.append((v, r.mean, float(np.nanmin(r.class_mean)), int(r.class_count[r.class_count > 0].min())))
            out.update(sweep_n_cluster=np.asarray([r[0] for r in rows], np.int32), sweep_mean=np.asarray([r[1] for r in rows]),
                       sweep_min_class_mean=np.asarray([r[2] for r in rows]),
                       sweep_smallest_class=np.asarray([r[3] for r in rows], np.int32))
            print("[cet_pick_amd] plot_2d: n_cluster  mean silhouette  lowest class mean  smallest class")
            for r in rows:
                print("[cet_pick_amd] plot_2d: %9d  %15.6f  %17.6f  %14d" % r)
        if other is not None:
            cmp = compare_labelings(label, other, device=device)
            out.update(compare_table=cmp.table, compare_ari=np.float64(cmp.ari), compare_nmi=np.float64(cmp.nmi),
                       compare_ids=cmp.ids_a, compare_ids_other=cmp.ids_b)
            print("[cet_pick_amd] plot_2d: against the other labels: %d x %d classes, adjusted Rand index %.6f, normalised mutual "
                  "information %.6f" % (cmp.table.shape[0], cmp.table.shape[1], cmp.ari, cmp.nmi))
    np.savez(os.path.join(path, "cluster_quality.npz"), **out)


def unit_square(y):
    """(y - min) / (max - min) per axis, as the reference normalises its map (an axis of one value maps to 0)."""
    lo, hi = y.min(0), y.max(0)
    return ((y - lo) / np.where(hi > lo, hi - lo, 1)).astype(np.float32)


def main(args):
    gpu = int(str(args.gpus).split(",")[0])
    if gpu < 0:
        raise RuntimeError("the MI355X path has no CPU mode (--gpus -1)")
    import torch
    from .utils.kmeans import Kmeans
    data = np.load(args.input)
    projs = np.ascontiguousarray(data["pred"], dtype=np.float32)
    projs = projs.reshape(projs.shape[0], -1)
    names, coords = data["name"], data["coords"]
    with_tsne = args.mode == "tsne" and args.num_neighbor is not None
    # the bare default is "umap" as well, and keeps writing no map (the module docstring says why); to change that, drop the
    # isinstance test
    with_umap = args.mode == "umap" and not isinstance(args.mode, DefaultMode) and args.num_neighbor is not None
    with_map = with_tsne or with_umap
    if with_map:
        from .utils.vis3d import load_colormap
        if with_umap:
            from .utils.umap import check_range
        else:
            from .utils.tsne import check_range
        check_range(len(projs), args.num_neighbor)
        table = load_colormap(args.colormap)
    if args.label_map:
        if args.num_neighbor is None:
            raise ValueError("--label_map needs --num_neighbor K: the label-supervised map is a UMAP map with n_neighbors K")
        from .utils.umap import check_range as check_umap_range, check_target_weight
        check_umap_range(len(projs), args.num_neighbor)
        check_target_weight(args.target_weight)
    with_vis = args.min_dist_vis is not None
    if with_vis:
        if args.plot_size < 128:
            raise ValueError("--plot_size is at least 128, got %d" % args.plot_size)
        if "subvol" not in data.files:
            raise ValueError("--min_dist_vis draws the picks' patches: %s holds no 'subvol' (it has %s)"
                             % (args.input, ", ".join(data.files)))
        subvol = np.asarray(data["subvol"], dtype=np.float32)
        if subvol.ndim != 4 or len(subvol) != len(projs) or subvol.shape[2] != subvol.shape[3]:
            raise ValueError("'subvol' of %s must be (%d, C, b, b), got %s" % (args.input, len(projs), subvol.shape))
        thr = np.float32(args.min_dist_vis)
        pictures = (["2d_visualization_out.png"] if with_map else []) + (
            ["2d_visualization_labels.png"] if args.label_map and args.num_neighbor is not None else [])
        print("[cet_pick_amd] plot_2d: --min_dist_vis %g writes %s%s" % (
            args.min_dist_vis, "imgs/{i}.png of %d picks" % len(projs) if args.save_out_img == 1 else "no imgs/ (--save_out_img "
            "%d)" % args.save_out_img, (", " + ", ".join(pictures) + " (%d x %d) and plot_2d_shown.npz" % (args.plot_size,
            args.plot_size)) if pictures else " only: without a map (--mode umap | tsne with --num_neighbor K) there is no picture"))
    if args.class_gallery:
        if "subvol" not in data.files:
            raise ValueError("--class_gallery averages the picks' patches: %s holds no 'subvol' (it has %s)"
                             % (args.input, ", ".join(data.files)))
        if not 1 <= args.gallery_exemplars <= 64:
            raise ValueError("--gallery_exemplars is 1..64, got %d" % args.gallery_exemplars)
        gallery_patches = np.asarray(data["subvol"])
        if gallery_patches.ndim != 4 or len(gallery_patches) != len(projs) or 0 in gallery_patches.shape:
            raise ValueError("'subvol' of %s must be (%d, C, h, w), got %s" % (args.input, len(projs), gallery_patches.shape))
        gallery_patches = np.ascontiguousarray(gallery_patches[:, 0], dtype=np.float32)       # channel 0, as the pictures show it
    quality = quality_plan(args, len(projs))
    if with_vis:
        pass                                               # the line above says what is written
    elif with_umap:
        print("[cet_pick_amd] plot_2d: the plots and thumbnails are not made here (--min_dist_vis, --save_out_img are ignored); "
              "--mode umap --num_neighbor %d writes the neighbour graph knn_graph.npz, the UMAP map embeddings_2d.npz (min_dist "
              "%g) and its colours all_colors.npy" % (args.num_neighbor, args.min_dist_umap))
    elif with_tsne:
        print("[cet_pick_amd] plot_2d: the plots and thumbnails are not made here (--min_dist_umap, --min_dist_vis, "
              "--save_out_img are ignored); --mode tsne --num_neighbor %d writes the neighbour graph knn_graph.npz, the "
              "t-SNE map embeddings_2d.npz and its colours all_colors.npy" % args.num_neighbor)
    elif args.num_neighbor is None:
        print("[cet_pick_amd] plot_2d: the 2-D plots, thumbnails and colour map are not made here (--num_neighbor, --mode, "
              "--min_dist_umap, --min_dist_vis, --save_out_img are ignored)")
    else:
        print("[cet_pick_amd] plot_2d: the 2-D plots, thumbnails and colour map are not made here (--mode, --min_dist_umap, "
              "--min_dist_vis, --save_out_img are ignored); --num_neighbor %d writes the neighbour graph knn_graph.npz"
              % args.num_neighbor)
    os.makedirs(args.path, exist_ok=True)
    km = Kmeans(projs.shape[1], args.k, niter=args.niter, seed=args.seed, device=torch.device("cuda", gpu))
    with torch.cuda.device(gpu):
        km.train(projs)
        D, I = km.assign(projs)
    assign = I[:, 0].astype(np.int32)
    centroids = km.centroids
    class_of = None                                        # of every centroid, where --n_cluster merges
    if 0 < args.n_cluster < args.k:
        y = class_of = merge_centroids(centroids, args.n_cluster)
        print("Actual number of clusters is:", len(set(y.tolist())))
        label = y[assign].astype(np.int32)
    else:
        label = assign.copy()
    np.savez(os.path.join(args.path, "kmeans_labels.npz"), centroids=centroids, assign=assign, dist=D[:, 0].astype(np.float32),
             label=label, obj=km.obj.astype(np.float32), name=names, coords=coords)
    write_parquet(os.path.join(args.path, "interactive_info_parquet.gzip"), names, coords, projs, label, args.host)
    if with_vis and args.save_out_img == 1:
        n_img = write_patch_images(subvol, os.path.join(args.path, "imgs"), torch.device("cuda", gpu))
        print("[cet_pick_amd] plot_2d: %d grey PNGs -> %s" % (n_img, os.path.join(args.path, "imgs")))
    print("[cet_pick_amd] plot_2d: %d picks, %d centroids, %d classes, objective %.6g -> %s"
          % (len(assign), args.k, len(set(label.tolist())), float(km.obj[-1]) if len(km.obj) else float("nan"), args.path))
    if args.class_gallery:
        n_classes = args.n_cluster if 0 < args.n_cluster < args.k else args.k      # the final labels: merged classes, or centroids
        write_class_gallery(args.path, gallery_patches, projs, centroids, assign, label, n_classes, args.gallery_exemplars,
                            torch.device("cuda", gpu))
    if quality is not None:
        write_quality(args.path, projs, assign, label, class_of, centroids, args.k, quality, torch.device("cuda", gpu))
    if args.num_neighbor is not None:
        if with_umap:
            if args.umap_init == "spectral":
                index, dist, y, n_epochs, a, b, (init_used, n_comp, eigenvalues) = umap_map(
                    projs, args.num_neighbor, args.min_dist_umap, args.map_seed, torch.device("cuda", gpu), init="spectral")
                start = dict(init=np.array(init_used), n_graph_components=np.int32(n_comp),
                             eigenvalues=np.asarray([] if eigenvalues is None else eigenvalues, np.float64))
            else:
                index, dist, y, n_epochs, a, b = umap_map(projs, args.num_neighbor, args.min_dist_umap, args.map_seed,
                                                          torch.device("cuda", gpu))
                start = {}
        elif with_tsne:
            index, dist, y, kl, n_iter = tsne_map(projs, args.num_neighbor, args.map_seed, torch.device("cuda", gpu))
        else:
            index, dist = knn_graph(projs, args.num_neighbor, torch.device("cuda", gpu))
        np.savez(os.path.join(args.path, "knn_graph.npz"), index=index, dist=dist, k=np.int32(args.num_neighbor))
        print("[cet_pick_amd] plot_2d: %d nearest neighbours of %d picks (squared L2, self excluded) -> %s"
              % (args.num_neighbor, len(index), os.path.join(args.path, "knn_graph.npz")))
    shown_sets = {}
    if args.label_map:
        ys, n_epochs_s, a_s, b_s, far, start_s = umap_label_map(
            projs, index, dist, label, args.num_neighbor, args.min_dist_umap, args.map_seed, torch.device("cuda", gpu),
            init=args.umap_init, target_weight=args.target_weight)
        ys = np.asarray(ys, np.float32)
        start_s = {} if start_s is None else dict(
            init=np.array(start_s[0]), n_graph_components=np.int32(start_s[1]),
            eigenvalues=np.asarray([] if start_s[2] is None else start_s[2], np.float64))
        np.savez(os.path.join(args.path, "embeddings_2d_labels.npz"), y=ys, y01=unit_square(ys), label=label,
                 n_epochs=np.int32(n_epochs_s), n_neighbors=np.int32(args.num_neighbor), min_dist=np.float32(args.min_dist_umap),
                 a=np.float64(a_s), b=np.float64(b_s), seed=np.int32(args.map_seed), target_weight=np.float64(args.target_weight),
                 far_dist=np.float64(far), **start_s)
        print("[cet_pick_amd] plot_2d: label-supervised UMAP map of %d picks in %d classes, n_neighbors %d, min_dist %g, "
              "target_weight %g, %d epochs%s -> %s"
              % (len(ys), len(set(label.tolist())), args.num_neighbor, args.min_dist_umap, args.target_weight, n_epochs_s,
                 ", start %s" % start_s["init"] if start_s else "", os.path.join(args.path, "embeddings_2d_labels.npz")))
        if with_vis:
            shown_l, pic = map_picture(unit_square(ys), subvol, thr, args.plot_size, torch.device("cuda", gpu), labels=label)
            write_picture(os.path.join(args.path, "2d_visualization_labels"), pic)
            shown_sets["shown_idx_labels"] = shown_l
            print("[cet_pick_amd] plot_2d: %d of %d picks shown with their class -> %s"
                  % (len(shown_l), len(ys), os.path.join(args.path, "2d_visualization_labels.png")))
    if with_map:
        y = np.asarray(y, np.float32)
        y01 = unit_square(y)
        if with_umap:
            np.savez(os.path.join(args.path, "embeddings_2d.npz"), y=y, y01=y01, n_epochs=np.int32(n_epochs),
                     n_neighbors=np.int32(args.num_neighbor), min_dist=np.float32(args.min_dist_umap), a=np.float64(a),
                     b=np.float64(b), seed=np.int32(args.map_seed), **start)
            if start:
                print("[cet_pick_amd] plot_2d: UMAP start %s (--umap_init spectral), %d graph components" % (init_used, n_comp))
            print("[cet_pick_amd] plot_2d: UMAP map of %d picks, n_neighbors %d, min_dist %g, %d epochs -> %s"
                  % (len(y), args.num_neighbor, args.min_dist_umap, n_epochs, os.path.join(args.path, "embeddings_2d.npz")))
        else:
            np.savez(os.path.join(args.path, "embeddings_2d.npz"), y=y, y01=y01, kl=np.float32(kl), n_iter=np.int32(n_iter),
                     perplexity=np.int32(args.num_neighbor), seed=np.int32(args.map_seed))
            print("[cet_pick_amd] plot_2d: t-SNE map of %d picks, perplexity %d, %d iterations, KL %.6g -> %s"
                  % (len(y), args.num_neighbor, n_iter, kl, os.path.join(args.path, "embeddings_2d.npz")))
        if not torch.cuda.is_available():
            # only reached when every device step in front of this one was replaced (tests/test_tsne_cpu.py drives main with
            # stubs for the clustering, the search and the map): the sampler is a kernel, and there is no host form of it
            print("[cet_pick_amd] plot_2d: all_colors.npy left out: no MI355X (cuda) device for the colour sampler")
            return
        colours = map_colours(y01, table, torch.device("cuda", gpu))
        np.save(os.path.join(args.path, "all_colors.npy"), colours)
        print("[cet_pick_amd] plot_2d: colours of %d picks on the %d x %d table%s -> %s"
              % (len(y), table.shape[0], table.shape[1], "" if args.colormap else " (built in, not the reference's)",
                 os.path.join(args.path, "all_colors.npy")))
        if with_vis:
            shown, pic = map_picture(y01, subvol, thr, args.plot_size, torch.device("cuda", gpu), colours=colours)
            write_picture(os.path.join(args.path, "2d_visualization_out"), pic)
            shown_sets["shown_idx"] = shown
            print("[cet_pick_amd] plot_2d: %d of %d picks shown over their colours -> %s"
                  % (len(shown), len(y), os.path.join(args.path, "2d_visualization_out.png")))
    if shown_sets:
        from .utils.plot2d import THUMB
        np.savez(os.path.join(args.path, "plot_2d_shown.npz"), min_dist_vis=thr, plot_size=np.int32(args.plot_size),
                 thumb=np.int32(THUMB), **shown_sets)


if __name__ == "__main__":
    main(add_arguments(argparse.ArgumentParser("cluster exploration embeddings into classes")).parse_args())
