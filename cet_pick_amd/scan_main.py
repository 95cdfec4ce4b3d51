"""Learn pick classes from the neighbour graph: the SCAN step of the reference in its head-only form (`--cluster_head`) on the
stored exploration embeddings (utils/scan.py, csrc/scan_loss.hip):

    python -m cet_pick_amd.scan_main --input exp/.../all_output_info.npz --path OUT --nclusters 10 [--nheads 1]
                                     [--num_neighbor 20] [--graph OUT/knn_graph.npz] [--num_epochs 100] [--batch_size 1024]
                                     [--lr 1e-3] [--weight_decay 1e-4] [--entropy_weight 2.0] [--seed 317] [--min_conf 0]
                                     [--load_model OUT/scan_heads.pth] [--gpus 0] [--select_head epoch|graph]
                                     [--selflabel_epochs 0] [--selflabel_threshold 0.99] [--selflabel_lr 1e-4]
                                     [--no_class_balancing] [--quality]

--nheads linear heads on the rows of `pred` are trained so that a pick and a random one of [itself, its --num_neighbor graph
neighbours] get the same class while the classes stay balanced.  --graph takes the `index` of a knn_graph.npz that plot_2d wrote
(all its columns; a wrong row count is refused); without it the graph is searched as plot_2d does (squared L2 over `pred`, the
pick itself excluded).  --load_model classifies with stored heads and trains nothing.

    OUT/scan_heads.pth      epoch, state_dict (cluster_head.{h}.weight, .bias: the reference's names), optimizer, best_loss,
                            best_loss_head - the reference's save_model_scan layout
    OUT/scan_labels.npz     name, coords; label (N,) i32: the class the best head (lowest mean total loss of the last epoch) gives
                            every pick, -1 where its probability is below --min_conf; conf (N,) f32 that probability; head: the
                            best head; counts (nheads, nclusters) i32: picks per class and head; stats (nheads, 3) f32: total,
                            consistency, entropy per head, the mean over the last epoch's batches (with --load_model: the stored
                            best loss, NaN elsewhere); prob (N, nclusters) f32 of the best head.  interactive_to_training_coords --input OUT/scan_labels.npz --labels ... reads it.

--select_head graph chooses the best head as the reference's scan_evaluate does (csrc/scan_selflabel.hip): every
head is scored on every pick against all entries of [itself, its graph neighbours] under the final weights, total = consistency
- entropy, and `stats` holds these figures for every head; also with --load_model (which then needs --graph or searches).  The
default, epoch, is the lowest mean training loss of the last epoch.

--selflabel_epochs E > 0 adds SCAN's third step: the best head alone is trained on with the confidence-based cross-entropy (a
pick whose class probability exceeds --selflabel_threshold is its own label; the graph-neighbour draw stands in for the strong
view; classes weighted by their inverse share unless --no_class_balancing; Adam, --selflabel_lr, --weight_decay).  With
--load_model the stored best head is self-labelled and nothing is clustered.  scan_heads.pth and scan_labels.npz are the
clustering step's, as without the flag; in addition

    OUT/scan_heads_selflabel.pth   the same layout with the one head (cluster_head.0.*): --load_model reads it with --nheads 1
    OUT/scan_labels_selflabel.npz  the keys of scan_labels.npz from that head (head 0; stats: its graph figures), and
                                   selflabel_stats (E, 3) f32: per epoch the mean loss, the share of confident picks, the mean
                                   number of classes present in a batch

--quality (this project's own) scores the classes of every head by their exact silhouette over `pred`
(utils/cluster_quality.py, csrc/cluster_quality.hip); also with --load_model.  `stats` of scan_labels.npz then has a fourth column,
the mean silhouette of every head (NaN for a head that leaves fewer than two classes with members), and

    OUT/scan_quality.npz    of the best head: head; s, a, b (N,) f64 and nearest (N,) i32 per pick (a: mean distance to the own
                            class, b: to the nearest other class, s = (b - a) / max(a, b)); class_mean (C,) f64 (NaN: no member),
                            class_count (C,) i32, mean, confusion (C, C) i32 [own][nearest] - the classes BEFORE --min_conf

The optimiser defaults (Adam, lr 1e-3, weight decay 1e-4, 100 epochs, batch 1024) are the reference's SCAN settings, and
--selflabel_threshold 0.99 and --selflabel_lr 1e-4 are SCAN's published self-labelling settings; all are unmeasured on real data
here.  Not made: the backbone-in-the-loop `scan` / `scan2d3d` tasks (with them the image augmentation of the strong view).
"""
import argparse
import os

import numpy as np


def add_arguments(parser):
    parser.add_argument("--input", required=True, help="all_output_info.npz of the exploration inference (pred, name, coords)")
    parser.add_argument("--path", required=True, help="output directory")
    parser.add_argument("--nclusters", type=int, required=True, help="classes per head, 1..64")
    parser.add_argument("--nheads", type=int, default=1, help="heads trained side by side, 1..16; the one with the lowest loss labels")
    parser.add_argument("--num_neighbor", type=int, default=20, help="graph neighbours per pick when the graph is searched here")
    parser.add_argument("--graph", default=None, help="knn_graph.npz of plot_2d: use its index instead of searching")
    parser.add_argument("--num_epochs", type=int, default=100)
    parser.add_argument("--batch_size", type=int, default=1024, help="pairs per step; clipped to the number of picks")
    parser.add_argument("--lr", type=float, default=1e-3)
    parser.add_argument("--weight_decay", type=float, default=1e-4)
    parser.add_argument("--entropy_weight", type=float, default=2.0, help="weight of the class-balance term (the reference: 2.0)")
    parser.add_argument("--seed", type=int, default=317, help="seed of the heads' start and of the neighbour draws")
    parser.add_argument("--min_conf", type=float, default=0.0, help="picks whose class probability is below this get label -1")
    parser.add_argument("--load_model", default=None, help="scan_heads.pth: classify only")
    parser.add_argument("--gpus", default="0", help="GPU index; -1 (CPU) is refused")
    parser.add_argument("--select_head", choices=("epoch", "graph"), default="epoch",
                        help="best head: lowest mean loss of the last epoch, or lowest total over the whole graph (scan_evaluate)")
    parser.add_argument("--selflabel_epochs", type=int, default=0, help="self-labelling epochs on the best head; 0: none")
    parser.add_argument("--selflabel_threshold", type=float, default=0.99,
                        help="a pick above this class probability labels itself, in [0, 1) (SCAN's 0.99; unmeasured on real data)")
    parser.add_argument("--selflabel_lr", type=float, default=1e-4, help="Adam's rate of the self-labelling (SCAN's 1e-4; unmeasured)")
    parser.add_argument("--no_class_balancing", action="store_true", help="self-labelling without the inverse-share class weights")
    parser.add_argument("--quality", action="store_true", help="also score every head's classes by their exact silhouette over "
                        "`pred`: a fourth column of stats, and scan_quality.npz for the best head")
    return parser


def load_graph(path, n):
    index = np.asarray(np.load(path)["index"])
    if index.ndim != 2 or index.shape[0] != n:
        raise ValueError("--graph %s has an index of shape %s, the input has %d picks" % (path, index.shape, n))
    if index.size and (index.min() < 0 or index.max() >= n):
        raise ValueError("--graph %s names a pick outside 0..%d" % (path, n - 1))
    return index.astype(np.int32)


def search_graph(projs, k, device):
    from .plot_2d import knn_graph
    if not 1 <= k <= len(projs) - 1:
        raise ValueError("--num_neighbor must be in 1..%d (the other picks), got %d" % (len(projs) - 1, k))
    return knn_graph(projs, k, device)[0]


def labels_file(names, coords, label, conf, head, counts, stats, prob, min_conf):
    """The arrays of scan_labels.npz: label and conf are the best head's columns; a pick below min_conf gets -1."""
    best_label = np.where(conf[:, head] < np.float32(min_conf), -1, label[:, head]).astype(np.int32)
    return dict(name=names, coords=coords, label=best_label, conf=conf[:, head].astype(np.float32), head=np.int32(head),
                counts=counts.astype(np.int32), stats=np.asarray(stats, np.float32), prob=prob.astype(np.float32))


def main(args):
    gpu = int(str(args.gpus).split(",")[0])
    if gpu < 0:
        raise RuntimeError("the MI355X path has no CPU mode (--gpus -1)")
    from .utils import scan as S
    S.check_sizes(args.nclusters, args.nheads)
    if args.selflabel_epochs < 0:
        raise ValueError("--selflabel_epochs must be >= 0, got %d" % args.selflabel_epochs)
    if not 0.0 <= args.selflabel_threshold < 1.0:
        raise ValueError("--selflabel_threshold must be in [0, 1), got %g" % args.selflabel_threshold)
    data = np.load(args.input)
    projs = np.ascontiguousarray(data["pred"], dtype=np.float32)
    projs = projs.reshape(projs.shape[0], -1)
    names, coords = data["name"], data["coords"]
    n = len(projs)
    by_graph, selflabel = args.select_head == "graph", args.selflabel_epochs > 0
    need_graph = not args.load_model or by_graph or selflabel
    index = load_graph(args.graph, n) if args.graph and need_graph else None
    import torch
    device = torch.device("cuda", gpu)
    os.makedirs(args.path, exist_ok=True)
    if args.load_model:
        heads = S.ScanHeads.load(args.load_model, device=device)
        if (heads.d, heads.nclusters, heads.nheads) != (projs.shape[1], args.nclusters, args.nheads):
            raise ValueError("--load_model %s holds %d heads of %d classes on %d-dimensional embeddings; asked for %d heads of %d "
                             "classes on %d" % (args.load_model, heads.nheads, heads.nclusters, heads.d, args.nheads,
                                                args.nclusters, projs.shape[1]))
        stats = np.full((heads.nheads, 3), np.nan, np.float32)
        stats[heads.best_loss_head, 0] = heads.best_loss
        print("[cet_pick_amd] scan_main: %s: %d heads of %d classes after %d epochs, best head %d (loss %.6g); classifying %d picks"
              % (args.load_model, heads.nheads, heads.nclusters, heads.epoch, heads.best_loss_head, heads.best_loss, n))
        if index is None and need_graph:
            index = search_graph(projs, args.num_neighbor, device)
    else:
        batch_size = args.batch_size
        if batch_size > n:
            print("[cet_pick_amd] scan_main: --batch_size %d clipped to the %d picks" % (batch_size, n))
            batch_size = n
        if index is None:
            index = search_graph(projs, args.num_neighbor, device)
        heads = S.ScanHeads(projs.shape[1], args.nclusters, args.nheads, seed=args.seed, device=device)

        def log(epoch, mean):
            print("[cet_pick_amd] scan_main: epoch %d: %s" % (epoch, "  ".join(
                "head %d total %.5f consistency %.5f entropy %.5f" % (h, m[0], m[1], m[2]) for h, m in enumerate(mean))))

        history = heads.fit(projs, index, num_epochs=args.num_epochs, batch_size=batch_size, lr=args.lr,
                            weight_decay=args.weight_decay, entropy_weight=args.entropy_weight, log=log)
        stats = history[-1]
    if by_graph:
        stats = graph_stats(heads, projs, index)
    if not args.load_model:
        heads.save(os.path.join(args.path, "scan_heads.pth"))
    if args.quality:
        stats = head_quality(args, heads, projs, stats, device)
    out = write_labels(args, heads, projs, names, coords, stats, "scan_labels.npz")
    if selflabel:
        def log_selflabel(epoch, mean):
            print("[cet_pick_amd] scan_main: self-label epoch %d: loss %.5f confident %.4f classes present %.2f"
                  % (epoch, mean[0], mean[1], mean[2]))

        one, sl_stats = heads.selflabel(projs, index, heads.best_loss_head, num_epochs=args.selflabel_epochs,
                                        batch_size=min(args.batch_size, n), lr=args.selflabel_lr, threshold=args.selflabel_threshold,
                                        balance=not args.no_class_balancing, log=log_selflabel, weight_decay=args.weight_decay)
        stats = graph_stats(one, projs, index)             # (best_loss of the checkpoint: this head's total over the graph)
        one.save(os.path.join(args.path, "scan_heads_selflabel.pth"))
        write_labels(args, one, projs, names, coords, stats, "scan_labels_selflabel.npz", selflabel_stats=sl_stats.astype(np.float32))
    return out


def graph_stats(heads, projs, index):
    stats = heads.evaluate(projs, index)
    print("[cet_pick_amd] scan_main: over the graph: %s; best head %d" % ("  ".join(
        "head %d total %.5f consistency %.5f entropy %.5f" % (h, m[0], m[1], m[2]) for h, m in enumerate(stats)), heads.best_loss_head))
    return stats


def head_quality(args, heads, projs, stats, device):
    """--quality: the exact silhouette (utils/cluster_quality.py) of every head's classes over the embeddings;
    -> stats with the per-head mean as a fourth column (NaN for a head that leaves fewer than two classes with members); the
    best head's full record goes to scan_quality.npz."""
    from .utils.cluster_quality import silhouette
    label = heads.predict(projs)[0]
    means = np.full((heads.nheads, 1), np.nan, np.float32)
    for h in range(heads.nheads):
        try:
            q = silhouette(projs, label[:, h], device=device)
        except ValueError as e:
            print("[cet_pick_amd] scan_main: head %d has no silhouette: %s" % (h, e))
            continue
        means[h, 0] = q.mean
        if h == heads.best_loss_head:
            np.savez(os.path.join(args.path, "scan_quality.npz"), head=np.int32(h), **q.arrays())
    print("[cet_pick_amd] scan_main: mean silhouette per head: %s; best head %d -> %s" % (
        " ".join("%.6f" % v for v in means[:, 0]), heads.best_loss_head, os.path.join(args.path, "scan_quality.npz")))
    return np.concatenate([np.asarray(stats, np.float32).reshape(heads.nheads, -1), means], axis=1)


def write_labels(args, heads, projs, names, coords, stats, file_name, **more):
    label, conf, counts, prob = heads.predict(projs, with_prob=True)
    head, c = heads.best_loss_head, heads.nclusters
    out = labels_file(names, coords, label, conf, head, counts, stats, prob[:, head * c:(head + 1) * c], args.min_conf)
    np.savez(os.path.join(args.path, file_name), **out, **more)
    print("[cet_pick_amd] scan_main: %d picks, head %d of %d, %d below --min_conf %g; picks per class: %s -> %s"
          % (len(projs), head, heads.nheads, int((out["label"] < 0).sum()), args.min_conf,
             " ".join(str(int(v)) for v in counts[head]), os.path.join(args.path, file_name)))
    return out


if __name__ == "__main__":
    main(add_arguments(argparse.ArgumentParser("SCAN heads on the exploration embeddings")).parse_args())
