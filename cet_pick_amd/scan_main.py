"""Learn pick classes from the neighbour graph: the SCAN step of the reference in its head-only form (`--cluster_head`) on the
stored exploration embeddings (utils/scan.py, csrc/scan_loss.hip):

    python -m cet_pick_amd.scan_main --input exp/.../all_output_info.npz --path OUT --nclusters 10 [--nheads 1]
                                     [--num_neighbor 20] [--graph OUT/knn_graph.npz] [--num_epochs 100] [--batch_size 1024]
                                     [--lr 1e-3] [--weight_decay 1e-4] [--entropy_weight 2.0] [--seed 317] [--min_conf 0]
                                     [--load_model OUT/scan_heads.pth] [--gpus 0]

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

The optimiser defaults (Adam, lr 1e-3, weight decay 1e-4, 100 epochs, batch 1024) are the reference's SCAN settings and are
unmeasured on real data here.  Not made: the backbone-in-the-loop `scan` / `scan2d3d` tasks and SCAN's self-labelling step.
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
    data = np.load(args.input)
    projs = np.ascontiguousarray(data["pred"], dtype=np.float32)
    projs = projs.reshape(projs.shape[0], -1)
    names, coords = data["name"], data["coords"]
    n = len(projs)
    index = load_graph(args.graph, n) if args.graph and not args.load_model else None
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
        heads.save(os.path.join(args.path, "scan_heads.pth"))
    label, conf, counts, prob = heads.predict(projs, with_prob=True)
    head, c = heads.best_loss_head, heads.nclusters
    out = labels_file(names, coords, label, conf, head, counts, stats, prob[:, head * c:(head + 1) * c], args.min_conf)
    np.savez(os.path.join(args.path, "scan_labels.npz"), **out)
    print("[cet_pick_amd] scan_main: %d picks, head %d of %d, %d below --min_conf %g; picks per class: %s -> %s"
          % (n, head, heads.nheads, int((out["label"] < 0).sum()), args.min_conf, " ".join(str(int(v)) for v in counts[head]),
             os.path.join(args.path, "scan_labels.npz")))
    return out


if __name__ == "__main__":
    main(add_arguments(argparse.ArgumentParser("SCAN heads on the exploration embeddings")).parse_args())
