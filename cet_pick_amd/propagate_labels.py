"""From a few hand-labelled examples to every similar pick: label spreading over the neighbour graph of the exploration embeddings
(this project's stand-in for selecting picks by hand on the map of the reference's interactive session; utils/label_spread.py,
csrc/label_spread.hip):

    python -m cet_pick_amd.propagate_labels --input exp/.../all_output_info.npz --path OUT
                                            (--seeds seeds.txt | --seed_index seeds.npz)
                                            [--graph OUT/knn_graph.npz | --num_neighbor 15] [--edge_weight gauss] [--alpha 0.9]
                                            [--tol 1e-6] [--max_iter 1000] [--seed_radius 8] [--if_double] [--min_conf 0.5] [--gpus 0]

--seeds is the tab-separated table of training_coordinates.txt (image_name x_coord y_coord z_coord, the header optional) with an
optional fifth column `class`: integers >= 0, class 0 for every seed without the column.  Each seed is matched to the nearest pick
of its tomogram within --seed_radius (on the GPU); --if_double halves the seeds' z first, the inverse of what
interactive_to_training_coords --if_double does.  --seed_index names the picks directly: an npz with index (M,) and class (M,).
At least two classes must end up with a matched seed: with one class every reachable pick has confidence 1 and no threshold
separates anything, so give counter-examples (junk, membrane, gold) a class of their own.

--graph takes index and dist of a knn_graph.npz that plot_2d wrote (a graph without dist only with --edge_weight binary); without
it the --num_neighbor nearest other picks are searched here, as scan_main does.  The seeds' classes are spread with
F <- alpha S F + (1 - alpha) Y (Zhou et al. 2004; S the symmetric, degree-normalised graph) until the largest change is at most
--tol or --max_iter sweeps have run.

    OUT/propagated_labels.npz   name, coords; label (N,) i32: the class with the largest score, -1 where no seed reaches the pick or
                                its confidence is below --min_conf; conf (N,) f32 = that score over mass; mass (N,) f32 = the sum
                                of the pick's scores; score (N, C) f32 = F; seed_pick, seed_class, seed_dist: per seed the matched
                                pick (-1: none), its class and its distance; n_iter, residual, alpha, edge_weight; seed_flipped:
                                the matched seeds whose final label is not their own (the scheme clamps softly).
                                interactive_to_training_coords --input OUT/propagated_labels.npz --labels 0 reads it.

alpha 0.9 and tol 1e-6 are unmeasured on real data here.  Not made: hard clamping of the seeds, other kernels than the two edge
weights, ranking by one class alone.
"""
import argparse
import os

import numpy as np


def add_arguments(parser):
    parser.add_argument("--input", required=True, help="all_output_info.npz of the exploration inference (pred, name, coords)")
    parser.add_argument("--path", required=True, help="output directory")
    parser.add_argument("--seeds", default=None, help="seed table: image_name x_coord y_coord z_coord [class], tab-separated")
    parser.add_argument("--seed_index", default=None, help="npz with index (M,) and class (M,): the seeds as pick numbers")
    parser.add_argument("--graph", default=None, help="knn_graph.npz of plot_2d: use its index and dist instead of searching")
    parser.add_argument("--num_neighbor", type=int, default=15, help="graph neighbours per pick when the graph is searched here")
    parser.add_argument("--edge_weight", choices=("gauss", "binary"), default="gauss")
    parser.add_argument("--alpha", type=float, default=0.9, help="share a pick takes from its neighbours per sweep, in (0, 1)")
    parser.add_argument("--tol", type=float, default=1e-6, help="stop when no score changes by more than this")
    parser.add_argument("--max_iter", type=int, default=1000)
    parser.add_argument("--seed_radius", type=float, default=8.0, help="a seed matches the nearest pick of its tomogram within this")
    parser.add_argument("--if_double", action="store_true", help="halve the seeds' z (full -> compressed tomogram) before matching")
    parser.add_argument("--min_conf", type=float, default=0.5, help="picks whose confidence is below this get label -1")
    parser.add_argument("--gpus", default="0", help="GPU index; -1 (CPU) is refused")
    return parser


def read_seeds(path, if_double=False):
    """names (M,) str, xyz (M, 3) float64, cls (M,) int64 of a seed table; z halved with if_double."""
    names, xyz, cls = [], [], []
    width = None
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            cells = line.rstrip("\r\n").split("\t")
            if not line.strip():
                continue
            if not names and width is None and cells[0] == "image_name":
                continue                                       # the header
            if len(cells) not in (4, 5) or (width is not None and len(cells) != width):
                raise ValueError("%s line %d: expected image_name x_coord y_coord z_coord [class] in %s tab-separated columns, got %d"
                                 % (path, ln, "4 or 5" if width is None else str(width), len(cells)))
            width = len(cells)
            try:
                p = [float(v) for v in cells[1:4]]
                c = int(cells[4]) if width == 5 else 0
            except ValueError:
                raise ValueError("%s line %d: coordinates are numbers and the class an integer: %r" % (path, ln, line.strip())) from None
            if c < 0:
                raise ValueError("%s line %d: classes are integers >= 0, got %d" % (path, ln, c))
            names.append(cells[0]); xyz.append(p); cls.append(c)
    if not names:
        raise ValueError("%s names no seed" % path)
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    if if_double:
        xyz[:, 2] *= 0.5
    return np.asarray(names), xyz, np.asarray(cls, np.int64)


def tomo_ids(pick_names, seed_names):
    """int32 ids of the tomograms: the picks' in [0, T), a seed's -1 where no pick carries its name."""
    uniq, pick_id = np.unique(np.asarray(pick_names).astype(str), return_inverse=True)
    seed_names = np.asarray(seed_names).astype(str)
    at = np.searchsorted(uniq, seed_names)
    at = np.minimum(at, len(uniq) - 1)
    return pick_id.astype(np.int32), np.where(uniq[at] == seed_names, at, -1).astype(np.int32)


def check_classes(seed_pick, seed_class):
    """The refusals on the matched seeds: one pick with two classes, fewer than two classes.  -> matched (pick, class) arrays."""
    ok = seed_pick >= 0
    pick, cls = seed_pick[ok].astype(np.int64), seed_class[ok].astype(np.int64)
    first = {}
    for i, c in zip(pick.tolist(), cls.tolist()):
        if first.setdefault(i, c) != c:
            raise ValueError("pick %d is matched by seeds of class %d and of class %d" % (i, first[i], c))
    present = np.unique(cls)
    if len(present) < 2:
        raise ValueError("the matched seeds hold %s; label spreading needs at least two: with one class every reachable pick has "
                         "confidence 1 and no threshold separates anything.  Add counter-examples (junk, membrane, gold) as a "
                         "class of their own" % ("class %d only" % present[0] if len(present) else "no class"))
    return pick, cls


def load_graph(path, n, edge_weight):
    from .scan_main import load_graph as load_index
    index = load_index(path, n)
    data = np.load(path)
    if "dist" not in data.files:
        if edge_weight != "binary":
            raise ValueError("--graph %s holds no dist; --edge_weight %s needs it (--edge_weight binary does not)" % (path, edge_weight))
        return index, None
    dist = np.asarray(data["dist"], np.float32)
    if dist.shape != index.shape:
        raise ValueError("--graph %s: dist is %s, index %s" % (path, dist.shape, index.shape))
    return index, dist


def main(args):
    gpu = int(str(args.gpus).split(",")[0])
    if gpu < 0:
        raise RuntimeError("the MI355X path has no CPU mode (--gpus -1)")
    if (args.seeds is None) == (args.seed_index is None):
        raise ValueError("give the seeds as --seeds (a coordinate table) or as --seed_index (pick numbers), one of the two")
    if not 0.0 < args.alpha < 1.0:
        raise ValueError("--alpha must be in (0, 1), got %g" % args.alpha)
    data = np.load(args.input)
    names, coords = data["name"], data["coords"]
    n = len(names)
    graph = load_graph(args.graph, n, args.edge_weight) if args.graph else None
    if args.seeds is not None:
        seed_names, seed_xyz, seed_class = read_seeds(args.seeds, args.if_double)
    else:
        sd = np.load(args.seed_index)
        seed_pick, seed_class = np.asarray(sd["index"], np.int64).ravel(), np.asarray(sd["class"], np.int64).ravel()
        if len(seed_pick) != len(seed_class) or len(seed_pick) == 0:
            raise ValueError("--seed_index %s: index and class name %d and %d seeds" % (args.seed_index, len(seed_pick), len(seed_class)))
        if seed_pick.min() < 0 or seed_pick.max() >= n or seed_class.min() < 0:
            raise ValueError("--seed_index %s names a pick outside 0..%d or a class below 0" % (args.seed_index, n - 1))
        seed_dist = np.zeros(len(seed_pick), np.float64)
        check_classes(seed_pick, seed_class)                   # before the device is touched
    import torch
    from .utils import label_spread as LS
    device = torch.device("cuda", gpu)
    if args.seeds is not None:
        pick_tomo, seed_tomo = tomo_ids(names, seed_names)
        seed_pick, seed_dist = LS.match_seeds(np.asarray(coords, np.float64).reshape(n, 3), pick_tomo, seed_xyz, seed_tomo,
                                              args.seed_radius, device=device)
    print("[cet_pick_amd] propagate_labels: %d seeds, %d unmatched (no pick of their tomogram within %g)"
          % (len(seed_pick), int((seed_pick < 0).sum()), args.seed_radius))
    pick, cls = check_classes(seed_pick, seed_class)
    n_classes = int(cls.max()) + 1
    if n_classes > 64:
        raise ValueError("classes are numbered 0..63, got %d" % (n_classes - 1))
    if graph is None:
        from .plot_2d import knn_graph
        projs = np.ascontiguousarray(data["pred"], dtype=np.float32).reshape(n, -1)
        if not 1 <= args.num_neighbor <= n - 1:
            raise ValueError("--num_neighbor must be in 1..%d (the other picks), got %d" % (n - 1, args.num_neighbor))
        graph = knn_graph(projs, args.num_neighbor, device)
    os.makedirs(args.path, exist_ok=True)
    g = LS.spread_graph(graph[0], graph[1], args.edge_weight, device=device)
    F, n_iter, residual = LS.spread(g, pick, cls, n_classes, alpha=args.alpha, tol=args.tol, max_iter=args.max_iter)
    label, conf, mass = (t.cpu().numpy() for t in LS.decide(F, args.min_conf))
    free = np.asarray(LS.decide(F, 0.0)[0].cpu().numpy())      # the class before --min_conf
    flipped = int((free[pick] != cls).sum())
    out = dict(name=names, coords=coords, label=label.astype(np.int32), conf=conf.astype(np.float32), mass=mass.astype(np.float32),
               score=F.cpu().numpy().astype(np.float32), seed_pick=np.asarray(seed_pick, np.int32),
               seed_class=np.asarray(seed_class, np.int32), seed_dist=np.asarray(seed_dist, np.float64), n_iter=np.int32(n_iter),
               residual=np.float64(residual), alpha=np.float64(args.alpha), edge_weight=np.asarray(args.edge_weight),
               seed_flipped=np.int32(flipped))
    path = os.path.join(args.path, "propagated_labels.npz")
    np.savez(path, **out)
    unreachable = int((mass == 0).sum())
    print("[cet_pick_amd] propagate_labels: %d picks, %d sweeps (residual %.3g); picks per class: %s; %d below --min_conf %g, %d "
          "unreachable from any seed, %d seeds flipped -> %s"
          % (n, n_iter, residual, " ".join(str(int((label == c).sum())) for c in range(n_classes)),
             int((label < 0).sum()) - unreachable, args.min_conf, unreachable, flipped, path))
    return out


if __name__ == "__main__":
    main(add_arguments(argparse.ArgumentParser("spread a few hand labels over the neighbour graph")).parse_args())
