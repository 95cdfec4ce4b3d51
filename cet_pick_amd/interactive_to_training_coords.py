"""Picks of the chosen classes -> the coordinate table of the refinement training (`main.py semi --train_coord_txt`):

    python -m cet_pick_amd.interactive_to_training_coords --input X --output training_coordinates.txt [--if_double]
                                                          [--labels 3,17,42]

X: a parquet file or a folder of *.parquet exported from the interactive session (the reference's input; needs pandas), or the
kmeans_labels.npz of `cet_pick_amd.plot_2d` (numpy only).  --labels keeps the picks of those classes only.  The table is
tab-separated with the header image_name x_coord y_coord z_coord; --if_double doubles z (compressed -> full tomogram).
"""
import argparse
import glob
import os

import numpy as np

HEADER = ("image_name", "x_coord", "y_coord", "z_coord")


def add_arguments(parser):
    parser.add_argument("--input", type=str, required=True, help="parquet file, folder of *.parquet, or kmeans_labels.npz")
    parser.add_argument("--output", type=str, required=True, help="output with all training coordinates")
    parser.add_argument("--if_double", action="store_true", help="double the z coordinate (from compressed to uncompressed)")
    parser.add_argument("--labels", type=str, default=None, help="comma-separated classes to keep (default: every pick)")
    return parser


def _rows_npz(path):
    data = np.load(path)
    names, coords, labels = data["name"], data["coords"], data["label"]
    for n, c, l in zip(names, coords, labels):
        yield str(n), [str(j) for j in list(c)], int(l)


def _rows_parquet(path):
    try:
        import pandas as pd
    except ImportError as e:
        raise RuntimeError("reading %s needs pandas with a parquet engine (%s); a kmeans_labels.npz needs numpy only" % (path, e)) from None
    df = pd.read_parquet(path)
    names, coords = df.loc[:, "name"].to_numpy(), df.loc[:, "coord"].to_numpy()
    labels = df.loc[:, "label"].to_numpy() if "label" in df.columns else [None] * len(names)
    for n, c, l in zip(names, coords, labels):
        yield str(n), [str(j) for j in c], (None if l is None else int(l))


def rows(path):
    if os.path.isfile(path):
        files = [path]
    else:
        files = sorted(glob.glob(os.path.join(path, "*.parquet")))
        if not files:
            raise FileNotFoundError("%s is neither a file nor a folder with *.parquet files" % path)
    for f in files:
        yield from (_rows_npz(f) if f.endswith(".npz") else _rows_parquet(f))


def main(args):
    keep = None if args.labels is None else {int(v) for v in args.labels.split(",") if v.strip()}
    n_out = 0
    with open(args.output, "w") as f:
        f.write("\t".join(HEADER) + "\n")
        for name, (x, y, z), label in rows(args.input):
            if keep is not None:
                if label is None:
                    raise ValueError("--labels needs a `label` column in %s" % args.input)
                if label not in keep:
                    continue
            if args.if_double:
                z = str(float(z) * 2)
            f.write("\t".join([name, x, y, z]) + "\n")
            n_out += 1
    print("[cet_pick_amd] %d training coordinates -> %s" % (n_out, args.output))
    return n_out


if __name__ == "__main__":
    main(add_arguments(argparse.ArgumentParser("class table -> training coordinates of the refinement module")).parse_args())
