"""Merge the per-tomogram pick files of `test.py` into one table (mirror of the reference's cet_pick/merge_output.py).

    python -m cet_pick_amd.merge_output --path exp/semi/run/output --out all_coords.txt

Writes `--out` inside `--path`: the header `image_name x_coord z_coord y_coord score` and one line per pick, prefixed with the
stem of the file it came from.  The `*.txt` files are taken in sorted order, and the output file itself is skipped if it
already lies in `--path`.

As in the reference, the FIRST line of every file is dropped (`if i > 0`).  The files `test.py` writes have no header, so
one pick per tomogram is not scored.
"""
import glob
import os


def add_arguments(parser):
    parser.add_argument('--path', help='path to file containing predicted particle coordinates with scores')
    parser.add_argument('--out', help='output file for all merged coordinates')
    return parser


def main(args):
    out_file = os.path.join(args.path, args.out)
    txts = sorted(f for f in glob.glob(os.path.join(args.path, '*.txt'))
                  if os.path.abspath(f) != os.path.abspath(out_file))
    with open(out_file, 'w') as out:
        out.write('\t'.join(['image_name', 'x_coord', 'z_coord', 'y_coord', 'score']) + '\n')
        for f in txts:
            name = os.path.basename(f)[:-4]
            with open(f) as dets:
                for i, line in enumerate(dets):
                    if i > 0:          # the reference's: line 0 of every file is dropped
                        out.write('\t'.join([name] + line.split()) + '\n')
    return out_file


if __name__ == '__main__':
    import argparse
    main(add_arguments(argparse.ArgumentParser('Script for merge all coordinates')).parse_args())
