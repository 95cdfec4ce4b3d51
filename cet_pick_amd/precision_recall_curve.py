"""Precision-recall curve of scored picks against target centres (mirror of the reference's cet_pick/precision_recall_curve.py).

    python -m cet_pick_amd.precision_recall_curve --predicted out/all_coords.txt --targets val_coords.txt --path out \
        -r 10 --out pr.txt --stats stats.txt --folder run1 --w overall.txt

Every image of the list is matched in ONE batched launch of the device's optimal matching (evaluation/algorithms.py).  A pick
and a target may pair where their squared distance is below the CUBE of `-r`, as in the reference.  The images are taken in
sorted order (the reference walks a `set`; its order changes nothing but the order in which tied scores are concatenated).

Files: `--out` in `--path`, the table `threshold precision recall f1`; `--stats` in `--path`, a header and the rows of best
precision, best recall and best f1; one line `folder<TAB>auprc` appended to `--w`; `# auprc=..., mae=...` on stdout.
"""
import os

import numpy as np
import pandas as pd

from cet_pick_amd.evaluation.metrics import precision_recall_curve


def add_arguments(parser):
    parser.add_argument('--predicted', help='path to file containing predicted particle coordinates with scores')
    parser.add_argument('--targets', help='path to file specifying target particle coordinates')
    parser.add_argument('--path', help='path to all output files')
    parser.add_argument('-r', '--assignment-radius', required=True, type=int,
                        help='maximum distance between prediction and labeled target allowed for considering them a match')
    parser.add_argument('--images', choices=['target', 'predicted', 'union'], default='target',
                        help='only count particles on micrographs with coordinates labeled in the targets file, the predicted '
                             'file, or the union of those (default: target)')
    parser.add_argument('--stats', help='file to output max stats')
    parser.add_argument('--out', help='out file for precision recall stats')
    parser.add_argument('--folder', help='folder name')
    parser.add_argument('--w', help='overall stats file')
    return parser


def main(args, match_batch=None):
    """match_batch(targets, preds, radius) -> ([(assignment, dist)], costs): the device's by default; the tests pass the host
    arbiter to write the files it expects."""
    if match_batch is None:
        from cet_pick_amd.evaluation.algorithms import match_coordinates_batch as match_batch
    predicts = pd.read_csv(args.predicted, sep='\t', comment='#')
    targets = pd.read_csv(args.targets, sep='\t')
    if args.images == 'union':
        image_list = set(targets.image_name.unique()) | set(predicts.image_name.unique())
    elif args.images == 'target':
        image_list = set(targets.image_name.unique())
    else:
        image_list = set(predicts.image_name.unique())
    image_list = sorted(image_list)
    N = len(targets)

    cols = ['x_coord', 'y_coord', 'z_coord']
    target_coords = [targets.loc[targets.image_name == name][cols].values for name in image_list]
    predict_coords = [predicts.loc[predicts.image_name == name][cols].values for name in image_list]
    scores = [predicts.loc[predicts.image_name == name].score.values.astype(np.float32) for name in image_list]
    matched, _ = match_batch(target_coords, predict_coords, args.assignment_radius)

    count = 0
    mae = 0
    with np.errstate(invalid='ignore', divide='ignore'):
        for match, dist in matched:        # the reference's running mean, image by image
            this_mae = np.sum(dist[match == 1])
            count += np.sum(match)
            delta = this_mae - np.sum(match) * mae
            mae += delta / count
    matches = np.concatenate([m for m, _ in matched], 0)
    scores = np.concatenate(scores, 0)

    precision, recall, threshold, auprc = precision_recall_curve(matches, scores, N=N)
    with open(args.w, 'a') as overall_output:
        overall_output.write('\t'.join([str(args.folder), str(auprc)]) + '\n')
    print('# auprc={}, mae={}'.format(auprc, np.sqrt(mae)))

    mask = (precision + recall) == 0
    f1 = 2 * precision * recall
    f1[mask] = 0
    f1[~mask] /= (precision + recall)[~mask]

    table = pd.DataFrame({'threshold': threshold})
    table['precision'] = precision
    table['recall'] = recall
    table['f1'] = f1
    table.to_csv(os.path.join(args.path, args.out), sep='\t', index=False)
    with open(os.path.join(args.path, args.stats), 'w') as out_file:
        out_file.write('\t'.join(['threshold', 'precision', 'recall', 'f1']) + '\n')
        for col in ('precision', 'recall', 'f1'):
            out_file.write('\t'.join(str(i) for i in list(table.loc[table[col].idxmax()])) + '\n')
    return auprc


if __name__ == '__main__':
    import argparse
    main(add_arguments(argparse.ArgumentParser(
        'Script for calculating the precision-recall curve for a set of predicted particle coordinates and a set of target '
        'coordinates.')).parse_args())
