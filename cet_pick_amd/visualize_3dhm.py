"""Paint the picks into the tomograms in the colours of the 2-D map (the reference's visualize_3dhm.py, same command line):

    python -m cet_pick_amd.visualize_3dhm --input exp/.../all_output_info.npz --color exp/.../all_colors.npy
                                          --dir_simsiam OUT (--image_txt LIST.txt | --rec_dir DIR [--ext .rec])
                                          [--compress] [--order xzy] [--gpus 0]

--input holds `name` and `coords` (x, y, z per pick), --color the (N, 3) uint8 colour of every pick as
`plot_2d --mode tsne --num_neighbor P` writes it.  With --image_txt every listed image_name / rec_path whose file exists is
taken, otherwise rec_dir/name + ext for every unique name of the input.  For each tomogram with picks:

    OUT/{name}_rec3d.npy         (Z, R, C, 3) uint8: the tomogram, per-slice normalised, quantised and smoothed by the 8-bit
                                 Gaussian (sigma 0.8) - scipy.ndimage.gaussian_filter on the stacked bytes, bit for bit
    OUT/{name}_hm3d_simsiam.npy  (Z, R, C, 3) uint8: on every slice that holds a pick, the discs (radius 12 - |dz|, |dz| <= 2)
                                 of the picks in their colours, the last pick of the input on top; zero elsewhere

to be overlaid in napari.  Everything volume-sized runs on the MI355X (utils/vis3d.py, csrc/vis3d.hip).
Differences from the reference: fp32 storage between the normalisation steps as utils/loader.py has it; a slice of zero
variance gives bytes 0 where the reference casts NaN; the disc is dx^2 + dy^2 <= r^2, so rim pixels may differ from
cv2.circle's; an odd number of slices with --compress and a pick outside the volume are refused (the reference indexes out
of range).  There is no CPU path.
"""
import argparse
import os

import numpy as np


def add_arguments(parser):
    parser.add_argument("--input", type=str, help="all_output_info.npz of the exploration inference (name, coords)")
    parser.add_argument("--color", type=str, help="all_colors.npy of plot_2d: one (r, g, b) uint8 row per pick")
    parser.add_argument("--dir_simsiam", type=str, help="output directory")
    parser.add_argument("--image_txt", type=str, help="tab-separated list with the columns image_name and rec_path (the "
                        "exploration training list); listed tomograms whose file exists are taken")
    parser.add_argument("--rec_dir", type=str, help="without --image_txt: directory that holds <name><ext> for every name of the input")
    parser.add_argument("--compress", action="store_true", help="max of every two neighbouring slices, as the data set was read")
    parser.add_argument("--order", type=str, default="xzy", help="axis order of the tomogram files: xyz, xzy, yxz or zxy")
    parser.add_argument("--ext", type=str, default=".rec", help="file extension of the tomograms under --rec_dir (.rec or .mrc)")
    parser.add_argument("--gpus", default="0", help="GPU index; -1 (CPU) is refused")
    return parser


def get_3d_hm(volume, coords, labels, names, use_name, out_dir):
    """Both volumes of one tomogram: `volume` (Z, R, C) fp32 on the device as utils.vis3d.load_volume returns it, coords / labels
    / names of the whole input.  True when they were written, False (the reference's message) without picks."""
    from .utils import vis3d as V
    rows, picks = V.tomogram_picks(coords, names, use_name, volume.shape[0])
    if len(rows) == 0:
        print("skipping 3D tomogram visualization for {}, no coordinates in the file....".format(use_name))
        return False
    np.save(os.path.join(out_dir, use_name) + "_rec3d.npy", V.rec3d(volume).cpu().numpy())
    hm = V.paint(picks, np.asarray(labels)[rows], tuple(volume.shape), device=volume.device)
    np.save(os.path.join(out_dir, use_name) + "_hm3d_simsiam.npy", hm.cpu().numpy())
    return True


def main(args):
    gpu = int(str(args.gpus).split(",")[0])
    if gpu < 0:
        raise RuntimeError("the MI355X path has no CPU mode (--gpus -1)")
    import torch
    from .utils import vis3d as V
    data = np.load(args.input)
    names, coords = data["name"], data["coords"]
    colors = np.load(args.color)
    if colors.ndim != 2 or colors.shape != (len(names), 3):
        raise ValueError("%s: one (r, g, b) colour per pick of %s is needed, (%d, 3); got %s"
                         % (args.color, args.input, len(names), colors.shape))
    if args.image_txt is not None:
        print("using image list files from training file..")
        from .datasets.tomo_files import read_image_list
        todo = read_image_list(args.image_txt)
    else:
        if args.rec_dir is None:
            raise ValueError("one of --image_txt and --rec_dir is needed")
        todo = [(str(nm), os.path.join(args.rec_dir, str(nm)) + args.ext) for nm in np.unique(names)]
    os.makedirs(args.dir_simsiam, exist_ok=True)
    with torch.cuda.device(gpu):
        for nm, rec in todo:
            if not os.path.exists(rec):
                print("skipping 3D tomogram visualization for {}, file not found....".format(nm))
                continue
            print("constructing 3D tomogram visualization for {}....".format(nm))
            get_3d_hm(V.load_volume(rec, order=args.order, compress=args.compress), coords, colors, names, nm, args.dir_simsiam)


if __name__ == "__main__":
    main(add_arguments(argparse.ArgumentParser("Script for visualizing 3D tomogram visualization")).parse_args())
