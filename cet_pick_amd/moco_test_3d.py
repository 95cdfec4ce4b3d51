"""`python -m cet_pick_amd.moco_test_3d moco --arch moco3d_18 --load_model exp/moco/<id>/model_last.pth --test_img_txt LIST.txt
--bbox 32 --dog 3,5 [--tta 1|2|4|8]` - exploration inference with the encoder `moco_main` trains: every DoG pick of the listed
tomograms that keeps a whole bbox^3 box inside its volume is embedded by `encoder_q` in eval mode, and `all_output_info.npz` =
{proj, pred, name, coords, subvol, tta, bbox} is written under save_dir for the tools that read the SimSiam tests' file
(plot_2d, scan_main, visualize_3dhm, interactive_to_training_coords).

The reference's cet_pick/moco_test_3d.py is a copy of its SimSiam test that feeds (3, bbox, bbox) pictures to the 3-D encoder;
this is the intended behaviour, as moco_main is: z-normalised bbox^3 crops (`crop_znorm`'s) through `forward_test`.  A 3-D
convolutional embedding is not invariant to the in-plane orientation a particle happens to lie at, so the descriptor is pooled
over `--tta` of the eight in-plane lattice poses of the box (quarter turns, each with or without the mirror image: no
interpolation): each pose's embedding is L2-normalised, the mean is taken and normalised again.  With all eight the descriptor
is invariant under that group; `--tta 1` is the reference's `F.normalize(feature, dim=1)` of the crop as it lies.  `pred` is
`proj`: in this encoder the `pred` head IS the `proj` module.  `subvol` holds the 2-D picture of every pick as
simsiam_test_hm_3d stores it.  The reference's `preselect_*_f.npy` files are not written: nothing in this project reads them.
"""
import os

import numpy as np
import torch

from . import hipops as H
from .datasets import subvols as S
from .datasets.synthetic_moco import centre_border
from .datasets.tomo_files import load_listed_tomos
from .models.model import create_model
from .opts import opts
from .utils import image as Im
from .utils.utils import TextLog

LAST_STAGES = {}         # seconds of the last call's stages

POSE_SETS = {1: [0], 2: [0, 4], 4: [0, 1, 2, 3], 8: [0, 1, 2, 3, 4, 5, 6, 7]}     # pose p: p & 3 quarter turns, p & 4 mirror


def pose_set(tta):
    if tta not in POSE_SETS:
        raise ValueError("--tta must be one of %s, got %r" % (sorted(POSE_SETS), tta))
    return list(POSE_SETS[tta])


def encoder_state_dict(state_dict):
    """The query encoder's entries of a checkpoint's state dict: `encoder_q.*` of the MoCo wrapper moco_main saves (the key
    encoder and the queue are dropped), or a bare encoder's own keys.  Anything else raises, naming the keys it found."""
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
    q = {k[len("encoder_q."):]: v for k, v in sd.items() if k.startswith("encoder_q.")}
    if q:
        return q
    if "conv1.weight" in sd and not any(k.startswith("encoder_k.") for k in sd):
        return sd
    raise ValueError("the checkpoint holds neither a MoCo wrapper (encoder_q.*) nor a moco3d encoder (conv1.weight ...); "
                     "its keys: %s" % ", ".join(sorted(state_dict)))


def load_encoder(model, path):
    """Fill `model` from the file moco_main's save_model writes ({'epoch', 'state_dict'}) or from a plain state dict.  Every
    parameter and buffer of the encoder must be there: inference on half-loaded weights is refused, not reported."""
    ckpt = torch.load(path, map_location="cpu")
    sd = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
    model.load_state_dict(encoder_state_dict(sd), strict=True)
    return model


def whole_box_picks(rec, sigmas, bbox):
    """The DoG picks (x, y, z) of `rec` that TomoFileMocoLoader keeps in its "mirror" form: bbox // 2 + 1 voxels from every face."""
    d, h, w = rec.shape
    bd = centre_border(bbox, "mirror")
    _, c = Im.get_potential_coords_pyramid(rec, sigmas=list(sigmas), border_z=min(10, max(d // 4, 1)))
    keep = ((c[:, 0] >= bd) & (c[:, 0] < w - bd) & (c[:, 1] >= bd) & (c[:, 1] < h - bd) & (c[:, 2] >= bd) & (c[:, 2] < d - bd))
    return c[keep].astype(np.int32)


def picks_per_batch(bbox, n_poses, batch=256):
    """`batch`, shrunk for the encoder: the kernels take operands below 2 GiB.  The batch's crops are b P bbox^3 floats, but the
    encoder's largest activation is the stem's output, 64 channels at half the extent: 8 x the crops.  b shrinks until THAT is
    at most 512 MiB (64 picks = 512 crops at --bbox 32 --tta 8, which fill the chip), so the crops stay under 64 MiB."""
    return max(1, min(int(batch), (1 << 29) // (int(n_poses) * int(bbox) ** 3 * 32)))


def embed_picks(model, rec, coords, bbox, tta=8, batch=256):
    """(n, 128) unit rows on the device: the pose-pooled `proj` embedding of the bbox^3 box around every centre (x, y, z) of
    the (D, H, W) device tensor `rec`.  `model`: the encoder, in eval mode; the caller holds torch.no_grad().  Per batch: one
    crop launch for all poses, `forward_test` on the (b P, 1, bbox, bbox, bbox) view, one pooling launch; nothing goes to the
    host."""
    poses = pose_set(tta)
    p, bbox = len(poses), int(bbox)
    coords = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 3)
    n = len(coords)
    table = S.CropTable([rec], np.zeros(n, np.int32), coords)
    b = picks_per_batch(bbox, p, batch)
    out = torch.empty((n, model.fc.out_f), dtype=torch.float32, device=rec.device)     # (the heads keep fc's 128 columns)
    for i in range(0, n, b):
        k = min(b, n - i)
        crops = table.cut_poses(i, k, (bbox, bbox, bbox), poses)
        z = model.forward_test(crops.view(k * p, 1, bbox, bbox, bbox))["proj"]
        H.embed_pool(z.contiguous().view(k, p, -1), out=out[i:i + k])
    return out


def test(opt):
    import time
    t_start = time.time()

    class _DS:                                   # dataset info of task 'moco' (opts.py:321), as moco_main
        default_resolution, num_classes = [32, 32], 256
    opt = opts().update_dataset_info_and_set_heads(opt, _DS)
    TextLog(opt).close()
    if opt.gpus[0] < 0:
        raise RuntimeError("the MI355X path has no CPU mode (--gpus -1)")
    if opt.load_model == "":
        raise ValueError("moco_test_3d needs --load_model: the checkpoint moco_main wrote")
    opt.device = torch.device("cuda", opt.gpus[0])
    model = create_model(opt.arch, opt.heads, opt.head_conv, last_k=opt.last_k)
    model = load_encoder(model, opt.load_model).to(opt.device)
    model.eval()
    t_model = time.time()
    names, coords, pictures, projs = [], [], [], []
    with torch.no_grad(), torch.cuda.device(opt.device):
        for name, rec in load_listed_tomos(opt, "test").items():
            c = whole_box_picks(rec, opt.dog, opt.bbox)
            if len(c) == 0:
                continue
            projs.append(embed_picks(model, rec, c, opt.bbox, opt.tta))
            pictures.append(S.extract_subvols(rec, c, (3, opt.bbox, opt.bbox)))
            names += [name] * len(c)
            coords.append(c)
        if not coords:
            raise RuntimeError("the DoG picker found no crop centre with a whole %d^3 box on the listed tomograms" % opt.bbox)
        pictures = torch.cat(pictures, 0)
        mean, std = S.subvol_mean_std(pictures)
        subvol = S.to_uint8_normalize(pictures, mean, std).cpu().numpy()
        proj = torch.cat(projs, 0).cpu().numpy()              # (the one copy to the host)
    t_net = time.time()
    out_file = os.path.join(opt.save_dir, "all_output_info.npz")
    np.savez(out_file, proj=proj, pred=proj, name=np.asarray(names), coords=np.concatenate(coords, 0), subvol=subvol,
             tta=np.int32(opt.tta), bbox=np.int32(opt.bbox))
    LAST_STAGES.update({"model": t_model - t_start, "load_pick_embed": t_net - t_model, "save": time.time() - t_net})
    print("opt.save_dir", opt.save_dir)
    return out_file


if __name__ == "__main__":
    test(opts().parse())
