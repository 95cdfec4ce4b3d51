"""`python -m cet_pick_amd.simsiam_test_hm_2d3d simsiam2d3d --arch simsiam2d3d_18 --load_model ...` - the reference's
cet_pick/simsiam_test_hm_2d3d.py (:151-232): exploration inference of the 2d3d mode.  Every kept pick's tilt patch and
tomogram patch go through the per-channel 8-bit round trip + `Normalize((mean_subvols, mean_subvols3d), (std_subvols,
std_subvols3d))` of `PrefetchDatasetProj` (:47-53, on the device: datasets/subvols.py `to_uint8_normalize`), the encoder's
`forward_test(x_2d, x_3d)`, and `all_output_info.npz` = {proj, pred, name, coords, subvol, subvols_2d} is written under
save_dir (:224-226): `subvol` the normalised tomogram patches (n, 1, bbox, bbox), `subvols_2d` the normalised tilt patches.

The test list is the 4-column list of the 2d3d mode (datasets/simsiam2d3d.py); without one the synthetic twin is used."""
import os

import numpy as np
import torch

from .datasets.simsiam2d3d import SyntheticSimSiam2D3DDataset
from .models.model import create_model, load_model
from .opts import opts
from .utils.utils import TextLog


LAST_STAGES = {}         # seconds of the last call's stages


def test(opt):
    import time
    t_start = time.time()
    Dataset = SyntheticSimSiam2D3DDataset
    opt = opts().update_dataset_info_and_set_heads(opt, Dataset)
    TextLog(opt).close()
    if opt.gpus[0] < 0:
        raise RuntimeError("the MI355X path has no CPU mode (--gpus -1)")
    opt.device = torch.device("cuda", opt.gpus[0])
    model = create_model(opt.arch, opt.heads, opt.head_conv)
    if opt.load_model != "":
        model = load_model(model, opt.load_model)
    model = model.to(opt.device)
    model.eval()
    from .datasets.tomo_files import use_files
    if use_files(opt, "test"):
        from .datasets.simsiam2d3d import TomoFileSimSiam2D3DDataset as Dataset
    t_model = time.time()
    dataset = Dataset(opt, "test", (3, opt.bbox, opt.bbox), sigma1=opt.dog, device=opt.device)
    torch.cuda.synchronize()
    t_data = time.time()
    x2d, x3d = dataset.normed_2d[:, 0].contiguous(), dataset.normed_3d[:, 0].contiguous()
    all_proj, all_pred = [], []
    with torch.no_grad():
        for i in range(0, x2d.shape[0], 256):                           # batch_size=256 (:167)
            ret = model.forward_test(x2d[i:i + 256], x3d[i:i + 256])
            all_proj.append(ret["proj"].detach())                       # (on the device until the one copy below)
            all_pred.append(ret["pred"].detach())
    proj, pred = torch.cat(all_proj, 0).cpu().numpy(), torch.cat(all_pred, 0).cpu().numpy()
    subvol, subvols_2d = x3d.cpu().numpy(), x2d.cpu().numpy()
    t_net = time.time()
    out_file = os.path.join(opt.save_dir, "all_output_info.npz")
    np.savez(out_file, proj=proj, pred=pred, name=np.asarray(dataset.names_all), coords=np.asarray(dataset.coords),
             subvol=subvol, subvols_2d=subvols_2d)
    LAST_STAGES.update({"model": t_model - t_start, "load_pick_crop": t_data - t_model, "net": t_net - t_data, "save": time.time() - t_net})
    print("opt.save_dir", opt.save_dir)
    return out_file


if __name__ == "__main__":
    test(opts().parse())
