"""What the detector's validation leaves in `opt.debug_dir` under `--debug` (csrc/debug_vis.hip): the
reference's `TomoCRSemiTrainer.debug` (trains/tomo_cr_semi_trainer.py:123-186) with utils/debugger.py.

    mm = slice_minmax(vol, z0, nz)                       # (nz, 2) fp32 on the device
    out = render(tomo, hm_pred, hm_gt, z0, nz, pred_dets, gt_dets)      # (4, nz, H, W, 3) uint8 on the device
    write_detection_table(path, post_dets)               # host: the reference's save_detection
    render_validation_sample(opt, batch, output, iter_id)               # one validation sample: table + PNGs
    finish()                                             # returns when every file handed out so far is on disk

The pictures are rendered in z-slabs into one of two device buffers, copied on a side stream into one of two pinned
buffers of STAGE_BYTES, and encoded by a small thread pool while the device goes on.  There is no CPU path.
"""
import ctypes
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _lib as L
from .post_process import tomo_post_process

PICTURES = ("pred_hm", "gt_hm", "pred_out", "gt_out")     # picture k of `render`
CONF_THRESH = 0.3                                         # save_detection's and add_particle_detection's center_thresh
RING_RADIUS = 8
Z_MARGIN = 20                                             # the reference renders the slices [20, D - 20)
STAGE_BYTES = 64 << 20                                    # one pinned staging buffer (there are two)
PNG_LEVEL = 3
MAX_POOL = 16


# ---- thin wrappers --------------------------------------------------------------------------------------------------------

def _volume(t, name):
    t = L.require_cuda(t, name)
    if t.dim() != 3:
        raise ValueError("%s must be (D, H, W), got %s" % (name, tuple(t.shape)))
    return t.contiguous()


def _host_rows(a, cols):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, cols))
    return a, (a.ctypes.data_as(ctypes.c_void_p) if len(a) else ctypes.c_void_p(0))


def slice_minmax(vol, z0=0, nz=None):
    """(nz, 2) fp32 device tensor: min and max of the slices z0 .. z0 + nz - 1 of a finite (D, H, W) fp32 volume."""
    vol = _volume(vol, "vol")
    D, H, W = vol.shape
    nz = D - z0 if nz is None else nz
    out = torch.empty((max(int(nz), 0), 2), dtype=torch.float32, device=vol.device)
    L.call("mi_dbgvis_minmax", vol, D, H, W, int(z0), int(nz), out)
    return out


def render(tomo, hm_pred, hm_gt, z0, nz, pred_dets, gt_dets, conf_thresh=CONF_THRESH, radius=RING_RADIUS, minmax=None,
           out=None):
    """(4, nz, H, W, 3) uint8 device tensor, RGB: PICTURES of the slices z0 .. z0 + nz - 1.  tomo (D, H, W), hm_pred and hm_gt
    (D, H / 2, W / 2) fp32 on the device; pred_dets (n, 5) [x, y, z, score, conf] and gt_dets (n, 3) [x, y, z] host arrays in
    picture coordinates.  `out`: a device uint8 buffer of at least 12 nz H W bytes to render into."""
    tomo, hm_pred, hm_gt = _volume(tomo, "tomo"), _volume(hm_pred, "hm_pred"), _volume(hm_gt, "hm_gt")
    D, H, W = tomo.shape
    if hm_pred.shape != hm_gt.shape or hm_pred.shape[0] != D:
        raise ValueError("hm_pred %s and hm_gt %s must be equal, with the depth of tomo %s"
                         % (tuple(hm_pred.shape), tuple(hm_gt.shape), tuple(tomo.shape)))
    h, w = int(hm_pred.shape[1]), int(hm_pred.shape[2])
    z0, nz = int(z0), int(nz)
    pred, pred_p = _host_rows(pred_dets, 5)
    gt, gt_p = _host_rows(gt_dets, 3)
    lib = L.lib()
    if minmax is None:
        minmax = slice_minmax(tomo, z0, nz)
    nbytes = 12 * max(nz, 0) * H * W
    if out is None:
        out = torch.empty((nbytes,), dtype=torch.uint8, device=tomo.device)
    elif out.dtype != torch.uint8 or not out.is_cuda or out.numel() < nbytes or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 device buffer of at least %d bytes" % nbytes)
    ws = L.workspace(max(lib.mi_dbgvis_workspace_bytes(nz, len(pred), len(gt)), 16), tomo.device, "debug_vis")
    L.call("mi_dbgvis_render", tomo, hm_pred, hm_gt, D, H, W, h, w, z0, nz, minmax, pred_p, len(pred), gt_p, len(gt), float(conf_thresh),
           int(radius), out, ws, ws.numel())
    return out.reshape(-1)[:nbytes].view(4, nz, H, W, 3)


# ---- the detection table --------------------------------------------------------------------------------------------------

def write_detection_table(path, post_dets):
    """debugger.py:73-82 `save_detection`: per pick [x, y, z, score, conf] of {z: rows} with conf > 0.3 one line
    int(x) <tab> int(floor(z)) <tab> int(floor(y)) <tab> score - the reference's column order."""
    with open(path, "w+") as f:
        for rows in post_dets.values():
            for c in rows:
                x, y, z = int(c[0]), int(np.floor(c[1])), int(np.floor(c[2]))
                if c[4] > CONF_THRESH:
                    print(str(x) + "\t" + str(z) + "\t" + str(y) + "\t" + str(c[3]), file=f)


# ---- staging, copy and PNG encoding ---------------------------------------------------------------------------------------

def pool_size():
    """Encoder threads: OMP_NUM_THREADS when set, 8 otherwise, at most 16 (never the machine's CPU count)."""
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", ""))
    except ValueError:
        n = 8
    return max(1, min(MAX_POOL, n))


class _Stage:
    """Two device buffers, two pinned buffers, a copy stream and the encoder pool of one device."""

    def __init__(self, device):
        self.device = device
        self.copy_stream = torch.cuda.Stream(device)
        self.pinned = [None, None]
        self.dev = [None, None]
        self.copied = [None, None]                # event: the copy out of dev[b] into pinned[b] is done
        self.busy = [[], []]                      # encoder tasks that still read pinned[b]
        self.turn = 0
        self.pool = ThreadPoolExecutor(max_workers=pool_size(), thread_name_prefix="debug_vis_png")
        self.pending = []
        self.lock = threading.Lock()
        self.encode_s = 0.0
        self.files = 0

    def buffers(self, nbytes):
        """The next (device, pinned) pair, free to be written: its earlier readers are waited for."""
        b = self.turn
        self.turn ^= 1
        for f in self.busy[b]:
            f.result()
        self.busy[b] = []
        size = max(STAGE_BYTES, nbytes)
        if self.pinned[b] is None or self.pinned[b].numel() < size:
            self.pinned[b] = torch.empty((size,), dtype=torch.uint8, pin_memory=True)
            self.dev[b] = torch.empty((size,), dtype=torch.uint8, device=self.device)
        if self.copied[b] is not None:
            torch.cuda.current_stream(self.device).wait_event(self.copied[b])
        return b

    def _encode(self, event, views, paths):
        from PIL import Image
        event.synchronize()
        t0 = time.perf_counter()
        for v, p in zip(views, paths):
            Image.fromarray(v).save(p, format="PNG", compress_level=PNG_LEVEL)
        with self.lock:
            self.encode_s += time.perf_counter() - t0
            self.files += len(paths)

    def ship(self, b, nz, H, W, paths_of_slice):
        """Copy the slab rendered into dev[b] to pinned[b] on the copy stream and hand its slices to the pool."""
        nbytes = 12 * nz * H * W
        cur = torch.cuda.current_stream(self.device)
        rendered = torch.cuda.Event()
        rendered.record(cur)
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(rendered)
            self.pinned[b][:nbytes].copy_(self.dev[b][:nbytes], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.copy_stream)
        self.copied[b] = done
        host = self.pinned[b].numpy()[:nbytes].reshape(4, nz, H, W, 3)
        for i in range(nz):
            f = self.pool.submit(self._encode, done, [host[k, i] for k in range(4)], paths_of_slice(i))
            self.busy[b].append(f)
            self.pending.append(f)

    def finish(self):
        pending, self.pending = self.pending, []
        for f in pending:
            f.result()


_stages = {}


def _stage(device):
    key = str(device)
    if key not in _stages:
        _stages[key] = _Stage(device)
    return _stages[key]


def finish():
    """Returns when every picture handed to the encoders is on disk (an encoder's error is raised here)."""
    for s in _stages.values():
        s.finish()


def encode_stats(reset=False):
    """(seconds spent inside the PNG encoders summed over the threads, files written) since the last reset"""
    sec = sum(s.encode_s for s in _stages.values())
    n = sum(s.files for s in _stages.values())
    if reset:
        for s in _stages.values():
            s.encode_s, s.files = 0.0, 0
    return sec, n


def render_slices(tomo, hm_pred, hm_gt, pred_dets, gt_dets, z_lo, z_hi, path_of):
    """PNGs of the four pictures of the slices [z_lo, z_hi): path_of(picture name, z) names each file.  Returns at once;
    `finish()` waits for the files."""
    D, H, W = tomo.shape
    if z_hi <= z_lo:
        return
    stage = _stage(tomo.device)
    per = max(1, STAGE_BYTES // (12 * H * W))
    mm = slice_minmax(tomo, z_lo, z_hi - z_lo)
    for z0 in range(z_lo, z_hi, per):
        nz = min(per, z_hi - z0)
        b = stage.buffers(12 * nz * H * W)
        render(tomo, hm_pred, hm_gt, z0, nz, pred_dets, gt_dets, minmax=mm[z0 - z_lo:], out=stage.dev[b])
        stage.ship(b, nz, H, W, lambda i, z0=z0: [path_of(k, z0 + i) for k in PICTURES])


# ---- one validation sample ------------------------------------------------------------------------------------------------

def decode_sample(opt, output):
    """The picks of one sample as the reference's debug() has them: (1, K, 5) numpy [x, y, z, score, conf], x and y at full
    resolution."""
    from ..models.decode import tomo_decode
    dets = tomo_decode(output["hm"], K=opt.K, if_fiber=opt.fiber)
    dets = dets.detach().cpu().numpy().reshape(1, -1, dets.shape[2])
    dets[:, :, :2] *= opt.down_ratio
    return dets


def render_validation_sample(opt, batch, output, iter_id):
    """debug() of one validation sample (batch size 1): `<debug_dir>/<name>_<iter_id>.txt` and, under --debug 4, the PNGs
    `<debug_dir>/<iter_id>_<name><picture><z>.png` of the slices [20, D - 20).  -> the picks grouped by slice, or None when
    --debug is off.  Two things differ from the reference on purpose: a ring is drawn at the pick's
    full-resolution position (not at twice that), and the ground truth is in the coordinates of the validation window."""
    if opt.debug <= 0:
        return None
    hm = output["hm"]
    D = int(hm.shape[2])
    post = tomo_post_process(decode_sample(opt, output), z_dim_tot=D)[0]
    name = batch["meta"]["name"][0]
    os.makedirs(opt.debug_dir, exist_ok=True)
    write_detection_table(os.path.join(opt.debug_dir, "{}_{}.txt".format(name, iter_id)), post)
    if opt.debug != 4:
        return post
    pred = np.asarray([r for rows in post.values() for r in rows], dtype=np.float32).reshape(-1, 5)
    gt = np.array(batch["meta"].get("gt_det", np.zeros((0, 3))), dtype=np.float32).reshape(-1, 3)
    gt[:, :2] *= opt.down_ratio
    prefix = "{}_{}".format(iter_id, name)
    render_slices(batch["input"][0], hm[0, 0], batch["hm"][0, 0], pred, gt, Z_MARGIN, D - Z_MARGIN,
                  lambda k, z: os.path.join(opt.debug_dir, "{}{}{}.png".format(prefix, k, z)))
    return post
