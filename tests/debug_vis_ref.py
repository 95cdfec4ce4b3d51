"""numpy restatement of csrc/debug_vis.hip (the arbiter of tests/test_debug_vis_cpu.py and tests/test_debug_vis_gpu.py): the four
pictures that the detector's validation writes per slice under --debug 4, as DESIGN.md 4.19 defines them.  The reference
draws them with cv2, which the build machine does not have: equality with cv2's own pixels is not verified anywhere.

    ring_offsets(r)                     the (dx, dy) of the midpoint circle algorithm
    ring_mask(r)                        the same as a (2r+1, 2r+1) bool array [dy + r, dx + r]
    unit_bytes(m)                       trunc(min(max(255 m, 0), 255)) in float32
    upsample2x(a)                       2 x bilinear, half-pixel centres, replicated edges, exact integers
    grey_slice(v)                       min-max normalisation of one slice to bytes, float32, one rounding per operation
    blend(grey, fore)                   the reference's add_blend_img(trans=0.7) in float64
    render(...)                         (4, nz, H, W, 3) uint8: pred_hm, gt_hm, pred_out, gt_out
"""
import numpy as np

BLUE = (0, 0, 255)


def ring_offsets(r):
    r = int(r)
    pts = set()
    x, y, err = r, 0, 1 - r
    while x >= y:
        for dx, dy in ((x, y), (y, x), (-x, y), (-y, x), (x, -y), (y, -x), (-x, -y), (-y, -x)):
            pts.add((dx, dy))
        y += 1
        if err < 0:
            err += 2 * y + 1
        else:
            x -= 1
            err += 2 * (y - x) + 1
    return pts


def ring_mask(r):
    m = np.zeros((2 * r + 1, 2 * r + 1), dtype=bool)
    for dx, dy in ring_offsets(r):
        m[dy + r, dx + r] = True
    return m


def unit_bytes(m):
    t = np.asarray(m, dtype=np.float32) * np.float32(255)
    return np.minimum(np.maximum(t, np.float32(0)), np.float32(255)).astype(np.int64)


def upsample2x(a):
    a = np.asarray(a, dtype=np.int64)
    h, w = a.shape
    y, x = np.arange(2 * h), np.arange(2 * w)
    sy, sx = y >> 1, x >> 1
    ny = np.where(y & 1, np.minimum(sy + 1, h - 1), np.maximum(sy - 1, 0))
    nx = np.where(x & 1, np.minimum(sx + 1, w - 1), np.maximum(sx - 1, 0))
    a00, a01 = a[sy][:, sx], a[sy][:, nx]
    a10, a11 = a[ny][:, sx], a[ny][:, nx]
    return (9 * a00 + 3 * a01 + 3 * a10 + a11 + 8) >> 4


def grey_slice(v):
    v = np.asarray(v, dtype=np.float32)
    mn, mx = v.min(), v.max()
    d = np.float32(mx - mn)
    s = np.float32(0) if d == 0 else np.float32(1) / d
    t = (v - mn) * s
    return unit_bytes(t)


def blend(grey, fore):
    b = np.asarray(grey, dtype=np.float64) * (1.0 - 0.7) + np.asarray(fore, dtype=np.float64) * 0.7
    b[b > 255] = 255
    b[b < 0] = 0
    return b.astype(np.uint8)


def draw_rings(img, centres, radius):
    """(0, 0, 255) at every ring pixel inside the picture; centres: iterable of integer (cx, cy)"""
    H, W = img.shape[:2]
    off = ring_offsets(radius)
    for cx, cy in centres:
        for dx, dy in off:
            x, y = cx + dx, cy + dy
            if 0 <= x < W and 0 <= y < H:
                img[y, x] = BLUE


def render(tomo, hm_pred, hm_gt, z0, nz, pred_dets, gt_dets, conf_thresh=0.3, radius=8):
    tomo = np.asarray(tomo, dtype=np.float32)
    D, H, W = tomo.shape
    pred_dets = np.asarray(pred_dets, dtype=np.float32).reshape(-1, 5)
    gt_dets = np.asarray(gt_dets, dtype=np.float32).reshape(-1, 3)
    pred_dets = pred_dets[np.isfinite(pred_dets[:, :3]).all(1)]             # rows that are not finite are ignored
    gt_dets = gt_dets[np.isfinite(gt_dets).all(1)]
    thr = np.float32(conf_thresh)
    out = np.zeros((4, nz, H, W, 3), dtype=np.uint8)
    for i in range(nz):
        z = z0 + i
        g = grey_slice(tomo[z]).astype(np.uint8)
        grey = np.repeat(g[:, :, None], 3, 2)
        out[0, i] = upsample2x(unit_bytes(hm_pred[z])).astype(np.uint8)[:, :, None]
        out[1, i] = blend(g, upsample2x(unit_bytes(hm_gt[z])))[:, :, None]
        out[2, i] = grey
        out[3, i] = grey
        draw_rings(out[2, i], [(int(r[0]), int(r[1])) for r in pred_dets if r[4] > thr and int(r[2]) == z], radius)
        draw_rings(out[3, i], [(int(r[0]), int(r[1])) for r in gt_dets if int(r[2]) == z], radius)
    return out
