"""Float64 numpy restatements of csrc/class_gallery.hip and small inputs for them.  Nothing of this is in the
reference project: these restatements, checked against numpy's own mean, std and stable argsort in test_class_gallery_cpu.py, are
what the kernels are held to.

    moments(patches, labels, k)                          -> mean, std (k, h, w) float64, count (k,) int32
    exemplars(emb, centroids, assign, labels, k, m)      -> idx (k, m) int32 (-1 padded), d2 (k, m) float64 (+inf padded)
    row_order(count)                                     -> (k,) int32: descending count, ascending class among equal counts
    raster(mean, std, count, idx, patches, m_show, scale) -> (H, W, 3) uint8: the bytes of the picture
"""
import numpy as np

CHUNK = 256                                # members per partial sum in the kernels (GAL_CHUNK)
PAD, GLYPH_PX, DIGIT_PITCH, TEXT_W, LINE_H, LINE_GAP, TEXT_H = 4, 2, 12, 94, 14, 4, 32
DIGITS_5X7 = np.array([                    # 7 rows of 5 bits per digit, bit 4 the left pixel
    [0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E], [0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E],
    [0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F], [0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E],
    [0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02], [0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E],
    [0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E], [0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08],
    [0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E], [0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C]], np.uint8)


def moments(patches, labels, k):
    """Two passes in float64: the mean, then the squared distances from it, both divided by the count; zeros for an empty class."""
    x = np.asarray(patches, np.float64)
    labels = np.asarray(labels)
    mean, std = np.zeros((k,) + x.shape[1:]), np.zeros((k,) + x.shape[1:])
    count = np.zeros(k, np.int32)
    for c in range(k):
        members = x[labels == c]
        count[c] = len(members)
        if len(members):
            mean[c] = members.sum(0) / len(members)
            std[c] = np.sqrt(((members - mean[c]) ** 2).sum(0) / len(members))
    return mean, std, count


def distances(emb, centroids, assign):
    """d2 (n,) float64 = sum_j (emb[i, j] - centroids[assign[i], j])^2, j ascending, one rounding per operation (numpy's own
    sum over an axis adds in pairs, which gives other doubles)."""
    d = np.asarray(emb, np.float32).astype(np.float64) - np.asarray(centroids, np.float32).astype(np.float64)[np.asarray(assign)]
    s = np.zeros(len(d))
    for j in range(d.shape[1]):
        s = s + d[:, j] * d[:, j]
    return s


def exemplars(emb, centroids, assign, labels, k, m):
    d2 = distances(emb, centroids, assign)
    labels = np.asarray(labels)
    idx, out = np.full((k, m), -1, np.int32), np.full((k, m), np.inf)
    for c in range(k):
        members = np.flatnonzero(labels == c)
        best = members[np.lexsort((members, d2[members]))][:m]             # by distance, then by pick index
        idx[c, :len(best)], out[c, :len(best)] = best, d2[best]
    return idx, out


def row_order(count):
    count = np.asarray(count, np.int64)
    return np.lexsort((np.arange(len(count)), -count)).astype(np.int32)


def canvas(k, h, w, m_show, scale):
    row = max(h * scale, TEXT_H)
    return PAD + k * (row + PAD), 2 * PAD + TEXT_W + (2 + m_show) * (w * scale + PAD)


def grey(v, lo, span):
    """float32, every operation rounded: rint(((v - lo) / span) 255) held in 0..255; 0 where span is not positive."""
    v, lo, span = np.asarray(v, np.float32), np.float32(lo), np.float32(span)
    if not span > 0:
        return np.zeros(v.shape, np.uint8)
    with np.errstate(invalid="ignore"):
        t = np.rint(((v - lo) / span) * np.float32(255))
    assert t.dtype == np.float32
    return np.where(t >= 255, 255, np.where(t > 0, t, 0)).astype(np.uint8)


def _number(pic, value, x, y):
    for d, ch in enumerate(str(max(int(value), 0))):
        for gy in range(7):
            for gx in range(5):
                if (DIGITS_5X7[int(ch), gy] >> (4 - gx)) & 1:
                    yy, xx = y + gy * GLYPH_PX, x + d * DIGIT_PITCH + gx * GLYPH_PX
                    pic[yy:yy + GLYPH_PX, xx:xx + GLYPH_PX] = 0


def raster(mean, std, count, idx, patches, m_show, scale):
    mean, std, patches = np.asarray(mean, np.float32), np.asarray(std, np.float32), np.asarray(patches, np.float32)
    k, h, w = mean.shape
    H, W = canvas(k, h, w, m_show, scale)
    pic = np.full((H, W), 255, np.uint8)
    row = max(h * scale, TEXT_H)
    smax = np.float32(max(std.max(), 0))

    def put(r, cell, bytes_):
        y, x = PAD + r * (row + PAD), 2 * PAD + TEXT_W + cell * (w * scale + PAD)
        pic[y:y + h * scale, x:x + w * scale] = np.repeat(np.repeat(bytes_, scale, 0), scale, 1)

    for r, c in enumerate(row_order(count)):
        y = PAD + r * (row + PAD)
        _number(pic, c, PAD, y)
        _number(pic, count[c], PAD, y + LINE_H + LINE_GAP)
        put(r, 0, grey(mean[c], mean[c].min(), mean[c].max() - mean[c].min()))
        put(r, 1, grey(std[c], 0, smax))
        for e in range(m_show):
            i = idx[c, e]
            if 0 <= i < len(patches):
                put(r, 2 + e, grey(patches[i], patches[i].min(), patches[i].max() - patches[i].min()))
    return np.repeat(pic[:, :, None], 3, 2)


def case(counts, h, w, seed, offset=0.0, dim=8, k_centroids=None):
    """Picks of len(counts) classes with counts[c] members each, shuffled: patches (n, h, w) fp32 with a class-dependent mean and
    spread (plus `offset`), labels (n,) int32, and embeddings (n, dim) fp32 around centroids (k_centroids, dim) with assign (n,)."""
    rs = np.random.RandomState(seed)
    k = len(counts)
    labels = rs.permutation(np.repeat(np.arange(k), counts)).astype(np.int32)
    n = len(labels)
    patches = (rs.standard_normal((n, h, w)) * (0.5 + labels)[:, None, None] + 3 * labels[:, None, None]).astype(np.float32)
    patches = (patches + np.float32(offset)).astype(np.float32)
    kc = k if k_centroids is None else k_centroids
    centroids = (rs.standard_normal((kc, dim)) * 4).astype(np.float32)
    assign = (labels if kc == k else rs.randint(0, kc, n)).astype(np.int32)
    emb = (centroids[assign] + rs.standard_normal((n, dim))).astype(np.float32)
    return dict(patches=patches, labels=labels, emb=emb, centroids=centroids, assign=assign, k=k)
