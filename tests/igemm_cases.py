"""Case table of tests/test_igemm_gpu.py and the host rules of csrc/conv_igemm.hip restated in Python (axis_runs, build_border_classes,
dgrad_class, make_plan's tile choice): a test works out the schedule a shape should get from these and confirms it through
mi_debug_last_conv_plan.  No GPU here: tests/test_igemm_cases.py checks the rules against hand-counted shapes."""
import collections

FWD, DGRAD, WGRAD = "fwd", "dgrad", "wgrad"

_Case = collections.namedtuple("Case", "n d h w ci co k3 stride p3 d3")


def case(n, d, h, w, ci, co, k=3, stride=1, pad=None, dil=(1, 1, 1)):
    """(N, D, H, W, Ci -> Co), window k (int: cubic), stride, padding (None: k // 2 per axis), dilation."""
    k3 = (k,) * 3 if isinstance(k, int) else tuple(k)
    p3 = tuple(v // 2 for v in k3) if pad is None else ((pad,) * 3 if isinstance(pad, int) else tuple(pad))
    return _Case(n, d, h, w, ci, co, k3, stride, p3, tuple(dil))


def case_id(c):
    return "%dx%dx%dx%d_%dto%d_k%s_s%d_p%s_d%s" % (c.n, c.d, c.h, c.w, c.ci, c.co, "".join(map(str, c.k3)), c.stride,
                                                   "".join(map(str, c.p3)), "".join(map(str, c.d3)))


def out_extent(c):
    return tuple((v + 2 * p - dl * (k - 1) - 1) // c.stride + 1 for v, k, p, dl in zip((c.d, c.h, c.w), c.k3, c.p3, c.d3))


def taps(c):
    return c.k3[0] * c.k3[1] * c.k3[2]


def reduction_length(mode, c):
    """K of the GEMM: elements summed into one output value."""
    if mode == FWD:
        return taps(c) * c.ci
    if mode == DGRAD:
        return taps(c) * c.co
    do, ho, wo = out_extent(c)
    return c.n * do * ho * wo


# ---- border classes (axis_runs / build_border_classes) ---------------------------------------------------------------------------
def axis_runs(mode, n_pos, n_src, k, s, p, dl, max_runs=3):
    """Runs of consecutive row positions with one valid tap range: [(pos0, cnt, tlo, tcnt)], or None for more than max_runs."""
    runs = []
    for o in range(n_pos):
        ok = [t for t in range(k) if 0 <= (o * s - p + t * dl if mode == FWD else o + p - t * dl) < n_src]
        tlo, tcnt = (ok[0], ok[-1] - ok[0] + 1) if ok else (0, 0)
        if runs and runs[-1][2:] == (tlo, tcnt):
            runs[-1] = (runs[-1][0], runs[-1][1] + 1, tlo, tcnt)
            continue
        if len(runs) == max_runs:
            return None
        runs.append((o, 1, tlo, tcnt))
    return runs


def border_classes(mode, c, no_border=False):
    """The border classes of a forward or stride-1 data-gradient launch as [(rows per sample, taps)], heaviest first - or None where
    the host code takes the plain schedule (one input channel, strided data gradient, weight gradient, more than 3 runs on an axis,
    a single class, or more than 92 % of the multiply-adds useful)."""
    if c.ci == 1 or mode == WGRAD or (mode == DGRAD and c.stride != 1) or no_border:
        return None
    ext_in, ext_out = (c.d, c.h, c.w), out_extent(c)
    per_axis = []
    for a in range(3):
        n_pos, n_src = (ext_out[a], ext_in[a]) if mode == FWD else (ext_in[a], ext_out[a])
        r = axis_runs(mode, n_pos, n_src, c.k3[a], c.stride, c.p3[a], c.d3[a])
        if r is None:
            return None
        per_axis.append(r)
    cls = [(rz[1] * ry[1] * rx[1], rz[3] * ry[3] * rx[3]) for rz in per_axis[0] for ry in per_axis[1] for rx in per_axis[2]]
    if len(cls) < 2:
        return None
    useful = sum(r * t for r, t in cls)
    full = sum(r for r, _ in cls) * taps(c)
    if useful > 0.92 * full:
        return None
    return sorted(cls, key=lambda rt: -rt[1])         # (stable, as the host's sort)


# ---- parity classes of a strided data gradient (dgrad_class) ---------------------------------------------------------------------
def parity_classes(c):
    """[(rows, taps)] of the stride^3 classes, in class order."""
    s = c.stride
    out = []
    for cl in range(s ** 3):
        cc = (cl // (s * s), (cl // s) % s, cl % s)
        rows, t = c.n, 1
        for a, dim in enumerate((c.d, c.h, c.w)):
            f = ((cc[a] - c.p3[a]) % s + s) % s
            rows *= (dim - f + s - 1) // s if f < dim else 0
            t *= (c.k3[a] - cc[a] + s - 1) // s if cc[a] < c.k3[a] else 0
        out.append((rows, t))
    return out


def ceil_div(a, b):
    return (a + b - 1) // b


# ---- the plan (setup_conv / make_plan / launch_mode) -----------------------------------------------------------------------------
def expected_plan(mode, c, env=None):
    """The schedule fields that follow from the shape and the switches alone: bm, bn, bk, n_classes, border, fold, wbox, bf16x3,
    stem and row_tiles / col_tiles (blocks = row_tiles * col_tiles * splits).  env: the MI_CONV_* switches of the call.  The split
    count of the load model is not restated: a test that needs one sets MI_CONV_SPLITS."""
    env = env or {}
    geti = lambda name: int(env.get(name, 0) or 0)
    stem = c.ci == 1
    f32 = env.get("MI_CONV_ARITH", "")[:1] == "f"
    ncols = c.ci if mode == DGRAD else c.co
    red_ch = 0 if (mode == WGRAD or stem) else (c.ci if mode == FWD else c.co)
    bm, bn = 64, 64
    bk = 32 if red_ch % 32 == 0 else 16
    if geti("MI_CONV_BM"):
        bm = 128 if geti("MI_CONV_BM") == 128 else 64
    if geti("MI_CONV_BN"):
        bn = 128 if (geti("MI_CONV_BN") == 128 and ncols % 128 == 0) else 64
    v = geti("MI_CONV_BK")
    if v in (16, 32, 64) and (red_ch == 0 or red_ch % v == 0):
        bk = v
    if bk != 32 or stem:
        bn = 64
    if bk == 64 and (stem or bm != 128):
        bk = 32
    no_border = bool(geti("MI_CONV_NO_BORDER"))
    border = border_classes(mode, c, no_border)
    do, ho, wo = out_extent(c)
    if border is not None:
        rows = [c.n * r for r, _ in border]
        n_classes = len(border)
    elif mode == DGRAD and c.stride > 1:
        rows = [r for r, _ in parity_classes(c)]
        n_classes = len(rows)
    else:
        rows = [{FWD: c.n * do * ho * wo, DGRAD: c.n * c.d * c.h * c.w, WGRAD: taps(c) * c.ci}[mode]]
        n_classes = 1
    tiles_of = lambda m: sum(ceil_div(r, m) for r in rows)
    if (mode == FWD and not stem and ncols <= 32 and (bm, bn, bk) == (64, 64, 32) and not f32
            and env.get("MI_CONV_NARROW", "1") != "0" and tiles_of(128) >= 512):
        bm, bn = 128, 32
    bf16x3 = (not stem and not f32 and ((mode == FWD and (bm, bn, bk) == (128, 32, 32)) or ((bm, bn) == (64, 64) and bk in (16, 32))))
    wbox = int(mode == WGRAD and not stem and not no_border and border_classes(FWD, c) is not None and c.ci % bm == 0)
    return dict(bm=bm, bn=bn, bk=bk, n_classes=n_classes, border=int(border is not None),
                fold=int(n_classes > 1 and not geti("MI_CONV_NO_FOLD")), wbox=wbox, bf16x3=int(bf16x3), stem=int(stem),
                row_tiles=tiles_of(bm), col_tiles=ceil_div(ncols, bn))


PLAN_FIELDS = ("bm", "bn", "bk", "splits", "n_classes", "border", "fold", "wbox", "blocks", "bf16x3", "stem")

# ---- the cases (N, D, H, W, Ci -> Co; 3^3 window, stride 1, padding k // 2 unless said) ------------------------------------------
# A: border classes, forward and stride-1 data gradient.  (case, border expected in both passes)
BORDER = [
    (case(3, 2, 2, 2, 32, 32), 1),
    (case(2, 1, 5, 4, 64, 32), 1),                    # an axis of extent 1: one run, tlo = 1, tcnt = 1
    (case(1, 5, 6, 7, 16, 32), 1),
    (case(2, 3, 4, 2, 48, 16), 1),
    (case(2, 1, 9, 11, 32, 64, k=(1, 3, 3)), 1),      # a 2-D layer
    (case(2, 3, 3, 3, 16, 16, k=5), 1),               # 5^3 on 3^3: 3 runs per axis, all 27 classes (the table's size)
    (case(1, 4, 5, 4, 16, 16, k=5), 0),               # 5^3 on extents >= 4: more than 3 runs on an axis - the plain schedule
    (case(1, 3, 7, 6, 32, 32, pad=(1, 2, 2), dil=(1, 2, 2)), 1),
    (case(1, 1, 16, 16, 32, 32, k=(1, 3, 3)), 1),     # the 0.92 rule: 0.918 of the multiply-adds useful ...
    (case(1, 1, 17, 17, 32, 32, k=(1, 3, 3)), 0),     # ... and 0.923
]
# B: parity classes of the stride-2 data gradient
PARITY = [
    case(2, 7, 5, 6, 32, 16, stride=2),
    case(3, 4, 4, 4, 64, 128, stride=2),
    case(2, 1, 4, 3, 32, 32, stride=2),               # an extent of 1: classes without rows
    case(2, 4, 5, 6, 64, 128, k=1, stride=2),         # seven of eight classes without taps: their rows are exactly zero
    case(3, 4, 4, 4, 32, 32, k=2, stride=2, pad=0),
    case(1, 9, 8, 10, 16, 16, k=7, stride=2),
]
# C: weight gradient.  (case, switches, wbox expected)
WBOX = [
    (case(2, 3, 4, 5, 64, 32), {}, 1),
    (case(2, 3, 4, 5, 128, 16), {}, 1),
    (case(2, 3, 4, 5, 16, 32), {}, 0),
    (case(2, 3, 4, 5, 32, 16), {}, 0),
    (case(2, 3, 4, 5, 48, 32), {}, 0),
    (case(2, 1, 6, 5, 64, 32), {}, 1),                # taps a = 0 and a = 2 never meet the input: an empty box, dw exactly zero
    (case(3, 5, 6, 7, 64, 64, stride=2), {}, 1),
    (case(1, 3, 7, 6, 64, 32, pad=(1, 2, 2), dil=(1, 2, 2)), {}, 1),
    (case(2, 3, 4, 5, 64, 32), {"MI_CONV_BM": "128"}, 0),     # a 128-row tile spans two taps: declined by Ci % BM
    (case(2, 3, 4, 5, 128, 16), {"MI_CONV_BM": "128"}, 1),
]
# D: split-K
SPLIT_LAYERS = [case(2, 4, 4, 4, 64, 64), case(2, 1, 9, 11, 32, 32, k=(1, 3, 3))]
SPLITS = (1, 2, 3, 5, 20)         # 5: no divisor of any slice count here; 20: more than the shortest reductions have slices
# E: tiles.  Rows M = N D H W: 65 and 127 (M % 64 = 1, 63), 35 (< 64)
TILE_SHAPES = [case(1, 1, 5, 13, 64, 128, k=(1, 3, 3)), case(1, 1, 1, 127, 64, 256, k=(1, 3, 3)), case(1, 1, 5, 7, 128, 128, k=(1, 3, 3))]
TILE_SWITCHES = [{}, {"MI_CONV_BM": "128"}, {"MI_CONV_BN": "128"}, {"MI_CONV_BM": "128", "MI_CONV_BN": "128"}, {"MI_CONV_BK": "16"},
                 {"MI_CONV_BK": "32"}, {"MI_CONV_BK": "64"}, {"MI_CONV_BM": "128", "MI_CONV_BK": "64"},
                 {"MI_CONV_BM": "128", "MI_CONV_BK": "16"}]
RAGGED_CHANNELS = [case(2, 3, 4, 5, 16, 48), case(2, 3, 4, 5, 48, 80), case(1, 2, 3, 5, 32, 16)]
RAGGED_SWITCHES = [{}, {"MI_CONV_BM": "128"}, {"MI_CONV_BK": "32"}]
# F: one input channel outside 7^3 stride 2
STEM = [case(n, d, h, w, 1, co, k=k, stride=s) for (n, d, h, w) in ((2, 5, 6, 7), (1, 9, 9, 9)) for k in (3, 5, 7) for s in (1, 2)
        for co in (16, 64)]
# G: fold.  (case, pass, MI_CONV_SPLITS): more than 512 blocks, no multiple of 256
FOLD = [(case(16, 8, 8, 8, 16, 16), FWD, 4), (case(16, 8, 8, 8, 16, 16), DGRAD, 4), (case(16, 8, 8, 8, 16, 16, stride=2), DGRAD, 5)]
# H: row decoding by multiply-shift
DECODE = [case(3, 11, 13, 5, 16, 16), case(2, 1, 1, 17, 16, 16)]
