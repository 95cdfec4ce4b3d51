"""torch.autograd glue over the training-path C-ABI (include/cetpick_hip.h).

Activations are channels-last fp32: 5-D (N, D, H, W, C) for volumes, 2-D (M, C) for vectors.
Weights are stored [tap][Cin][Cout]; modules expose them to state_dict() as permuted views with
the reference's logical shapes (Cout, Cin, kd, kh, kw) / (out, in).

Weight gradients are written straight into ``param.grad`` (a view of a flat gradient arena when
the model was flattened by :class:`ParamArena`): a parameter whose ``.grad`` is None gets the
gradient assigned, otherwise it is accumulated - the same contract as torch's AccumulateGrad.
PyTorch is the allocator / stream owner; all arithmetic happens in the HIP kernels.
"""
import collections
import ctypes
import math
import os
import torch
import torch.nn as nn

from . import _lib as L


PROFILE = None          # bench.py: list collecting (tag, flops, start_event, end_event, launches) per conv call
PROFILE_REPEAT = 8      # timed back-to-back launches per call (hides the eager-mode gap in front of a lone launch)


def _prof_run(tag, flops, fn):
    """Run one conv call; under bench.py's roofline pass also time PROFILE_REPEAT more launches of the same call
    (idempotent: outputs never alias inputs) between two HIP events on the launch stream."""
    fn()
    if PROFILE is not None:
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(PROFILE_REPEAT):
            fn()
        e1.record()
        PROFILE.append((tag, flops, e0, e1, PROFILE_REPEAT))


STAMPS = None           # tools/stamp_step.py: (device int64 buffer, [names]) - wall-clock stamps recorded into the step


STAMP_TAG = ""          # prefix of the stamps' names (models/moco.py labels the two encoder branches)


def stamp(name):
    """Measurement aid: a one-thread launch on the current stream that writes the 100 MHz wall clock; a no-op unless
    tools/stamp_step.py armed it.  Recorded into a captured step it times the step's phases WITHOUT a profiler attached."""
    if STAMPS is None:
        return
    buf, names = STAMPS
    if len(names) >= buf.numel():
        raise L.HipExtensionError("stamp buffer full")
    L.call("mi_debug_stamp", buf.data_ptr() + 8 * len(names))
    names.append(STAMP_TAG + name)


def _ws(nbytes, device, tag):
    return L.workspace(max(int(nbytes), 256), device, tag)


def _f32c(t, name):
    L.require_cuda(t, name)
    if not t.is_contiguous():
        raise L.HipExtensionError(name + " must be contiguous (channels-last storage)")
    return t


# ------------------------------------------------------------------------------------------------
# parameter plumbing
# ------------------------------------------------------------------------------------------------
def conv_weight_param(co, ci, k, device=None):
    """Parameter with logical shape (co, ci, k, k, k) over physical storage [k,k,k,ci,co]."""
    phys = torch.empty(k, k, k, ci, co, device=device)
    return nn.Parameter(phys.permute(4, 3, 0, 1, 2))


def linear_weight_param(out_f, in_f, device=None):
    """Parameter with logical shape (out, in) over physical storage [in][out]."""
    phys = torch.empty(in_f, out_f, device=device)
    return nn.Parameter(phys.t())


def _phys_ok(p):
    """True when the parameter's strides are the kernel layout (co fastest, then ci, then taps)."""
    if p.dim() == 5:
        co, ci, kd, kh, kw = p.shape
        return p.stride() == (1, co, kh * kw * ci * co, kw * ci * co, ci * co)
    if p.dim() == 4:
        co, ci, kh, kw = p.shape
        return p.stride() == (1, co, kw * ci * co, ci * co)
    if p.dim() == 2:
        out_f, in_f = p.shape
        return p.stride() == (1, out_f)
    return p.is_contiguous()


def _dense_layout(p):
    """True when the tensor's strides are a permutation of a contiguous layout (every element of a numel-sized storage
    block is addressed exactly once): such a parameter can live in a flat arena under its own strides."""
    exp = 1
    for st, sz in sorted((st, sz) for st, sz in zip(p.stride(), p.shape) if sz != 1):
        if st != exp:
            return False
        exp *= sz
    return True


def _grad_target(param):
    """(tensor to write into, accumulate?) for a parameter's gradient."""
    g = param.grad
    if g is None:
        view = getattr(param, "_mi_grad_view", None)
        if view is None:
            view = torch.empty_like(param)        # preserve_format keeps the kernel layout
        param.grad = view
        return view, False
    view2 = getattr(param, "_mi_grad_view2", None)
    if view2 is not None and not param._mi_grad2_used:
        # the second contribution of a step (a two-view model: SimSiamStepEngine) goes into the second gradient arena - the optimizer
        # kernel adds the two - instead of through a temporary and a grad.add_ launch per parameter
        param._mi_grad2_used = True
        return view2, False
    if g.stride() != param.stride():
        raise L.HipExtensionError("param.grad layout differs from the parameter's kernel layout")
    return g, True


class _GradInto:
    """Where the launch that computes `param`'s gradient writes: `with _GradInto(param) as tgt:` around the launch.  The target is
    decided when the object is MADE (_grad_target: .grad itself, the second arena or, for a gradient that accumulates, a temporary) -
    a launch deferred through _side_or_now makes the object where autograd reaches the layer and enters it inside the closure;
    leaving the block adds the temporary onto .grad.  param None (a gradient nobody asked for): tgt is None, the kernels' null pointer."""
    __slots__ = ("grad", "tgt")

    def __init__(self, param):
        self.grad = self.tgt = None
        if param is not None:
            self.grad, acc = _grad_target(param)
            self.tgt = torch.empty_like(self.grad) if acc else self.grad

    @property
    def accumulates(self):
        return self.tgt is not self.grad

    def __enter__(self):
        return self.tgt

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None and self.tgt is not self.grad:
            self.grad.add_(self.tgt)
        return False


class ParamArena:
    """Flatten a module's parameters (and their gradients) into two contiguous fp32 arenas so the
    momentum update (models/moco.py:31-39), SGD (moco_main.py:79) and the gradient all-reduce are
    single passes.  Parameters keep their identity, logical shapes and kernel strides."""

    def __init__(self, module, second_grad_arena=False):
        params = [p for p in module.parameters()]
        if not params:
            raise ValueError("module has no parameters")
        dev = params[0].device
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4          # keep every view 16-B aligned
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.params, self.offsets = params, offs
        for p, o in zip(params, offs):
            if not _dense_layout(p):
                raise L.HipExtensionError("parameter %s is not densely laid out" % (tuple(p.shape),))
            view = torch.as_strided(self.flat, p.shape, p.stride(), o)
            view.copy_(p.data)
            p.data = view
            p._mi_grad_view = torch.as_strided(self.flat_grad, p.shape, p.stride(), o)
            p.grad = None
        self.numel = total
        # a second gradient arena for models that apply every parameter twice per step (the two views of SimSiam): see _grad_target
        self.flat_grad2 = None
        if second_grad_arena:
            self.flat_grad2 = torch.zeros(total, dtype=torch.float32, device=dev)
            for p, o in zip(params, offs):
                p._mi_grad_view2 = torch.as_strided(self.flat_grad2, p.shape, p.stride(), o)
                p._mi_grad2_used = False
        else:
            self.drop_second_grads()               # views an earlier two-arena owner left behind would take every second contribution

    def drop_second_grads(self):
        """Remove the second-gradient views from the parameters: _grad_target accumulates a second contribution into .grad again."""
        for p in self.params:
            p.__dict__.pop("_mi_grad_view2", None)
            p.__dict__.pop("_mi_grad2_used", None)

    def attach_grads(self):
        for p in self.params:
            p.grad = p._mi_grad_view

    def zero_grad(self):
        """set_to_none semantics: the next backward overwrites the arena views."""
        for p in self.params:
            p.grad = None
        if self.flat_grad2 is not None:
            for p in self.params:
                p._mi_grad2_used = False

    def settle_grads(self):
        """After a backward pass, before a kernel reads the flat arenas: a parameter the pass did not reach (or reached once, with two
        arenas) holds last step's values there - zero it.  (No launch when every parameter was reached, the usual case.)"""
        for p in self.params:
            if p.grad is None:
                p._mi_grad_view.zero_()
            elif p.grad.data_ptr() != p._mi_grad_view.data_ptr():
                p._mi_grad_view.copy_(p.grad)
            if self.flat_grad2 is not None and not p._mi_grad2_used:
                p._mi_grad_view2.zero_()


class GradExchange:
    """Data-parallel gradient exchange for a module trained with a stock optimizer (main.py:34-56, simsiam_main.py:
    the reference wraps the model in DistributedDataParallel): the parameters are re-homed in one flat fp32 arena, the
    backward pass writes their gradients into a second arena, and `sync()` - between `backward()` and
    `optimizer.step()` - averages that arena over the ranks with a few large asynchronous all-reduces (RCCL over xGMI:
    bucket = a quarter of the arena, >= 1 Mi floats) instead of one collective per tensor.  SyncBN statistics are
    exchanged by the BatchNorm modules themselves (convert_sync_batchnorm)."""

    def __init__(self, module, n_buckets=4):
        import torch.distributed as dist
        self.dist = dist
        self.world = dist.get_world_size()
        self.arena = ParamArena(module)
        n = self.arena.numel
        per = max((n + n_buckets - 1) // n_buckets, 1 << 20)
        per = (per + 3) // 4 * 4
        self.buckets = [(a, min(a + per, n)) for a in range(0, n, per)]
        self.calls = 0

    def sync(self):
        for prm in self.arena.params:
            view = prm._mi_grad_view
            if prm.grad is None:
                view.zero_()                       # a parameter the step did not reach contributes zeros
            elif prm.grad.data_ptr() != view.data_ptr():
                view.copy_(prm.grad)               # gradient produced outside the arena (plain autograd)
            prm.grad = view
        pending = [self.dist.all_reduce(self.arena.flat_grad[a:b], async_op=True) for a, b in self.buckets]
        for w in pending:
            w.wait()
        self.arena.flat_grad.mul_(1.0 / self.world)
        self.calls += 1

    def broadcast_parameters(self, src=0):
        """identical replicas before the first step (DistributedDataParallel does this at construction)"""
        self.dist.broadcast(self.arena.flat, src)


# ------------------------------------------------------------------------------------------------
# conv / linear
# ------------------------------------------------------------------------------------------------
def conv2d_weight_param(co, ci, k, device=None):
    """Parameter with logical shape (co, ci, k, k) over physical storage [k,k,ci,co]."""
    phys = torch.empty(k, k, ci, co, device=device)
    return nn.Parameter(phys.permute(3, 2, 0, 1))


def _k3(k, nd5):
    """int or tuple -> (kd, kh, kw); 2-D activations (N,H,W,C) use kd = 1."""
    if isinstance(k, (tuple, list)):
        return tuple(int(v) for v in k) if len(k) == 3 else (1, int(k[0]), int(k[1]))
    return (int(k),) * 3 if nd5 else (1, int(k), int(k))


def _p3(p, nd5):
    if isinstance(p, (tuple, list)):
        return tuple(int(v) for v in p) if len(p) == 3 else (0, int(p[0]), int(p[1]))
    return (int(p),) * 3 if nd5 else (0, int(p), int(p))


def _as5d(x):
    """(N,H,W,C) -> (N,1,H,W,C) view; 5-D passes through."""
    return x if x.dim() == 5 else x.unsqueeze(1)


def _out_extent(extent, k3, stride, p3, d3):
    return tuple((v + 2 * p - dl * (k - 1) - 1) // stride + 1 for v, k, p, dl in zip(extent, k3, p3, d3))


class _Geom:
    """One convolution problem - (N, D, H, W, Ci) -> co channels, window k3, stride, padding p3, dilation d3 (None: none) - as the
    C-ABI takes it: the mi_conv_geom struct built once (`ref` is what the mi_conv_* entries get), the output extent, the tap count of
    the FLOP tags and a hashable key."""
    __slots__ = ("key", "c", "ref", "out", "taps")

    def __init__(self, shape5, co, k3, stride, p3, d3=None):
        d3 = (1, 1, 1) if d3 is None else tuple(d3)
        self.key = tuple(int(v) for v in shape5) + (int(co),) + tuple(k3) + (int(stride),) + tuple(p3) + d3
        self.c = L.ConvGeom(*self.key)
        self.ref = ctypes.byref(self.c)
        self.out = _out_extent(shape5[1:4], k3, stride, p3, d3)
        self.taps = k3[0] * k3[1] * k3[2]

    def workspace(self, device):
        return _ws(L.lib().mi_conv_workspace_bytes(self.ref), device, "conv")


def _linear_geom(m, ci, co):
    """nn.Linear on m rows: the 1 x 1 x 1 convolution of m one-voxel volumes."""
    return _Geom((m, 1, 1, 1, ci), co, (1, 1, 1), 1, (0, 0, 0))


# Pre-cut weight images of the conv_s2.hip / conv_direct3.hip / conv_p2d.hip convolutions.  Outside a step engine an image is cut in
# front of its convolution (by the C side, or on the parameter: _kept_image); a step engine (trains/step_graph.py) knows when its weights
# change, keeps them here and re-cuts a whole group in ONE launch per family.  The cache is only consulted while ACTIVE_IMAGES is set
# (the engine sets it around its step), so a stale image can never reach a convolution issued from anywhere else.
ACTIVE_IMAGES = None

_ImageFamily = collections.namedtuple("_ImageFamily", ("nbytes", "prep"))      # image size (lib, weight, dgrad flag), prep entry
# (in the order a refresh cuts them)
_IMAGE_FAMILIES = {
    # the stride-2 block fronts: image of (conv1.weight, downsample weight), forward or data gradient
    "s2": _ImageFamily(lambda lib, w, dgrad: (lib.mi_conv3d_s2_dgrad_workspace_bytes if dgrad else lib.mi_conv3d_s2_fwd_workspace_bytes)(
        int(w.shape[1]), int(w.shape[0])), "mi_conv3d_s2_prep"),
    # the 3-D 3^3 / stride-1 C -> C layers
    "direct": _ImageFamily(lambda lib, w, dgrad: lib.mi_conv3d_direct_wimg_bytes(int(w.shape[0])), "mi_conv3d_direct_prep"),
    # the 2-D 3 x 3 / stride-1 C -> C layers
    "p2d": _ImageFamily(lambda lib, w, dgrad: lib.mi_conv2d_p2d_wimg_bytes(int(w.shape[0])), "mi_conv2d_p2d_prep"),
}


def _prep_images(family, items):
    """items: [(weight, shortcut weight of an "s2" front or None, dgrad flag, image tensor)] - all cut by the family's prep entry (one
    launch for the s2 fronts, one per 16 images otherwise) on the current stream."""
    if not items:
        return
    fn = _IMAGE_FAMILIES[family].prep
    ints = lambda vals: L.host_array(vals, ctypes.c_int)
    w, img = L.host_array([it[0].data_ptr() for it in items]), L.host_array([it[3].data_ptr() for it in items])
    dgrad, co = ints([it[2] for it in items]), ints([int(it[0].shape[0]) for it in items])
    if family == "s2":               # two more operand arrays: the shortcut weights and the input channels
        args = (w, L.host_array([(it[1].data_ptr() if it[1] is not None else None) for it in items]), img,
                ints([int(it[0].shape[1]) for it in items]), co, dgrad)
    else:
        args = (w, img, dgrad, co)
    L.call(fn, *args, len(items))


class WeightImages:
    def __init__(self):
        self._groups = {}            # group -> {family: [(weight, shortcut weight of an "s2" front or None, dgrad flag, image)]}
        self._by_weight = {}         # (family, weight storage address, dgrad flag) -> image tensor

    @staticmethod
    def eligible(w, k, stride, pad):
        return (w.is_cuda and tuple(w.shape[:2]) in ((64, 64), (128, 128)) and _k3(k, True) == (3, 3, 3) and stride == 1
                and _p3(pad, True) == (1, 1, 1) and _phys_ok(w))

    def add(self, group, family, w, dgrad, w_ds=None):
        """Keep the `family` image of `w` (with the shortcut weight `w_ds` of an "s2" front) for the forward or data-gradient pass."""
        dgrad = int(bool(dgrad))
        img = torch.empty(int(_IMAGE_FAMILIES[family].nbytes(L.lib(), w, dgrad)), dtype=torch.uint8, device=w.device)
        self._groups.setdefault(group, {f: [] for f in _IMAGE_FAMILIES})[family].append((w, w_ds, dgrad, img))
        self._by_weight[(family, w.data_ptr(), dgrad)] = img

    def get(self, family, w, dgrad):
        return self._by_weight.get((family, w.data_ptr(), int(bool(dgrad))))

    def refresh(self, group):
        """Re-cut every image of `group` from the current weights on the current stream: one launch for the group's stride-2
        fronts, one (per 16 images) for its direct-kernel images, one for its p2d images."""
        for family, items in self._groups.get(group, {}).items():
            _prep_images(family, items)

    def refresh_all(self):
        for group in self._groups:              # (in registration order)
            self.refresh(group)

    def versions(self):
        """Sum of the torch version counters of the cached weights: changes when anything but the engine's own kernels
        (which refresh by themselves) wrote a weight."""
        return sum(it[0]._version + (it[1]._version if it[1] is not None else 0)
                   for g in self._groups.values() for items in g.values() for it in items)


def _held_image(w, dgrad):
    """(family, image) of the image the active step engine keeps of `w` for this pass; (None, None) without one."""
    if ACTIVE_IMAGES is not None:
        for family in _IMAGE_FAMILIES:
            img = ACTIVE_IMAGES.get(family, w, dgrad)
            if img is not None:
                return family, img
    return None, None


def _switch(name):
    """An environment switch of the routing, read per call (tests and A/B runs flip them between calls).  MI_CONV_ARITH (conv_igemm.hip
    conv_arith_bf16x3) is on when it selects the f32 MFMA path: anything starting with 'f'; the others when set to anything."""
    value = os.environ.get(name, "")
    return value.startswith("f") if name == "MI_CONV_ARITH" else bool(value)


def _arith_bf16x3():
    return not _switch("MI_CONV_ARITH")


SMALLK = os.environ.get("CETPICK_SMALLK", "1") != "0"

# Bumped by every kernel that writes parameters through raw pointers (sgd_step_, ema_update_: torch's version counters do
# not see those writes).  Part of the key of every cached derivative of a weight (conv_smallk images, folded BatchNorm).
WEIGHT_EPOCH = 0


def _bump_weight_epoch():
    global WEIGHT_EPOCH
    WEIGHT_EPOCH += 1


def _kept_image(holder, slot, w, geom, cut):
    """`cut(previous image or None)`'s image of the weights `w`, kept as `holder.<slot>` and cut again when the storage, holder's version
    (torch ops), WEIGHT_EPOCH (raw-pointer writes) or the geometry `geom` moved: the staleness rule of every lazily cut weight image."""
    key = (w.data_ptr(), holder._version, WEIGHT_EPOCH) + geom
    ent = getattr(holder, slot, None)
    if ent is None or ent[0] != key:
        ent = (key, cut(ent[1] if ent is not None else None))
        try:
            setattr(holder, slot, ent)
        except AttributeError:
            pass
    return ent[1]


def inference_mode():
    """True when the CALLER runs without autograd.  To be evaluated where the user's grad mode is visible - a module's
    forward, never inside an autograd.Function (grad mode is always off in there) - and handed down explicitly."""
    return not torch.is_grad_enabled()


def _smallk_image(w, owner, K, co):
    """The weight image of conv_smallk.hip for the kernel-layout weights `w` (a (K, co) matrix in memory), kept on `owner` (the
    parameter or folded-weight tensor that outlives the call) and rebuilt when the storage or its version changes."""
    lib = L.lib()
    def cut(_):
        img = torch.empty(int(lib.mi_smallk_image_bytes(K, co)), dtype=torch.uint8, device=w.device)
        L.call("mi_smallk_prep", w, img, K, co)
        return img
    return _kept_image(owner if owner is not None else w, "_mi_smallk", w, (K, co), cut)


POOL_FUSED = os.environ.get("CETPICK_POOL_FUSED", "1") != "0"


def _kernel_layout(w):
    if not _phys_ok(w):
        raise L.HipExtensionError("conv weight is not in kernel layout [tap][Cin][Cout]")


def _out_tensor(out, shape, x, sliced=False, who=""):
    """(out, channel stride): `out` checked - or made, when None - as the fp32 result of `shape` on x's device.  Dense, or (sliced) a channel
    slice of a wider contiguous tensor: the concatenation buffer of the up-convolution block that will consume it."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=x.device), shape[-1]
    ok = tuple(out.shape) == shape and out.dtype == torch.float32 and out.device == x.device
    if not sliced:
        if not (ok and out.is_contiguous()):
            raise L.HipExtensionError(who + "`out` must be a contiguous fp32 %s tensor on %s" % (shape, x.device))
        return out, shape[-1]
    cstride, want = int(out.stride(-2)), [1]
    for v in reversed(shape[1:-1]):
        want.insert(0, want[0] * v)
    if (not ok or tuple(out.stride()) != tuple(cstride * v for v in want) + (1,) or cstride < shape[-1] or cstride % 4
            or out.data_ptr() % 16):
        raise L.HipExtensionError("`out` must be an fp32 %s tensor or a channel slice of a wider contiguous one" % (shape,))
    return out, cstride


def _d32_launch(route, x, w, bias, relu, owner=None, out=None, pool=False):
    """y = act(conv(x, w) + bias) on conv_d32.hip; the pre-cut weight image is kept on `owner` (rebuilt when the weights change)."""
    kind = route.param
    lib = L.lib()
    x5 = _as5d(x)
    n, d, h, wd, ci = x5.shape
    ntap = 27 if kind == 2 else 1 if kind == 4 else 9
    co = int(w.shape[0]) if kind in (3, 4) else 32
    def cut(_):
        if kind == 3 or (kind == 4 and co >= 64):
            img = torch.empty((co // 64) * int(lib.mi_conv_d64_image_bytes(ci, ntap)), dtype=torch.uint8, device=w.device)
            L.call("mi_conv_d64_prep_co", w, img, ci, co, ntap)
        else:
            img = torch.empty(int(lib.mi_conv_d32_image_bytes(ci, ntap)), dtype=torch.uint8, device=w.device)
            L.call("mi_conv_d32_prep", w, img, ci, ntap)
        return img
    wimg = _kept_image(owner if owner is not None else w, "_mi_d32", w, (ci, ntap, co), cut)
    out, cstride = _out_tensor(out, tuple(x.shape[:-1]) + (co,), x, sliced=pool)
    if pool:                                          # kinds 1 / 3: the 2 x 2 max-pool of the result as a second output
        pooled = torch.empty(tuple(x.shape[:-3]) + (h // 2, wd // 2, co), dtype=torch.float32, device=x.device)
        L.call("mi_conv_d32_fwd_pool_strided_f32", x, wimg, bias, out, cstride, pooled, int(relu), n, d, h, wd, ci, co)
        return out, pooled
    # kind 4: 1 x 1, tile-resident; 3: 3 x 3 per plane to 64-column blocks; 1 / 2: to 32 channels (2: the dilated 3-D head)
    fn = {4: "mi_conv_d32_1x1_fwd_f32", 3: "mi_conv_d64_fwd_f32"}.get(kind, "mi_conv_d32_fwd_f32")
    def call():
        return L.call(fn, x, wimg, bias, out, int(relu), n, d, h, wd, ci, co if kind in (3, 4) else kind)
    _prof_run("fwd", 2.0 * n * d * h * wd * co * ci * ntap, call)
    return out


HEADS_FUSED = os.environ.get("CETPICK_HEADS_FUSED", "1") != "0"


def detector_heads_fused(v, proj, hm):
    """(normalize(proj(v)), hm(v)) for the detector's heads at inference in ONE pass over the feature volume v (N, D, H, W, C) - or None
    when the pair is not the one conv_smallk.hip's head kernel takes (proj: HipConvNd(C, 32, (3,1,1), padding (1,0,0)), hm: HipZHead(C,
    K <= 4); unet_small.py:86-97).  The caller has established inference (no gradient)."""
    if not (HEADS_FUSED and SMALLK and v.is_cuda and v.dim() == 5 and _arith_bf16x3()):
        return None
    if not (isinstance(proj, HipConvNd) and isinstance(hm, HipZHead)):
        return None
    n, d, h, wd, c = v.shape
    if (proj.co != 32 or proj.ci != c or tuple(proj.k) != (3, 1, 1) or tuple(proj.pad) != (1, 0, 0) or tuple(proj.dil) != (1, 1, 1)
            or hm.c != c or not 1 <= hm.k_out <= 4 or c % 16 or 3 * c > 512 or v.numel() * 4 >= 0x7fff0000
            or not _phys_ok(proj.weight) or not hm.weight.permute(2, 3, 4, 1, 0).is_contiguous()):
        return None
    _f32c(v, "v")
    img = _smallk_image(proj.weight, None, 3 * c, 32)
    m = n * d * h * wd
    y = torch.empty((n, d, h, wd, 32), dtype=torch.float32, device=v.device)
    yh = torch.empty((n, d, h, wd, hm.k_out), dtype=torch.float32, device=v.device)
    L.call("mi_smallk_heads_fwd_f32", v, img, y, hm.weight, yh, hm.k_out, m, c, h * wd, d)
    return y, yh


def _smallk_launch(route, x, w, bias, relu, owner=None, out=None):
    """The short-reduction inference kernel (conv_smallk.hip): a 1 x 1 / (3, 1, 1) convolution as route.param taps, no tile pipeline."""
    ntaps = route.param
    ci, co = x.shape[-1], w.shape[0]
    m = x.numel() // ci
    out, _ = _out_tensor(out, tuple(x.shape[:-1]) + (co,), x)
    img = _smallk_image(w, owner, ntaps * ci, co)
    plane, d = (x.shape[2] * x.shape[3], x.shape[1]) if ntaps == 3 else (1, 1)
    def call():
        return L.call("mi_smallk_fwd_f32", x, img, bias, out, int(relu), m, ci, co, ntaps, plane, d)
    _prof_run("fwd", 2.0 * m * co * ci * ntaps, call)
    return out


def p2d_usable(x_shape, ci, co, k3, stride, p3, dil=None):
    """True when conv_p2d.hip takes this 2-D convolution (forward of x / data gradient onto x): (N, H, W, C) -> C channels, 3 x 3,
    stride 1, padding 1, (W, C) one of the SimSiam 2-D encoder's three at --bbox 36."""
    if len(x_shape) != 4 or ci != co or tuple(k3) != (1, 3, 3) or stride != 1 or tuple(p3) != (0, 1, 1) or dil is not None:
        return False
    if not _arith_bf16x3():
        return False
    n, h, w, _ = x_shape
    return bool(L.lib().mi_conv2d_p2d_usable(int(n), int(h), int(w), int(ci)))


# Which kernel family a convolution takes: the family from a closed set and the family's parameter - the conv_d32.hip kind (1: 3 x 3 per
# plane to 32 channels, 2: the dilated 3-D head, 3: 3 x 3 per plane to 64-column blocks, 4: 1 x 1), the conv_smallk.hip taps (1 / 3),
# 1 where a "p2d" / "s2" launch reads the image the step engine keeps (0: it cuts its own), 1 where a "generic" weight gradient leaves
# its split-K slabs with the parameter (the deferred form: _WgradJob).  family None: declined - the caller has another way.
Route = collections.namedtuple("Route", ("family", "param"))
ROUTE_FAMILIES = ("d32", "smallk", "stem3", "stem2d", "p2d", "direct", "cube2", "s2", "generic", None)


def conv_route(pass_, shape, ci, co, k3, stride, p3, d3=None, *, inference=False, has_res=False, has_bias=False, relu=False, pool=False,
               image=None, profile=False, shortcut=False, phys_ok=True, accumulates=False, deferred=False, side=False):
    """The Route of one convolution call, from integers and flags alone (the library's *_usable / *_kind predicates need no device): every
    eligibility rule of conv_fwd, conv_bias_fwd, conv_dgrad, conv_wgrad_into and the stride-2 block fronts, each once, in their order
    of precedence.
    pass_: "fwd" / "dgrad" / "wgrad"; shape: the activation on the convolution's input side, (N, D, H, W, Ci) or (N, H, W, Ci); d3: the
    dilation, None when the caller gave none.  inference: the caller's word that no gradient will be asked (inference_mode()); has_res /
    has_bias / relu: the epilogue; pool: the 2 x 2 max-pool as a second output is asked for (declined unless conv_d32.hip makes it);
    image: the family of the image ACTIVE_IMAGES holds for this weight and pass (_held_image); profile: bench.py's roofline pass is
    on; shortcut: a block's stride-2 front with its 1 x 1 shortcut in one launch is asked for (declined unless conv_s2.hip takes it);
    phys_ok: the weights are in kernel layout (where the caller does not insist on it); accumulates / deferred / side (weight gradient): the
    gradient is added to an existing one, DEFERRED_WGRADS / SIDE_WGRADS are collecting."""
    lib = L.lib()
    nd5 = len(shape) == 5
    n, d, h, wd = (shape[0], shape[1], shape[2], shape[3]) if nd5 else (shape[0], 1, shape[1], shape[2])
    k3, p3 = tuple(k3), tuple(p3)
    dd = tuple(d3) if d3 is not None else (1, 1, 1)
    bf16x3 = _arith_bf16x3()
    if shortcut:
        # a BasicBlock's stride-2 front, cubic, one of the encoder's two shapes (csrc/conv_s2.hip)
        usable = lib.mi_conv3d_s2_fwd_usable if pass_ == "fwd" else lib.mi_conv3d_s2_dgrad_usable
        if nd5 and d == h == wd and phys_ok and usable(n, d, ci, co):
            return Route("s2", int(image == "s2" and not profile))
        return Route(None, 0)
    if pass_ == "fwd" and inference and not has_res and stride == 1:
        kind = 0                                      # conv_d32.hip's direct inference kernels: padding = dilation * (k - 1) / 2
        if ((co == 32 or (co % 64 == 0 and 64 <= co <= 512)) and bf16x3
                and p3 == tuple(dl * (k - 1) // 2 for dl, k in zip(dd, k3))):
            kind = int(lib.mi_conv_d32_kind(n, d, h, wd, ci, co, *k3, *dd))
        if pool:
            # (y, maxpool2x2(y)) in one launch where the patch-resident 2-D kernel runs and nothing else asks for the result elsewhere
            return Route("d32", kind) if (kind in (1, 3) and POOL_FUSED and not profile and not nd5) else Route(None, 0)
        if kind == 4:                                 # 1 x 1 (the transposed convolutions' products): the tile-resident kernel
            return Route("d32", 4)
        # short reduction: no tile pipeline (conv_smallk.hip).  At most 64 output channels: every wave streams the whole weight image of its
        # columns, which beyond that outweighs the activations it reads (measured: the transposed convolutions' products to 128 - 512
        # columns are 20 % slower than on the implicit GEMM)
        if (SMALLK and dd == (1, 1, 1) and not (ci % 16 or co % 32 or co > 64 or n * d * h * wd * ci * 4 >= 0x7fff0000)):
            if k3 == (1, 1, 1) and p3 == (0, 0, 0):
                return Route("smallk", 1)
            if nd5 and k3 == (3, 1, 1) and p3 == (1, 0, 0) and 3 * ci <= 512:
                return Route("smallk", 3)
        if kind:                                      # 3 x 3: the patch-resident direct kernel
            return Route("d32", kind)
    if pool:
        return Route(None, 0)
    if has_bias:
        # the detector's first layer: one input channel - a direct kernel instead of 49 single-float gathers per row
        stem2d = (ci == 1 and co == 16 and d == 1 and k3 == (1, 7, 7) and stride == 2 and p3 == (0, 3, 3) and n <= 65535
                  and not _switch("MI_NO_STEM2D"))
        return Route("stem2d" if stem2d else "generic", 0)
    # Conv2d(1, co, 3, padding=1) on its own kernels (conv_p2d.hip stem3_*): co a multiple of 4 that divides the block evenly
    if (pass_ != "dgrad" and not nd5 and ci == 1 and k3 == (1, 3, 3) and stride == 1 and p3 == (0, 1, 1) and d3 is None
            and not has_res and not relu and phys_ok
            and 4 <= co <= 64 and co % 4 == 0 and 256 % (co // 4) == 0 and not _switch("MI_NO_P2D")):
        return Route("stem3", 0)
    if not nd5 and p2d_usable(shape, ci, co, k3, stride, p3, d3):
        # the 2-D encoder's 3 x 3 / stride-1 layers; their weight gradient reads voxel-major operands through the transposing LDS read
        if pass_ != "wgrad":
            return Route("p2d", int(image == "p2d" and not profile))
        if phys_ok and not _switch("MI_NO_P2D_WGRAD") and lib.mi_conv2d_p2d_wgrad_workspace_bytes(n, h, wd, ci):
            return Route("p2d", 0)
    if pass_ == "wgrad":
        # the slab form (a _WgradJob that writes the gradient itself and leaves its split-K slabs to a batched reduce): always inside a step
        # engine's backward pass, else where run_wgrad_jobs can batch the layer (conv_direct3.hip's shapes) at the end of the pass.  Under
        # bench.py's roofline pass only the jobs the engine will queue take it - run_wgrad_jobs times them group by group -, everything else
        # is timed call by call
        rows = n * int(math.prod(_out_extent((d, h, wd), k3, stride, p3, dd)))
        slab = (not accumulates and dd == (1, 1, 1) and (not profile or (deferred and side and rows <= SIDE_ROWS_MAX))
                and (deferred or (WGRAD_BATCH and k3[0] == k3[1] == k3[2] and p3[0] == p3[1] == p3[2]
                                  and lib.mi_conv3d_direct_usable(n, d, h, wd, ci, co, k3[0], stride, p3[0]) in (1, 2))))
        return Route("generic", int(slab))
    # (a forward call's all-ones dilation is none; a data gradient's counts as one: HipConvNd's layers stay on the generic entry there)
    if nd5 and (d3 is None or (pass_ == "fwd" and dd == (1, 1, 1))) and k3 == (3, 3, 3) and p3 == (1, 1, 1) and bf16x3:
        # the direct kernels are bf16x3 only: an f32 A/B run keeps every conv on the f32 MFMA
        if image == "direct" and not profile and stride == 1 and lib.mi_conv3d_direct_usable(n, d, h, wd, co, co, 3, 1, 1):
            return Route("direct", 0)
        # 3^3 / padding 1 on a 2 x 2 x 2 volume (layer3, feature_3d): conv_cube2.hip, final in one launch (MI_CUBE2_REDUCE=1 keeps the
        # partial sums + reduce launch of mi_conv_fwd_f32 / mi_conv_dgrad_f32)
        if not _switch("MI_CUBE2_REDUCE") and lib.mi_conv3d_cube2_usable(n, d, h, wd, ci, co, 3, stride, 1):
            return Route("cube2", 0)
    return Route("generic", 0)


def _p2d_image(w, dgrad, held):
    """conv_p2d.hip's image of `w`: the one the step engine keeps (`held`), else cut on the parameter when the weights moved."""
    if held is not None:
        return held
    _kernel_layout(w)
    dgrad = int(bool(dgrad))
    def cut(old):
        img = old if (old is not None and old.device == w.device) else torch.empty(
            int(_IMAGE_FAMILIES["p2d"].nbytes(L.lib(), w, dgrad)), dtype=torch.uint8, device=w.device)
        _prep_images("p2d", [(w, None, dgrad, img)])
        return img
    return _kept_image(w, ("_mi_p2d", "_mi_p2d_dgrad")[dgrad], w, (), cut)


def _p2d_launch(route, a, w, dgrad, res, mask, relu, tag, held):
    for t, name in ((res, "res"), (mask, "mask")):
        if t is not None:
            _f32c(t, name)
    n, h, wd, c = a.shape
    out = torch.empty_like(a)
    img = _p2d_image(w, dgrad, held if route.param else None)
    def call():
        return L.call("mi_conv2d_p2d_f32", a, img, out, res, mask, int(relu), n, h, wd, c)
    _prof_run(tag, 2.0 * a.numel() * c * 9, call)
    return out


def _cube2_launch(lib, a, w, out, res, mask, relu, dgrad, n, c):
    # arrival counters in front of the partial sums: zero at allocation, left zero by every call; one buffer per stream
    ws = L.workspace(lib.mi_conv3d_cube2_workspace_bytes(n, c), a.device, "cube2", init=lambda b: b.zero_())
    def call():
        try:
            L.call("mi_conv3d_cube2_f32", a, w, out, res, mask, relu, dgrad, n, c, ws, ws.numel())
        except L.HipExtensionError:
            L.drop_workspace(a.device, "cube2")         # its counters can no longer be trusted
            raise
    return call


def _dense_launch(route, tag, g, a, w, out, res, mask, relu, held, flops, res_is_bias=0):
    """The launch of a "direct" / "cube2" / "stem2d" / "generic" route of the forward (tag "fwd": out = act(conv(a, w) + res), res a bias row
    when res_is_bias) or data-gradient pass (tag "dgrad": out = (conv_dgrad(a, w) + res) * (mask > 0)) of the geometry `g`."""
    lib = L.lib()
    n, d, h, wd, ci = g.key[:5]
    dgrad = int(tag == "dgrad")
    if route.family == "direct":                          # (the engine keeps the image current: no image build, never under PROFILE)
        ws = _ws(lib.mi_conv3d_direct_workspace_bytes(n, ci), a.device, "conv")
        L.call("mi_conv3d_direct_f32", a, held, out, res, mask, relu, n, d, h, wd, ci, ws, ws.numel())
        return out
    if route.family == "cube2":
        call = _cube2_launch(lib, a, w, out, res, mask, relu, dgrad, n, ci)
    elif route.family == "stem2d":
        def call():
            return L.call("mi_stem2d_fwd_bias_f32", a, w, res, out, relu, n, h, wd)
    else:
        ws = g.workspace(a.device)
        if dgrad:
            def call():
                return L.call("mi_conv_dgrad_f32", a, w, out, res, mask, g.ref, ws, ws.numel())
        else:
            def call():
                return L.call("mi_conv_fwd_f32", a, w, out, res, res_is_bias, relu, g.ref, ws, ws.numel())
    _prof_run(tag, flops, call)
    return out


def _conv_forward(x, w, k, stride, pad, res, bias, relu, dil, owner, inference, out, pool, who=""):
    """conv_fwd (res) and conv_bias_fwd (bias, out, pool) on one route."""
    _f32c(x, "x")
    _kernel_layout(w)
    nd5 = x.dim() == 5
    k3, p3 = _k3(k, nd5), _p3(pad, nd5)
    d3 = _k3(dil, nd5) if dil is not None else None
    ci, co = int(x.shape[-1]), int(w.shape[0])
    held_family, held = _held_image(w, False)
    route = conv_route("fwd", tuple(x.shape), ci, co, k3, stride, p3, d3, inference=inference, has_res=res is not None,
                       has_bias=bias is not None, relu=bool(relu), pool=pool, image=held_family, profile=PROFILE is not None)
    if route.family is None:
        return None
    if bias is not None:
        _f32c(bias, "bias")
    if route.family == "d32":
        return _d32_launch(route, x, w, bias, relu, owner, out, pool)
    if route.family == "smallk":
        return _smallk_launch(route, x, w, bias, relu, owner, out)
    if route.family == "stem3":
        n, h, wd, _ = x.shape
        y = torch.empty((n, h, wd, co), dtype=torch.float32, device=x.device)
        def call():
            return L.call("mi_conv2d_stem3_fwd_f32", x, w, y, n, h, wd, co)
        _prof_run("fwd", 2.0 * y.numel() * 9, call)
        return y
    if route.family == "p2d":
        return _p2d_launch(route, x, owner if owner is not None else w, False, res, None, relu, "fwd", held)
    if d3 not in (None, (1, 1, 1)) and stride != 1:
        raise L.HipExtensionError("dilated convolution needs stride 1")
    g = _Geom(_as5d(x).shape, co, k3, stride, p3, d3)
    y, _ = _out_tensor(out, (x.shape[0],) + (g.out if nd5 else g.out[1:]) + (co,), x, who=who)
    return _dense_launch(route, "fwd", g, x, w, y, res if bias is None else bias, None, int(relu), held, 2.0 * y.numel() * ci * g.taps,
                         int(bias is not None))


def conv_fwd(x, w, k, stride, pad, res=None, relu=False, dil=None, owner=None, inference=False):
    """y = act(conv(x, w) + res).  x: (N,D,H,W,Ci) or (N,H,W,Ci) channels-last; w in kernel layout.
    dil: per-axis dilation (stride 1 only).  inference: the caller ran inference_mode() where the user's grad mode is visible
    (this function is also called from autograd.Function.forward, where grad mode is always off); `owner`: the tensor that
    outlives a temporary view `w` and keeps its cached weight image."""
    return _conv_forward(x, w, k, stride, pad, res, None, relu, dil, owner, inference, None, False)


def conv_dgrad(dy, w, in_shape, k, stride, pad, res=None, mask=None, dil=None):
    _f32c(dy, "dy")
    in_shape = tuple(in_shape)
    nd5 = len(in_shape) == 5
    k3, p3 = _k3(k, nd5), _p3(pad, nd5)
    d3 = _k3(dil, nd5) if dil is not None else None
    ci, co = int(in_shape[-1]), int(w.shape[0])
    held_family, held = _held_image(w, True)
    route = conv_route("dgrad", in_shape, ci, co, k3, stride, p3, d3, has_res=res is not None, image=held_family,
                       profile=PROFILE is not None)
    if route.family == "p2d":
        return _p2d_launch(route, dy, w, True, res, mask, False, "dgrad", held)
    dx = torch.empty(in_shape, dtype=torch.float32, device=dy.device)
    g = _Geom(in_shape if nd5 else (in_shape[0], 1) + in_shape[1:], co, k3, stride, p3, d3)
    return _dense_launch(route, "dgrad", g, dy, w, dx, res, mask, 0, held, 2.0 * dy.numel() * ci * g.taps)


def conv_fwd_s2_block(x, w, w_ds):
    """Forward of a BasicBlock's stride-2 front in ONE launch (csrc/conv_s2.hip): (relu(conv(x; w, 3x3x3 stride 2 pad 1)),
    conv(x; w_ds, 1x1 stride 2)).  None when the shape is not one of the encoder's two (the caller runs the generic launches)."""
    if x.dim() != 5 or w_ds is None or not x.is_cuda:
        return None
    n, g, _, _, ci = x.shape
    co = int(w.shape[0])
    held_family, img = _held_image(w, False)
    route = conv_route("fwd", tuple(x.shape), ci, co, (3, 3, 3), 2, (1, 1, 1), image=held_family, profile=PROFILE is not None,
                       shortcut=True, phys_ok=_phys_ok(w) and _phys_ok(w_ds))
    if route.family is None:
        return None
    _f32c(x, "x")
    lib = L.lib()
    hmid = torch.empty((n, g // 2, g // 2, g // 2, co), dtype=torch.float32, device=x.device)
    r = torch.empty_like(hmid)
    if route.param:                                       # the engine keeps the image current: no image build here
        L.call("mi_conv3d_s2_fwd_img_f32", x, img, hmid, r, n, g, ci, co)
        return hmid, r
    ws = _ws(lib.mi_conv3d_s2_fwd_workspace_bytes(ci, co), x.device, "conv_s2f")
    def call():
        return L.call("mi_conv3d_s2_fwd_f32", x, w, w_ds, hmid, r, n, g, ci, co, ws, ws.numel())
    # algorithmic FLOPs of both convolutions the launch replaces (27 taps + the 1x1 shortcut)
    _prof_run("fwd", 2.0 * hmid.numel() * ci * 28, call)
    return hmid, r


def conv_dgrad_s2_block(dh, d2, w, w_ds, in_shape, res=None, mask=None):
    """Data gradient of a BasicBlock's stride-2 front in ONE launch (csrc/conv_s2.hip): conv_dgrad(dh; w, 3x3x3 stride 2 pad 1)
    + conv_dgrad(d2; w_ds, 1x1 stride 2) (+ res), times (mask > 0).  Returns None when the shape is not one of the encoder's two
    (the caller then runs the two generic launches)."""
    if not dh.is_cuda:
        return None
    n, g, _, _, ci = in_shape
    co = int(w.shape[0])
    held_family, img = _held_image(w, True) if d2 is not None else (None, None)
    route = conv_route("dgrad", tuple(in_shape), ci, co, (3, 3, 3), 2, (1, 1, 1), has_res=res is not None, image=held_family,
                       profile=PROFILE is not None, shortcut=True, phys_ok=_phys_ok(w) and (w_ds is None or _phys_ok(w_ds)))
    if route.family is None:
        return None
    _f32c(dh, "dh")
    if d2 is not None:
        _f32c(d2, "d2")
    lib = L.lib()
    dx = torch.empty(tuple(in_shape), dtype=torch.float32, device=dh.device)
    if route.param:                                       # the engine keeps the images current: no image build here
        L.call("mi_conv3d_s2_dgrad_img_f32", dh, d2, img, dx, res, mask, n, g, ci, co)
        return dx
    ws = _ws(lib.mi_conv3d_s2_dgrad_workspace_bytes(ci, co), dh.device, "conv_s2")
    def call():
        return L.call("mi_conv3d_s2_dgrad_f32", dh, d2, w, w_ds, dx, res, mask, n, g, ci, co, ws, ws.numel())
    # algorithmic FLOPs of both convolutions the launch replaces (27 taps + the 1x1 shortcut)
    _prof_run("dgrad", 2.0 * dh.numel() * ci * (27 + (1 if d2 is not None else 0)), call)
    return dx


# Deferred split-K reduction of the weight gradients: while DEFERRED_WGRADS is a list (MocoStepEngine sets it around the
# backward pass), every wgrad launch leaves its slabs in a slab buffer of its own and registers (slabs, target, splits,
# elements) here; flush_wgrad_reduces() sums them all in one launch (one per gradient bucket under data parallelism)
# instead of one small reduce launch behind each of the 18 weight-gradient kernels of a step.
DEFERRED_WGRADS = None


def flush_wgrad_reduces():
    global DEFERRED_WGRADS
    items = DEFERRED_WGRADS
    if not items:
        return
    L.call("mi_splitk_reduce_batch", L.host_array([it[0].data_ptr() for it in items]), L.host_array([it[1].data_ptr() for it in items]),
           L.host_array([it[2] for it in items], ctypes.c_int), L.host_array([it[3] for it in items], ctypes.c_long), len(items))
    del items[:]


# Weight gradients of the small layers on a side stream: while SIDE_WGRADS is a list (MocoStepEngine sets it around the
# backward pass), the weight-gradient launches of layers with at most SIDE_ROWS_MAX output rows (everything but the stem at
# the encoder's shapes) are not issued where autograd reaches them but collected here; the engine issues a whole stage's worth
# on ONE fork of a side stream when the data-gradient chain leaves the stage: layer3's and the head's next to layer2's
# data gradients, layer2's next to layer1's, layer1's next to the HBM-bound stem chain.  One cross-stream edge per stage - an
# edge per launch costs more than it returns (r03_experiments.txt items 6 and 9).
SIDE_WGRADS = None
SIDE_ROWS_MAX = int(os.environ.get("CETPICK_SIDE_ROWS", "32768"))


def _side_or_now(fn, rows):
    """True: queued for the side stream (MocoStepEngine issues it at the stage boundary); False: launched now."""
    # (bench.py's roofline pass - PROFILE - times every call by itself: closures run where they are; convolution jobs are still
    # collected, so that the pass times the launches the step really makes - run_wgrad_jobs times a group as one call)
    if SIDE_WGRADS is not None and rows <= SIDE_ROWS_MAX and (PROFILE is None or isinstance(fn, _WgradJob)):
        SIDE_WGRADS.append(fn)
        return True
    fn()
    return False


class _WgradJob:
    """One deferred convolution weight gradient (slab form): callable like the closures next to it in SIDE_WGRADS; jobs of one
    geometry (`geom`: a _Geom) that are issued together go out as ONE launch (run_wgrad_jobs -> mi_conv_wgrad_batch_f32)."""
    __slots__ = ("x", "dy", "tgt", "slab", "geom", "param", "flops")

    def __init__(self, x, dy, tgt, slab, geom, param=None, flops=0.0):
        self.x, self.dy, self.tgt, self.slab, self.geom, self.param, self.flops = x, dy, tgt, slab, geom, param, flops

    def __call__(self):
        splits = ctypes.c_int(0)
        L.call("mi_conv_wgrad_f32", self.x, self.dy, self.tgt, self.geom.ref, self.slab, self.slab.numel(), ctypes.addressof(splits))
        if splits.value > 1:
            DEFERRED_WGRADS.append((self.slab, self.tgt, int(splits.value), self.tgt.numel()))


WGRAD_BATCH = os.environ.get("CETPICK_WGRAD_BATCH", "1") != "0"
WGRAD_BATCH_MAX = 4

# Outside a MocoStepEngine step (plain autograd: loss.backward() of any trainer) the same grouping happens at the END of the backward
# pass: the jobs wait in _BACKWARD_END and one autograd final callback issues them (run_wgrad_jobs + the slab reduce) on the caller's
# stream.  Engine and plain sequence thus launch the same kernels on the same chains - their gradients stay equal bit for bit
# (tests/test_trainer_gpu.py::test_engine_step_equals_plain_sequence_bitwise) although a batched layer1 gradient is cut into other
# chains than a single one.
_BACKWARD_END = None
_BACKWARD_END_TASK = -1          # autograd graph-task id of the pass the queued jobs belong to


def _defer_to_backward_end(job):
    global _BACKWARD_END, _BACKWARD_END_TASK
    try:
        # (one callback per job: the first one to run flushes everything, the others find the list empty)
        torch.autograd.Variable._execution_engine.queue_callback(_flush_backward_end)
    except RuntimeError:                                   # not inside a backward pass (a direct call): launch now
        return False
    task = torch._C._current_graph_task_id()
    if _BACKWARD_END is not None and task != _BACKWARD_END_TASK:
        #  jobs of a backward pass that RAISED (its final callbacks never ran): their operands belong to a dead pass -
        # dropped, never launched into the gradients of this one
        for stale in _BACKWARD_END:
            if stale.param is not None:
                stale.param._mi_wgrad_pending = False
        _BACKWARD_END = None
    if _BACKWARD_END is None:
        _BACKWARD_END = []
        _BACKWARD_END_TASK = task
    _BACKWARD_END.append(job)
    if job.param is not None:
        job.param._mi_wgrad_pending = True                 # (a second contribution to this parameter flushes first: conv_wgrad_into)
    return True


def _flush_backward_end():
    global _BACKWARD_END, DEFERRED_WGRADS
    items, _BACKWARD_END = _BACKWARD_END, None
    if not items:
        return
    saved, DEFERRED_WGRADS = DEFERRED_WGRADS, []
    try:
        run_wgrad_jobs(items)
        flush_wgrad_reduces()
    finally:
        DEFERRED_WGRADS = saved


def _launch_wgrad_group(jobs):
    """Up to WGRAD_BATCH_MAX jobs of one geometry and slab size: ONE batched launch or - a single job, or a geometry the library has no
    batched kernel for - one launch each; split launches leave their slabs registered in DEFERRED_WGRADS."""
    batched = False
    if len(jobs) > 1:
        splits = ctypes.c_int(0)
        batched = L.call("mi_conv_wgrad_batch_f32", L.host_array([j.x.data_ptr() for j in jobs]),
                         L.host_array([j.dy.data_ptr() for j in jobs]), L.host_array([j.tgt.data_ptr() for j in jobs]),
                         L.host_array([j.slab.data_ptr() for j in jobs]), len(jobs), jobs[0].geom.ref, jobs[0].slab.numel(),
                         ctypes.addressof(splits), may_decline=True)
        if batched and splits.value > 1:
            for j in jobs:
                DEFERRED_WGRADS.append((j.slab, j.tgt, int(splits.value), j.tgt.numel()))
    if not batched:                                        # MI_E_UNSUPPORTED (or a single job): one launch each
        for j in jobs:
            j()


def run_wgrad_jobs(items):
    """Issue the collected weight-gradient launches of a stage on the current stream: convolution jobs of one geometry in
    groups of up to four per launch, everything else (and what the library declines) one by one, in collection order."""
    groups, order = {}, []
    for it in items:
        if isinstance(it, _WgradJob) and it.param is not None:
            it.param._mi_wgrad_pending = False
        if isinstance(it, _WgradJob) and WGRAD_BATCH and DEFERRED_WGRADS is not None:
            key = it.geom.key + (it.slab.numel(),)
            if key not in groups:
                groups[key] = []
                order.append(groups[key])
            groups[key].append(it)
        else:
            order.append(it)
    if PROFILE is not None:
        _run_wgrad_jobs_profiled(order)
        return
    for it in order:
        if not isinstance(it, list):
            it()
            continue
        for i0 in range(0, len(it), WGRAD_BATCH_MAX):
            _launch_wgrad_group(it[i0:i0 + WGRAD_BATCH_MAX])


def _run_wgrad_jobs_profiled(order):
    """bench.py's roofline pass: a group's launch + the reduce of its slabs is ONE timed call (what the step launches), with the
    group's algorithmic FLOPs; the slabs are reduced here instead of in the stage's deferred reduce."""
    for it in order:
        if not isinstance(it, list):
            if isinstance(it, _WgradJob):
                it = [it]
            else:
                it()
                continue
        for i0 in range(0, len(it), WGRAD_BATCH_MAX):
            jobs = it[i0:i0 + WGRAD_BATCH_MAX]

            def call(jobs=jobs):
                global DEFERRED_WGRADS
                saved, DEFERRED_WGRADS = DEFERRED_WGRADS, []
                try:
                    _launch_wgrad_group(jobs)
                    flush_wgrad_reduces()
                finally:
                    DEFERRED_WGRADS = saved
            _prof_run("wgrad", sum(j.flops for j in jobs), call)


def conv_wgrad_into(x, dy, param, k, stride, pad, dil=None):
    """dW for `param`, written (or accumulated) into param.grad."""
    nd5 = x.dim() == 5
    k3, p3 = _k3(k, nd5), _p3(pad, nd5)
    d3 = _k3(dil, nd5) if dil is not None else None
    n, d, h, wd, ci = _as5d(x).shape
    co = int(dy.shape[-1])
    lib = L.lib()
    if getattr(param, "_mi_wgrad_pending", False):
        # a module applied twice in one backward pass (the symmetric MoCo loss): the first contribution still waits for the end of
        # the pass with this parameter's gradient as its target and its slab buffer - it goes out now, this one accumulates onto it
        if DEFERRED_WGRADS is not None:
            raise L.HipExtensionError("MocoStepEngine: a convolution applied twice in one backward pass (its first weight gradient is "
                                      "still queued for the side stream) - run this model without the step engine")
        _flush_backward_end()
    dest = _GradInto(param)
    tgt = dest.tgt
    flops = 2.0 * dy.numel() * ci * k3[0] * k3[1] * k3[2]
    route = conv_route("wgrad", tuple(x.shape), ci, co, k3, stride, p3, d3, profile=PROFILE is not None, phys_ok=_phys_ok(param),
                       accumulates=dest.accumulates, deferred=DEFERRED_WGRADS is not None, side=SIDE_WGRADS is not None)
    geom = _Geom((n, d, h, wd, ci), co, k3, stride, p3, d3) if route.family == "generic" else None
    if route.family != "generic" or route.param:
        _f32c(x, "x"), _f32c(dy, "dy")
    if route.param:                                        # the slab form
        nbytes = lib.mi_conv_workspace_bytes(geom.ref)
        slab = getattr(param, "_mi_slabs", None)
        if slab is None or slab.numel() < nbytes or slab.device != x.device:
            slab = torch.empty(int(nbytes), dtype=torch.uint8, device=x.device)     # lives with the parameter
            if not getattr(param, "_mi_slabs_pinned", False):
                param._mi_slabs = slab
            # (pinned: a captured hipGraph writes and reads the old buffer on every replay - the step engines pin the slabs
            # when they capture; an eager call that needs more space gets a buffer of its own and the graph's stays alive)
        job = _WgradJob(x, dy, tgt, slab, geom, param, flops)    # (writes the gradient itself: no temporary to add behind it)
        if DEFERRED_WGRADS is not None:
            if _side_or_now(job, dy.numel() // co):
                param._mi_wgrad_pending = True             # queued: cleared by run_wgrad_jobs (a second contribution before that raises)
            return
        if _defer_to_backward_end(job):                    # plain autograd: layer1's / layer2's weight gradients, batched at the end
            return
    if route.family == "stem3":
        ws = _ws(lib.mi_conv2d_stem3_workspace_bytes(co), x.device, "stem3")
        def call():
            return L.call("mi_conv2d_stem3_wgrad_f32", x, dy, tgt, n, h, wd, co, ws, ws.numel())
    elif route.family == "p2d":
        ws = _ws(int(lib.mi_conv2d_p2d_wgrad_workspace_bytes(n, h, wd, ci)), x.device, "p2d_wgrad")
        def call():
            return L.call("mi_conv2d_p2d_wgrad_f32", x, dy, tgt, n, h, wd, ci, ws, ws.numel())
    else:
        ws = geom.workspace(x.device)
        def call():
            return L.call("mi_conv_wgrad_f32", x, dy, tgt, geom.ref, ws, ws.numel(), None)
    with dest:
        _prof_run("wgrad", flops, call)


def relu_mask(dy, y, add=None):
    out = torch.empty_like(dy)
    L.call("mi_relu_mask", dy, y, add, out, dy.numel())
    return out


def _stem_fwd_with_stats(x, w, mod):
    """The stem convolution with the batch statistics of the BatchNorm behind it from its epilogue (mi_conv3d_stem_stats_f32:
    no statistics pass over the 67 MB output).  Leaves them in mod.bn_sums for bn_relu_maxpool3d(..., sums=...); None where
    the stem kernel does not apply (the caller then takes the plain convolution and the BatchNorm its own statistics)."""
    mod.bn_sums = None
    if PROFILE is not None or x.dim() != 5 or x.shape[-1] != 1 or (mod.k, mod.stride, mod.pad) != (7, 2, 3) or not _phys_ok(w):
        return None
    lib = L.lib()
    n, d, h, wd, _ = x.shape
    co = w.shape[0]
    nbytes = lib.mi_conv3d_stem_stats_workspace_bytes(n, d, h, wd, co)
    if nbytes == 0:
        return None
    do, ho, wo = [(v + 6 - 7) // 2 + 1 for v in (d, h, wd)]
    y = torch.empty((n, do, ho, wo, co), dtype=torch.float32, device=x.device)
    sums = torch.empty(2 * co, dtype=torch.float64, device=x.device)
    ws = _ws(nbytes, x.device, "stem_stats")
    if not L.call("mi_conv3d_stem_stats_f32", x, w, y, n, d, h, wd, co, sums, ws, ws.numel(), may_decline=True):
        return None
    mod.bn_sums = sums
    return y


class GradSlot:
    """A gradient contribution handed from one autograd node to another of the same block instead of through autograd's sum: the
    node behind a residual connection (BatchNorm + residual + ReLU) leaves the residual branch's gradient here, the block's first
    convolution - whose input IS that residual - adds it in its data gradient's epilogue (`res`).  One element-wise launch less
    per identity block and pass; the sum is the same single rounding."""
    __slots__ = ("tensor",)

    def __init__(self):
        self.tensor = None


FUSE_RES_GRAD = os.environ.get("CETPICK_FUSE_RES_GRAD", "1") != "0"


def grad_slot_for(x):
    """A GradSlot when the gradient of `x` will be computed (and the fusion is on), else None."""
    return GradSlot() if (FUSE_RES_GRAD and torch.is_grad_enabled() and x.requires_grad and x.is_cuda and PROFILE is None) else None


class _ConvFn(torch.autograd.Function):
    """y = act(conv(x, W)); W's gradient goes to mod.weight.grad directly."""

    @staticmethod
    def forward(ctx, x, w, mod, relu, mask_dx=False, inference=False, grad_slot=None, dx_slot=None):
        ctx.mod, ctx.relu, ctx.mask_dx = mod, relu, mask_dx
        ctx.grad_slot = grad_slot                        # a gradient of x that arrives here instead of through autograd's sum: added in the epilogue
        ctx.dx_slot = dx_slot                            # ... and this node's own gradient of x LEAVES through a slot (a shortcut convolution:
                                                         # the block's first convolution, which runs later in the backward pass, adds it)
        y = _stem_fwd_with_stats(x, w, mod) if (getattr(mod, "stats_for_bn", False) and not relu) else None
        if y is None:
            y = conv_fwd(x, w, mod.k, mod.stride, mod.pad, None, relu, dil=getattr(mod, "dil", None), owner=mod.weight,
                         inference=inference)
        ctx.save_for_backward(x, y if relu else None)
        ctx.x_needs_grad = x.requires_grad
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        mod = ctx.mod
        dy = dy.contiguous()
        if ctx.relu:
            dy = relu_mask(dy, y)
        dil = getattr(mod, "dil", None)
        if mod.weight.requires_grad:
            conv_wgrad_into(x, dy, mod.weight, mod.k, mod.stride, mod.pad, dil=dil)
        dx = None
        extra = None
        if ctx.grad_slot is not None:
            extra, ctx.grad_slot.tensor = ctx.grad_slot.tensor, None
        if ctx.x_needs_grad:
            # mask_dx: x is the output of a ReLU whose derivative the producer left to this layer (see basic_block)
            # extra: the gradient x receives through the block's residual connection (GradSlot), added in the epilogue
            if extra is not None and ctx.mask_dx:
                raise L.HipExtensionError("a residual gradient slot and a masked data gradient do not combine")
            dx = conv_dgrad(dy, mod.weight, x.shape, mod.k, mod.stride, mod.pad, extra, x if ctx.mask_dx else None, dil=dil)
            if ctx.dx_slot is not None:
                if ctx.dx_slot.tensor is not None:
                    raise L.HipExtensionError("gradient slot already holds a tensor")
                ctx.dx_slot.tensor, dx = dx, None
        return dx, None, None, None, None, None, None, None


def conv_bias_fwd(x, w, bias, k, stride, pad, relu=False, out=None, pool=False):
    """y = act(conv(x, w) + bias[co]) in one launch (mi_conv_fwd_f32 with the residual read as a bias row), inference only: no
    autograd node.  `out`: a contiguous (N, [D,] Ho, Wo, Co) tensor (or a leading-axis slice of one) that receives the result.
    pool: (y, maxpool2x2(y)) in one launch, with `out` possibly a channel slice of a wider tensor - or None: the caller pools by itself."""
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
        raise L.HipExtensionError("conv_bias_fwd is inference only (no autograd node)")
    return _conv_forward(x, w, k, stride, pad, None, bias, relu, None, None, True, out, pool, who="conv_bias_fwd: ")


CONCAT_DIRECT = os.environ.get("CETPICK_CONCAT_DIRECT", "1") != "0"


def skip_into_concat_ok(conv, bn, x, co_up, up=None, up_bn=None):
    """True when a down-convolution block's last layer (conv -> bn -> ReLU -> pool on x) can write its un-pooled output - the skip
    connection - straight into the concatenation buffer of the up-convolution block that consumes it, AND that block's transposed
    convolution will write the other channels there with its fused epilogue (upconv_bn_relu_concat): inference, both on conv_d32.hip."""
    if not (CONCAT_DIRECT and POOL_FUSED and UPCONV_FUSED and FOLD_EVAL_BN and PROFILE is None and x.is_cuda and x.dim() == 4
            and not torch.is_grad_enabled() and not bn.training and bn.track_running_stats and _arith_bf16x3()):
        return False
    n, h, w, ci = x.shape
    co = conv.co
    if co != co_up or co not in (32, 64) or h % 16 or w % 32:          # the up block: 2 co -> co on (h / 2, w / 2), rows % 8, columns % 16
        return False
    # the concatenation buffer is co_up + co channels wide: both kernels that write into it address it with 32-bit byte offsets and
    # answer MI_E_UNSUPPORTED from 0x7fff0000 bytes on (a 32-slice chunk of a 1024 x 1024 tomogram: 2^31) - the dense form takes over
    if 4 * n * h * w * (co_up + co) >= 0x7fff0000:
        return False
    # ... and the up block's side of the bargain: evaluation-mode BatchNorm that can be folded, weights in kernel layout
    if up_bn is not None and (up_bn.training or not up_bn.track_running_stats):
        return False
    if up is not None and not _phys_ok(up.gemm_view()):
        return False
    # ... and this layer on the patch-resident kernel that makes the pooled second output (conv_d32.hip kinds 1 / 3)
    route = conv_route("fwd", (n, h, w, ci), ci, co, _k3(conv.k, False), conv.stride, _p3(conv.pad, False), inference=True, has_bias=True,
                       relu=True, pool=True)
    return route.family == "d32"


def conv_bn(conv, bn, x, relu=False, pool=False, out=None):
    """bn(conv(x), relu) for a HipConv2d / HipConvNd followed by a HipBatchNorm.  At inference (evaluation-mode BatchNorm with
    running statistics, no gradient) the BatchNorm folds into the convolution: w' = w * gamma / sqrt(var + eps) per output
    channel, bias = beta - mean * gamma / sqrt(var + eps), one launch with a bias + ReLU epilogue and no BatchNorm pass over
    the activation (reference: conv -> BatchNorm2d -> ReLU, models/networks/unet.py:198-249,319-399).  The folded weights are
    kept on the BatchNorm module and rebuilt when any of the five tensors they come from changes.  pool: returns (y, maxpool 2 x 2
    ceil-mode of y) - unet.py:198-249's down-convolution block."""
    folded = (not bn.training and bn.track_running_stats and not torch.is_grad_enabled() and x.is_cuda and
              getattr(conv, "dil", None) in (None, (1, 1, 1)) and FOLD_EVAL_BN)
    if not folded:
        if out is not None:
            raise L.HipExtensionError("conv_bn: `out` needs the folded inference path (skip_into_concat_ok)")
        y = bn(conv(x), relu=relu)
        return (y, maxpool2d_ceil(y, 2)) if pool else y
    src = (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    key = tuple((t.data_ptr(), t._version) if t is not None else None for t in src) + (float(bn.eps), WEIGHT_EPOCH)
    cache = getattr(bn, "_folded", None)
    if cache is None or cache[0] != key:
        with torch.no_grad():
            inv = torch.rsqrt(bn.running_var.double() + bn.eps)
            sc = inv if bn.weight is None else bn.weight.double() * inv
            sh = -bn.running_mean.double() * sc
            if bn.bias is not None:
                sh = sh + bn.bias.double()
            wf = (conv.weight.double() * sc.view(-1, *([1] * (conv.weight.dim() - 1)))).float()
            cache = (key, wf, sh.float().contiguous())
        if not _phys_ok(wf):
            raise L.HipExtensionError("folded convolution weight left the kernel layout")
        bn._folded = cache
    if pool:
        # pool = True: (y, MaxPool2d(2, ceil_mode)(y)) - in one launch where the patch-resident kernel takes the layer (the pool is
        # its epilogue's by-product), else the pooling pass behind it
        both = conv_bias_fwd(x, cache[1], cache[2], conv.k, conv.stride, conv.pad, relu, pool=True, out=out)
        if both is not None:
            return both
        if out is not None:
            raise L.HipExtensionError("conv_bn: `out` (a channel slice) needs the patch-resident kernel (skip_into_concat_ok)")
        y = conv_bias_fwd(x, cache[1], cache[2], conv.k, conv.stride, conv.pad, relu)
        return y, maxpool2d_ceil(y, 2)
    if out is not None:
        raise L.HipExtensionError("conv_bn: `out` is the pooled form's (pool=True)")
    return conv_bias_fwd(x, cache[1], cache[2], conv.k, conv.stride, conv.pad, relu)


def _d32_up_image(up, ci, co):
    """conv_d32.hip's image of the up-convolution's 1 x 1 product (4 co columns), kept on up.weight."""
    wv = up.gemm_view()
    lib = L.lib()
    def cut(_):
        img = torch.empty((4 * co // 64) * int(lib.mi_conv_d64_image_bytes(ci, 1)), dtype=torch.uint8, device=wv.device)
        L.call("mi_conv_d64_prep_co", wv, img, ci, 4 * co, 1)
        return img
    return _kept_image(up.weight, "_mi_d32_up", wv, (ci, co, "up"), cut)


def upconv_bn_relu_concat(up, bn, dec, enc, cat=None):
    """cat(relu(bn(up(dec))), enc) over the channel axis (unet.py:319-399).  At inference one 1 x 1 product + ONE pass that shuffles,
    applies the folded BatchNorm (the transposed convolution's bias included), the ReLU and writes the concatenation
    (mi_upconv_tail_fwd) - instead of shuffle, BatchNorm and concat passes over the feature map."""
    ho, wo = enc.shape[1], enc.shape[2]
    folded = (not bn.training and bn.track_running_stats and not torch.is_grad_enabled() and dec.is_cuda and FOLD_EVAL_BN)
    if not folded:
        if cat is not None:
            raise L.HipExtensionError("upconv_bn_relu_concat: `cat` needs the folded inference path")
        return concat_channels(bn(up(dec, ho, wo), relu=True), enc)
    src = (up.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    key = tuple((t.data_ptr(), t._version) if t is not None else None for t in src) + (float(bn.eps), WEIGHT_EPOCH)
    cache = getattr(bn, "_folded_up", None)
    if cache is None or cache[0] != key:
        with torch.no_grad():
            inv = torch.rsqrt(bn.running_var.double() + bn.eps)
            sc = inv if bn.weight is None else bn.weight.double() * inv
            sh = -bn.running_mean.double() * sc
            if up.bias is not None:
                sh = sh + up.bias.double() * sc
            if bn.bias is not None:
                sh = sh + bn.bias.double()
            cache = (key, sc.float().contiguous(), sh.float().contiguous())
        bn._folded_up = cache
    _f32c(dec, "dec")
    if cat is None:
        _f32c(enc, "enc")                                # (with `cat`, enc is a channel slice of it: checked below)
    n, h, w, _ = dec.shape
    co, ce = up.co, enc.shape[-1]
    ci = dec.shape[-1]
    if cat is not None:
        # `enc` IS cat[..., co:] (the down-convolution block wrote it there: skip_into_concat_ok): only the first co channels are missing
        if (tuple(cat.shape) != (n, ho, wo, co + ce) or not cat.is_contiguous() or enc.data_ptr() != cat.data_ptr() + 4 * co):
            raise L.HipExtensionError("upconv_bn_relu_concat: `cat` is not the buffer `enc` is a channel slice of")
        wimg = _d32_up_image(up, ci, co)
        L.call("mi_conv_d32_upconv_fwd_f32", dec, wimg, cache[1], cache[2], cat, n, h, w, ci, co, ho, wo, co + ce)
        return cat
    out = torch.empty((n, ho, wo, co + ce), dtype=torch.float32, device=dec.device)
    if (UPCONV_FUSED and _arith_bf16x3() and PROFILE is None and ci in (32, 64, 128) and co % 32 == 0 and 64 <= 4 * co <= 512
            and h % 8 == 0 and w % 16 == 0 and _phys_ok(up.gemm_view())):
        # the product, the pixel shuffle, the folded BatchNorm and the ReLU in ONE launch (conv_d32.hip, 1 x 1 form with the
        # up-convolution epilogue) straight into the concatenation; the encoder feature goes into the other channels
        wimg = _d32_up_image(up, ci, co)
        if L.call("mi_conv_d32_upconv_fwd_f32", dec, wimg, cache[1], cache[2], out, n, h, w, ci, co, ho, wo, co + ce, may_decline=True):
            L.call("mi_copy_channels_into", enc, ce, out, co + ce, co, n * ho * wo)
            return out
    t = conv_fwd(dec, up.gemm_view(), 1, 1, 0, owner=up.weight, inference=True)      # (`folded` above: no gradient)
    L.call("mi_upconv_tail_fwd", t, cache[1], cache[2], enc, out, n, h, w, co, ce, ho, wo)
    return out


FOLD_EVAL_BN = os.environ.get("CETPICK_FOLD_BN", "1") != "0"
UPCONV_FUSED = os.environ.get("CETPICK_UPCONV_FUSED", "1") != "0"       # the transposed convolution's product with the tail in its epilogue


def convnd_weight_param(co, ci, k3, device=None):
    """Parameter with logical shape (co, ci, kd, kh, kw) over physical storage [kd,kh,kw,ci,co]."""
    phys = torch.empty(*k3, ci, co, device=device)
    return nn.Parameter(phys.permute(4, 3, 0, 1, 2))


class HipConvNd(nn.Module):
    """nn.Conv3d(ci, co, kernel (kd,kh,kw), stride 1, padding (pd,ph,pw), dilation, bias=False), channels-last."""

    def __init__(self, ci, co, k3, pad3, dil3=(1, 1, 1)):
        super().__init__()
        self.ci, self.co, self.k, self.stride, self.pad, self.dil = ci, co, tuple(k3), 1, tuple(pad3), tuple(dil3)
        self.weight = convnd_weight_param(co, ci, k3)
        with torch.no_grad():
            bound = 1.0 / (ci * k3[0] * k3[1] * k3[2]) ** 0.5
            self.weight.uniform_(-bound, bound)

    def forward(self, x, relu=False):
        return _ConvFn.apply(x, self.weight, self, relu, False, inference_mode())


class HipConv3d(nn.Module):
    """nn.Conv3d(ci, co, k, stride, padding, bias=False) on channels-last activations."""

    def __init__(self, ci, co, k, stride=1, pad=0):
        super().__init__()
        self.ci, self.co, self.k, self.stride, self.pad = ci, co, k, stride, pad
        self.weight = conv_weight_param(co, ci, k)
        with torch.no_grad():
            # nn.Conv3d default init: kaiming_uniform(a=sqrt(5)) == U(-1/sqrt(fan_in), 1/sqrt(fan_in))
            bound = 1.0 / (ci * k ** 3) ** 0.5
            self.weight.uniform_(-bound, bound)

    def forward(self, x, relu=False, mask_dx=False):
        return _ConvFn.apply(x, self.weight, self, relu, mask_dx, inference_mode())


class HipConv2d(nn.Module):
    """nn.Conv2d(ci, co, k, stride, padding, bias=False) on channels-last (N,H,W,C) activations."""

    def __init__(self, ci, co, k, stride=1, pad=0):
        super().__init__()
        self.ci, self.co, self.k, self.stride, self.pad = ci, co, k, stride, pad
        self.weight = conv2d_weight_param(co, ci, k)
        with torch.no_grad():
            bound = 1.0 / (ci * k * k) ** 0.5
            self.weight.uniform_(-bound, bound)

    def forward(self, x, relu=False, grad_slot=None, dx_slot=None):
        return _ConvFn.apply(x, self.weight, self, relu, False, inference_mode(), grad_slot, dx_slot)


class _BNFuse:
    """One call's request to the Linear node (linear_bn, linear_with_local_sums -> HipLinear.forward(fuse=...)): let the product's
    launch also do the work of the BatchNorm `bn` behind it - apply it (+ ReLU), or `stats_only`: leave this rank's column sums
    (SyncBN: the all-reduce and the apply stay launches of their own).  _LinearFn.forward fills in what its launch produced:
    `sums`, `applied` = (y_bn, save), or neither where the library declined.  Made per call and dropped with it."""
    __slots__ = ("bn", "relu", "stats_only", "sums", "applied")

    def __init__(self, bn, relu, stats_only):
        self.bn, self.relu, self.stats_only = bn, relu, stats_only
        self.sums = self.applied = None


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, mod, inference=False, fuse=None):
        m, ci = x.shape
        w5 = w.view(w.shape[0], ci, 1, 1, 1) if w.dim() == 5 else _as5(w)
        y = None
        if (fuse is not None or b is not None) and PROFILE is None and _phys_ok(w5):
            # one launch with an epilogue: the fused entry `fuse` asks for, then - no request, or the entry declined (-3,
            # MI_E_UNSUPPORTED: rows, arithmetic switch) - the product with the bias in it, then the generic path below
            _f32c(x, "x")
            co = w5.shape[0]
            y = torch.empty((m, co), dtype=torch.float32, device=x.device)
            fused = False
            if fuse is not None and fuse.stats_only:
                # this rank's column sums come out of the product's epilogue; the BatchNorm node all-reduces them and applies
                sums = torch.empty(2 * co, dtype=torch.float64, device=x.device)
                fused = L.call("mi_linear_stats_fwd_f32", x, w5, b, y, sums, m, ci, co, may_decline=True)
                if fused:
                    fuse.sums = sums
            elif fuse is not None:
                # Linear + BatchNorm1d (+ ReLU) in one launch: the BatchNorm's output and saved statistics go back to linear_bn
                # for the BatchNorm node; this node's own output is the Linear's, as always
                bn = fuse.bn
                yb = torch.empty((m, co), dtype=torch.float32, device=x.device)
                save = torch.empty(2 * co, dtype=torch.float32, device=x.device)
                fused = L.call("mi_linear_bn_fwd_f32", x, w5, b, y, yb, m, ci, co, bn.weight, bn.bias, bn.eps, bn.momentum,
                               *_bn_running_ptrs(bn, bn.track_running_stats and bn.training), save, int(fuse.relu), may_decline=True)
                if fused:
                    fuse.applied = (yb, save)
            if not fused and b is not None:
                # the bias rides in the epilogue of the GEMM launch (or of its split-K reduce)
                ws = _linear_geom(m, ci, co).workspace(x.device)
                L.call("mi_linear_fwd_f32", x, w5, b, y, m, ci, co, ws, ws.numel())
            elif not fused:
                y = None
        if y is None:
            y = conv_fwd(x.view(m, 1, 1, 1, ci), w5, 1, 1, 0, owner=w, inference=inference).view(m, -1)
            if b is not None:
                L.call("mi_bias_add", y, b, m, y.shape[1])
        ctx.mod = mod
        ctx.save_for_backward(x)
        ctx.x_needs_grad = x.requires_grad
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        mod = ctx.mod
        dy = dy.contiguous()
        m, ci = x.shape
        co = dy.shape[1]
        if mod.weight.requires_grad:
            dest = _GradInto(mod.weight)               # (the target is bound now, the launch may wait for the side stream)
            def launch():
                geom = _linear_geom(m, ci, co)
                ws = geom.workspace(x.device)
                with dest as tgt:
                    L.call("mi_conv_wgrad_f32", x, dy, tgt, geom.ref, ws, ws.numel(), None)
            _side_or_now(launch, m)
        if mod.bias is not None and mod.bias.requires_grad:
            _side_or_now(_colsum_job(dy, mod.bias), m)  # the bias gradient is a parameter gradient too: same side-stream batch
        dx = None
        if ctx.x_needs_grad:
            dx = conv_dgrad(dy.view(m, 1, 1, 1, co), _as5(mod.weight), (m, 1, 1, 1, ci), 1, 1, 0).view(m, ci)
        return dx, None, None, None, None, None


def _as5(w2):
    """(out, in) weight with strides (1, out) viewed as (out, in, 1, 1, 1) in kernel layout."""
    out_f, in_f = w2.shape
    return torch.as_strided(w2, (out_f, in_f, 1, 1, 1), (1, out_f, in_f * out_f, in_f * out_f, in_f * out_f))


class HipLinear(nn.Module):
    def __init__(self, in_f, out_f, bias=True):
        super().__init__()
        self.in_f, self.out_f = in_f, out_f
        self.weight = linear_weight_param(out_f, in_f)
        self.bias = nn.Parameter(torch.empty(out_f)) if bias else None
        with torch.no_grad():
            bound = 1.0 / in_f ** 0.5
            self.weight.uniform_(-bound, bound)
            if bias:
                self.bias.uniform_(-bound, bound)

    def forward(self, x, fuse=None):
        """fuse: a _BNFuse request (linear_bn, linear_with_local_sums); the result is the Linear's output either way."""
        if not _phys_ok(self.weight):
            raise L.HipExtensionError("linear weight is not in kernel layout [in][out]")
        return _LinearFn.apply(_f32c(x, "x"), self.weight, self.bias, self, inference_mode(), fuse)


# ------------------------------------------------------------------------------------------------
# batch norm (+ReLU), SyncBN-capable
# ------------------------------------------------------------------------------------------------
def _dist_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size()
    return 1


FORCE_COLLECTIVES = False     # tests: issue every collective on a 1-rank group too (one-GPU rehearsal of the N>1 path)


# Collectives under hipGraph capture are issued SYNCHRONOUSLY (async_op=False), always.  A collective issued with
# async_op=True while its stream is being captured ends up polled by the process group's watchdog thread, whose
# hipEventQuery on the Work's end event - last recorded in a capturing stream - raises hipErrorCapturedEvent and
# terminates the process ("operation not permitted on an event last recorded in a capturing stream"; measured with
# tools/diag_captured_event.py / tools/diag_teardown.py, profiles/r02_teardown_diag.txt: 4 of 4 captured runs die with async
# works, 0 of 4 without).  That was the intermittent abort of
# the N > 1 captured step that round 1 hid behind os._exit: the engine's four bucket all-reduces were async.  Overlap
# with the backward pass comes from issuing the (synchronous) collective on a side stream instead - see
# MocoStepEngine._reduce_bucket.
def dist_all_reduce(tensor):
    import torch.distributed as dist
    dist.all_reduce(tensor)


def dist_all_reduce_pair(a, b):
    """all_reduce(a); all_reduce(b) as ONE collective where the backend can group them (RCCL: ncclGroupStart / End - one launch, one
    latency): the SyncBN statistics of encoder_q's and encoder_k's layer i, whose forward passes MoCo runs layer-locked (round 6).
    Synchronous, like every collective here (see above)."""
    import torch.distributed as dist
    if dist.get_backend() == "nccl" and a.is_cuda:
        with dist.distributed_c10d._coalescing_manager():
            dist.all_reduce(a)
            dist.all_reduce(b)
    else:
        dist.all_reduce(a)
        dist.all_reduce(b)


def _bn_stats(x, m, c):
    """Column sums (sum x, sum x^2: 2C doubles) of the (m, c) activation x: the statistics pass."""
    lib = L.lib()
    ws = _ws(lib.mi_colreduce_workspace_bytes(m, c), x.device, "colreduce")
    sums = torch.empty(2 * c, dtype=torch.float64, device=x.device)
    L.call("mi_bn_stats", x, m, c, sums, ws, ws.numel())
    return sums


def bn_local_sums(x):
    """This rank's column sums (sum x, sum x^2: 2C doubles) of a channels-last activation - the statistics pass of a SyncBN whose
    all-reduce the caller issues itself (paired with another branch's: MoCo's layer-locked forward)."""
    _f32c(x, "x")
    c = x.shape[-1]
    return _bn_stats(x, x.numel() // c, c)


def dist_all_gather(tensor_list, tensor):
    import torch.distributed as dist
    dist.all_gather(tensor_list, tensor)


def dist_all_gather_into(out, tensor):
    """all_gather along dim 0 into ONE contiguous tensor (synchronous, like the others: see above)."""
    import torch.distributed as dist
    dist.all_gather_into_tensor(out, tensor)


def _distributed():
    """True when the data-parallel exchanges (SyncBN sums, key all-gather, gradient all-reduce) have to be issued."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size() > 1 or FORCE_COLLECTIVES


BN_SMALL_MAX_ROWS = 4096      # == MI_BN_SMALL_MAX_ROWS


def _bn_batch_sums(x, m, c, mod, sums=None, reduced=False):
    """(sums, count) of a training-mode BatchNorm over the (m, c) activation x: the column sums over the whole batch and its number
    of rows.  sums: this rank's, where the producer of x already has them (the statistics pass is skipped); reduced: they are
    the GLOBAL sums already - the caller has all-reduced them (paired with another branch's)."""
    if sums is None:
        sums = _bn_stats(x, m, c)
    count = float(m)
    if mod.sync and _distributed():
        if not reduced:
            dist_all_reduce(sums)                         # RCCL: 2*C doubles
        count = float(m) * _dist_world()
    return sums, count


def _bn_running_ptrs(mod, track):
    """The (running_mean, running_var, num_batches_tracked) arguments of a BatchNorm launch: null unless `track`."""
    if not track:
        return None, None, None
    return mod.running_mean, mod.running_var, mod.num_batches_tracked


def _bn_affine_grads(mod):
    """The _GradInto pair (dgamma, dbeta) of a BatchNorm backward: null targets without affine parameters or with frozen ones."""
    gamma = mod.weight
    wanted = gamma is not None and gamma.requires_grad
    return _GradInto(gamma if wanted else None), _GradInto(mod.bias if wanted else None)


def _bn_sync_bwd_sums(sums, c, dg, db, distributed):
    """Between the reduce and the apply launch of a BatchNorm backward: the (dgamma, dbeta) pointers the apply launch gets.
    Single process: that launch writes them from the sums.  Distributed: they come from the LOCAL sums here (torch.nn.SyncBatchNorm
    does the same; the data-parallel gradient averaging then treats them like every other parameter), the sums are all-reduced
    for dx and the apply launch gets null pointers."""
    if not distributed:
        return dg, db
    if dg is not None:
        L.call("mi_bn_param_grads", sums, c, dg, db)
    dist_all_reduce(sums)
    return None, None


class _BNFn(torch.autograd.Function):
    """y = act(bn(x) + res); res (optional) is a residual branch added before the activation."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mod, relu, res=None, res_slot=None, sums=None, reduced=False, applied=None):
        ctx.res_slot = res_slot if res is not None else None
        c = x.shape[-1]
        m = x.numel() // c
        train = mod.training or not mod.track_running_stats
        ctx.small = train and m <= BN_SMALL_MAX_ROWS and not (mod.sync and _distributed())
        ctx.count = float(m)
        ctx.train_stats = train
        track = mod.track_running_stats and mod.training
        if applied is not None:
            # (y, save) came out of the producing Linear's launch (linear_bn): nothing to run here
            if not ctx.small or res is not None:
                raise L.HipExtensionError("fused Linear+BatchNorm output handed to a BatchNorm that would not take the small path")
            y, save = applied
        else:
            y = torch.empty_like(x)
            save = torch.empty(2 * c, dtype=torch.float32, device=x.device)
            if ctx.small:
                # one launch: statistics, running statistics, affine (+res, ReLU)
                L.call("mi_bn_small_fwd", x, y, m, c, gamma, beta, mod.eps, mod.momentum, *_bn_running_ptrs(mod, track), save, res,
                       int(relu))
            elif train:
                sums, ctx.count = _bn_batch_sums(x, m, c, mod, sums, reduced)
                L.call("mi_bn_apply_fwd", x, y, m, c, sums, ctx.count, gamma, beta, mod.eps, mod.momentum, *_bn_running_ptrs(mod, track),
                       save, res, int(relu))
            else:
                L.call("mi_bn_eval_fwd", x, y, m, c, mod.running_mean, mod.running_var, gamma, beta, mod.eps, save, res, int(relu))
        ctx.mod, ctx.relu, ctx.m, ctx.c = mod, relu, m, c
        ctx.has_res = res is not None
        ctx.save_for_backward(x, y if relu else None, save)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, save = ctx.saved_tensors
        mod, relu, m, c = ctx.mod, ctx.relu, ctx.m, ctx.c
        dy = dy.contiguous()
        lib = L.lib()
        if not ctx.train_stats:
            raise L.HipExtensionError("BatchNorm backward in eval mode is not on the hot path")
        dres = None
        want_dres = False
        if ctx.has_res:
            # the residual branch receives the gradient behind the activation; BN continues from it
            if relu and not ctx.small:
                want_dres = True                          # (written by the apply launch below: no masking launch in front of the two)
            else:
                if relu:
                    dy = relu_mask(dy, y)
                    relu = False
                dres = dy
        gamma = mod.weight
        dx = torch.empty_like(x)
        if ctx.small:
            dgamma, dbeta = _bn_affine_grads(mod)
            with dgamma as dg, dbeta as db:
                L.call("mi_bn_small_bwd", dy, x, y, dx, m, c, save, gamma, int(relu), dg, db)
        else:
            ws = _ws(lib.mi_colreduce_workspace_bytes(m, c), x.device, "colreduce")
            sums = torch.empty(2 * c, dtype=torch.float64, device=x.device)
            L.call("mi_bn_bwd_reduce", dy, x, y, m, c, save, int(relu), sums, ws, ws.numel())
            dgamma, dbeta = _bn_affine_grads(mod)
            with dgamma as dg, dbeta as db:
                pg, pb = _bn_sync_bwd_sums(sums, c, dg, db, mod.sync and _distributed())
                if want_dres:
                    dres = torch.empty_like(dy)
                    L.call("mi_bn_bwd_apply_res", dy, x, y, dx, dres, m, c, save, gamma, sums, ctx.count, pg, pb)
                else:
                    L.call("mi_bn_bwd_apply", dy, x, y, dx, m, c, save, gamma, sums, ctx.count, int(relu), pg, pb)
        if ctx.res_slot is not None and dres is not None:
            # through the block's GradSlot when its first convolution adds the residual gradient in its own epilogue
            ctx.res_slot.tensor = dres
            dres = None
        return dx, None, None, None, None, dres, None, None, None, None


class _BNReluPoolFn(torch.autograd.Function):
    """MaxPool3d(k, s, p)(relu(bn(x))) without materialising relu(bn(x)): the stem of the 3-D encoder."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mod, k, stride, pad, sums=None, reduced=False):
        n, d, h, w, c = x.shape
        dev = x.device
        do, ho, wo = [(v + 2 * pad - k) // stride + 1 for v in (d, h, w)]
        y = torch.empty((n, do, ho, wo, c), dtype=torch.float32, device=dev)
        save = torch.empty(2 * c, dtype=torch.float32, device=dev)
        train = mod.training or not mod.track_running_stats
        arg = torch.empty((n, do, ho, wo, c), dtype=torch.uint8, device=dev) if (train and x.requires_grad) else None
        m = n * d * h * w
        sums, count = _bn_batch_sums(x, m, c, mod, sums, reduced) if train else (None, float(m))
        track = mod.track_running_stats and mod.training
        running_mean, running_var, _ = _bn_running_ptrs(mod, track or not train)     # (eval mode READS the running statistics)
        L.call("mi_bn_relu_maxpool3d_fwd", x, y, arg, n, d, h, w, c, k, stride, pad, sums, count, gamma, beta, mod.eps, mod.momentum,
               running_mean, running_var, mod.num_batches_tracked if track else None, save)
        ctx.mod, ctx.geom, ctx.count, ctx.train = mod, (n, d, h, w, c, k, stride, pad), count, train
        ctx.save_for_backward(x, save, arg)
        return y

    @staticmethod
    def backward(ctx, dp):
        x, save, arg = ctx.saved_tensors
        if not ctx.train or arg is None:
            raise L.HipExtensionError("fused BatchNorm+ReLU+MaxPool backward needs a training-mode forward")
        mod = ctx.mod
        n, d, h, w, c, k, stride, pad = ctx.geom
        lib = L.lib()
        dev = x.device
        dp = dp.contiguous()
        m = n * d * h * w
        sums = torch.empty(2 * c, dtype=torch.float64, device=dev)
        gamma, beta = mod.weight, mod.bias
        # the pool's backward materialised once, then BatchNorm's two halves with the ReLU mask recomputed from x
        dy = torch.empty_like(x)
        L.call("mi_maxpool3d_bwd", dp, arg, dy, n, d, h, w, c, k, stride, pad)
        ws = _ws(lib.mi_colreduce_workspace_bytes(m, c), dev, "colreduce")
        L.call("mi_bn_relu_bwd_reduce_x", dy, x, m, c, save, gamma, beta, sums, ws, ws.numel())
        dx = dy                                            # in place: each element is read, then written, by one thread
        dgamma, dbeta = _bn_affine_grads(mod)
        with dgamma as dg, dbeta as db:
            pg, pb = _bn_sync_bwd_sums(sums, c, dg, db, mod.sync and _distributed())
            L.call("mi_bn_relu_bwd_apply_x", dy, x, dx, m, c, save, gamma, beta, sums, ctx.count, pg, pb)
        return dx, None, None, None, None, None, None, None, None


def bn_relu_maxpool3d(x, bn, k, stride, pad, sums=None, reduced=False):
    """maxpool3d(bn(x, relu=True), k, stride, pad) as one fused layer (bn: HipBatchNorm).  sums: the column sums of x and
    x^2 (2C doubles) where the producer of x already has them (the stem's epilogue) - the statistics pass is skipped."""
    return _BNReluPoolFn.apply(_f32c(x, "x"), bn.weight, bn.bias, bn, k, stride, pad, sums, reduced)


def linear_bn(x, lin, bn, relu=False):
    """bn(lin(x), relu) for a HipLinear followed by a HipBatchNorm over a batch of at most 64 rows in ONE launch
    (mi_linear_bn_fwd_f32: the product's tile holds every row of its columns, so the batch statistics are the workgroup's
    own); both autograd nodes stay, with their backward passes.  Anything else (more rows, eval mode, SyncBN across ranks)
    runs the two launches."""
    train = bn.training or not bn.track_running_stats
    if not (x.is_cuda and x.dim() == 2 and x.shape[0] <= 64 and train and PROFILE is None):
        return bn(lin(x), relu=relu)
    # SyncBN across ranks: only the statistics come out of the product's epilogue (this rank's column sums); the all-reduce and
    # the apply stay launches of their own
    req = _BNFuse(bn, relu, stats_only=bool(bn.sync and _distributed()))
    xl = lin(x, fuse=req)
    return bn(xl, relu=relu, sums=req.sums, applied=req.applied)     # (through the module: forward hooks keep firing)


def linear_with_local_sums(x, lin, bn):
    """(lin(x), this rank's column sums of it) for a SyncBN whose all-reduce the CALLER issues (MoCo's layer-locked forward pairs it
    with the other encoder's): the sums come out of the product's epilogue where linear_bn's would, else from a statistics pass."""
    train = bn.training or not bn.track_running_stats
    req = None
    if x.is_cuda and x.dim() == 2 and x.shape[0] <= 64 and train and PROFILE is None:
        req = _BNFuse(bn, False, stats_only=True)
    xl = lin(x, fuse=req)
    if req is not None and req.sums is not None:
        return xl, req.sums
    return xl, bn_local_sums(xl)


class HipBatchNorm(nn.Module):
    """nn.BatchNorm3d / nn.BatchNorm1d over the last (channel) axis, optional fused ReLU."""

    def __init__(self, c, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.num_features, self.eps, self.momentum = c, eps, momentum
        self.affine, self.track_running_stats = affine, track_running_stats
        self.sync = False
        if affine:
            self.weight = nn.Parameter(torch.ones(c))
            self.bias = nn.Parameter(torch.zeros(c))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    def forward(self, x, relu=False, res=None, res_slot=None, sums=None, reduced=False, applied=None):
        """sums / reduced: as in bn_relu_maxpool3d.  applied: the (y, save) a fused Linear+BatchNorm launch produced (linear_bn)."""
        return _BNFn.apply(_f32c(x, "x"), self.weight, self.bias, self, relu, res, res_slot, sums, reduced, applied)


def convert_sync_batchnorm(module):
    """Counterpart of nn.SyncBatchNorm.convert_sync_batchnorm (moco_main.py:65-66): the same
    modules, with their per-channel sums all-reduced over RCCL."""
    for m in module.modules():
        if isinstance(m, HipBatchNorm):
            m.sync = True
    return module


# ------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------
class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, stride, pad):
        n, d, h, w, c = x.shape
        do, ho, wo = [(v + 2 * pad - k) // stride + 1 for v in (d, h, w)]
        y = torch.empty((n, do, ho, wo, c), dtype=torch.float32, device=x.device)
        arg = torch.empty((n, do, ho, wo, c), dtype=torch.uint8, device=x.device)
        L.call("mi_maxpool3d_fwd", x, y, arg, n, d, h, w, c, k, stride, pad)
        ctx.save_for_backward(arg)
        ctx.geom = (x.shape, k, stride, pad)
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        shape, k, stride, pad = ctx.geom
        n, d, h, w, c = shape
        dx = torch.empty(shape, dtype=torch.float32, device=dy.device)
        L.call("mi_maxpool3d_bwd", dy.contiguous(), arg, dx, n, d, h, w, c, k, stride, pad)
        return dx, None, None, None


def maxpool3d(x, k, stride, pad):
    return _MaxPoolFn.apply(_f32c(x, "x"), k, stride, pad)


class _AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        n = x.shape[0]
        c = x.shape[-1]
        s = x.numel() // (n * c)
        y = torch.empty((n, c), dtype=torch.float32, device=x.device)
        L.call("mi_avgpool_fwd", x, y, n, s, c)
        ctx.shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        shape = ctx.shape
        n, c = shape[0], shape[-1]
        s = 1
        for v in shape[1:-1]:
            s *= v
        dx = torch.empty(shape, dtype=torch.float32, device=dy.device)
        L.call("mi_avgpool_bwd", dy.contiguous(), dx, n, s, c)
        return dx


def global_avgpool(x):
    return _AvgPoolFn.apply(_f32c(x, "x"))


class _BNReluAvgPoolFn(torch.autograd.Function):
    """global_avgpool(relu(bn(x))) in the one launch of the small-M BatchNorm, forward and backward (the pooled sum runs in
    row order, the gradient is dy / V: the values of the separate avgpool kernels)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mod, v):
        c = x.shape[-1]
        m = x.numel() // c
        y = torch.empty_like(x)
        pooled = torch.empty((x.shape[0], c), dtype=torch.float32, device=x.device)
        save = torch.empty(2 * c, dtype=torch.float32, device=x.device)
        L.call("mi_bn_small_pool_fwd", x, y, pooled, m, c, v, gamma, beta, mod.eps, mod.momentum,
               *_bn_running_ptrs(mod, mod.track_running_stats and mod.training), save)
        ctx.mod, ctx.m, ctx.c, ctx.v = mod, m, c, v
        ctx.save_for_backward(x, y, save)
        return pooled

    @staticmethod
    def backward(ctx, dp):
        x, y, save = ctx.saved_tensors
        mod, m, c, v = ctx.mod, ctx.m, ctx.c, ctx.v
        dx = torch.empty_like(x)
        dgamma, dbeta = _bn_affine_grads(mod)
        with dgamma as dg, dbeta as db:
            L.call("mi_bn_small_pool_bwd", dp.contiguous(), x, y, dx, m, c, v, save, mod.weight, dg, db)
        return dx, None, None, None, None


def bn_relu_global_avgpool(x, bn):
    """AdaptiveAvgPool3d(1)(relu(bn(x))) -> (N, C): one launch each way when the one-launch BatchNorm applies (training
    statistics, <= BN_SMALL_MAX_ROWS rows, no SyncBN exchange, a power-of-two number of voxels per sample <= 64);
    otherwise the separate kernels."""
    _f32c(x, "x")
    n, c = x.shape[0], x.shape[-1]
    m = x.numel() // c
    v = m // max(n, 1)
    fused = (x.is_cuda and (bn.training or not bn.track_running_stats) and m <= BN_SMALL_MAX_ROWS and c % 4 == 0
             and not (bn.sync and _distributed()) and 1 <= v <= 64 and (v & (v - 1)) == 0 and v * n == m)
    if not fused:
        return global_avgpool(bn(x, relu=True))
    return _BNReluAvgPoolFn.apply(x, bn.weight, bn.bias, bn, v)


# ------------------------------------------------------------------------------------------------
# BasicBlock (moco_encoder_3d.py:55-84): conv-ReLU-conv (+residual) -ReLU, no BN, with the ReLU
# derivatives fused into the data-gradient epilogues
# ------------------------------------------------------------------------------------------------
RELU_TAP = None      # tests set a dict: post-ReLU activations of a forward pass (block: id(module) -> (mid, out); the encoder
                     # adds "feature_3d", "proj.1", "proj.4"), copies - so that a float64 oracle can take the SAME branch of the
                     # piecewise-linear network the GPU took where a unit sits within rounding of zero


class _BasicBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, w2, wds, blk, mask_dx=False, dout_masked=False):
        s = blk.stride
        front = conv_fwd_s2_block(x, w1, wds) if (s == 2 and wds is not None) else None
        if front is not None:
            hmid, r = front                                  # stride-2 front: conv1 + ReLU and the shortcut in one launch
        else:
            hmid = conv_fwd(x, w1, 3, s, 1, None, True)
            r = conv_fwd(x, wds, 1, s, 0) if wds is not None else x
        out = conv_fwd(hmid, w2, 3, 1, 1, r, True)
        if RELU_TAP is not None:                             # (tests: the ReLU decisions of this forward pass)
            RELU_TAP[id(blk)] = (hmid.detach().clone(), out.detach().clone())
        ctx.blk = blk
        ctx.mask_dx, ctx.dout_masked = mask_dx, dout_masked
        ctx.save_for_backward(x, hmid, out)
        ctx.x_needs_grad = x.requires_grad
        return out

    @staticmethod
    def backward(ctx, dout):
        x, hmid, out = ctx.saved_tensors
        blk = ctx.blk
        s = blk.stride
        # through the block's last ReLU - unless the consumer of `out` already did it in its data-gradient epilogue
        d2 = dout.contiguous() if ctx.dout_masked else relu_mask(dout.contiguous(), out)
        xmask = x if ctx.mask_dx else None                           # ... as this block does for ITS producer
        if blk.conv2.weight.requires_grad:
            conv_wgrad_into(hmid, d2, blk.conv2.weight, 3, 1, 1)
        dh = conv_dgrad(d2, blk.conv2.weight, hmid.shape, 3, 1, 1, None, hmid)   # * (hmid > 0) fused
        if blk.conv1.weight.requires_grad:
            conv_wgrad_into(x, dh, blk.conv1.weight, 3, s, 1)
        dx = None
        ds = blk.downsample
        if ds is not None:
            if ds[0].weight.requires_grad:
                conv_wgrad_into(x, d2, ds[0].weight, 1, s, 0)
            if ctx.x_needs_grad:
                # stride-2 block front: both data gradients (+ the ReLU mask) in one launch where the shape is the encoder's
                dx = conv_dgrad_s2_block(dh, d2, blk.conv1.weight, ds[0].weight, x.shape, None, xmask) if s == 2 else None
                if dx is None:
                    dres = conv_dgrad(d2, ds[0].weight, x.shape, 1, s, 0)
                    dx = conv_dgrad(dh, blk.conv1.weight, x.shape, 3, s, 1, dres, xmask)
        elif ctx.x_needs_grad:
            dx = conv_dgrad(dh, blk.conv1.weight, x.shape, 3, s, 1, d2, xmask)   # + identity branch fused
        return dx, None, None, None, None, None, None


def basic_block(x, blk, mask_dx=False, dout_masked=False):
    """mask_dx: x is the output of a ReLU whose derivative its producer leaves to this block - the returned gradient is
    (dx) * (x > 0), applied in the data-gradient epilogue (x > 0 exactly where the producer's pre-activation was).
    dout_masked: the ONE consumer of this block's output does the same for this block's last ReLU, so the backward skips
    its own mask launch.  The caller (the encoder's trunk) pairs the two flags; defaults keep the block self-contained."""
    wds = blk.downsample[0].weight if blk.downsample is not None else None
    return _BasicBlockFn.apply(_f32c(x, "x"), blk.conv1.weight, blk.conv2.weight, wds, blk, mask_dx, dout_masked)


# ------------------------------------------------------------------------------------------------
# contrastive head: normalise, logits, cross-entropy
# ------------------------------------------------------------------------------------------------
class _L2NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        b, c = x.shape
        y = torch.empty_like(x)
        inv = torch.empty(b, dtype=torch.float32, device=x.device)
        L.call("mi_l2norm_fwd", x, y, inv, b, c)
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        b, c = y.shape
        dx = torch.empty_like(y)
        L.call("mi_l2norm_bwd", dy.contiguous(), y, inv, dx, b, c)
        return dx


def l2_normalize(x):
    return _L2NormFn.apply(_f32c(x, "x"))


class _MocoLogitsFn(torch.autograd.Function):
    """logits = cat([q.k, q @ queue], 1) / T   (models/moco.py:130-138); gradient w.r.t. q only."""

    @staticmethod
    def forward(ctx, q, k, queue, T):
        b, c = q.shape
        r = queue.shape[1]
        logits = torch.empty((b, r + 1), dtype=torch.float32, device=q.device)
        L.call("mi_moco_logits_fwd", q, k, queue, logits, b, c, r, float(T))
        ctx.save_for_backward(k, queue.clone())      # the queue is overwritten by the enqueue below
        ctx.T = float(T)
        return logits

    @staticmethod
    def backward(ctx, dl):
        k, queue = ctx.saved_tensors
        b, c = k.shape
        r = queue.shape[1]
        dq = torch.empty_like(k)
        L.call("mi_moco_logits_bwd", dl.contiguous(), k, queue, dq, b, c, r, ctx.T)
        return dq, None, None, None


def moco_logits(q, k, queue, T):
    return _MocoLogitsFn.apply(_f32c(q, "q"), _f32c(k, "k"), _f32c(queue, "queue"), T)


class _MocoLogitsNormFn(torch.autograd.Function):
    """(logits, k_hat) from the un-normalised projections: normalize(q), normalize(k) and the logits in one launch; the
    backward is logits_bwd + l2norm_bwd on the saved q_hat / 1/|q| (gradient w.r.t. q_raw only).
    queue_stable: the caller enqueues only after the backward pass, so the queue needs no copy."""

    @staticmethod
    def forward(ctx, q_raw, k_raw, queue, T, queue_stable):
        b, c = q_raw.shape
        r = queue.shape[1]
        dev = q_raw.device
        logits = torch.empty((b, r + 1), dtype=torch.float32, device=dev)
        q_hat = torch.empty_like(q_raw)
        k_hat = torch.empty_like(q_raw)
        q_inv = torch.empty(b, dtype=torch.float32, device=dev)
        L.call("mi_moco_logits_norm_fwd", q_raw, k_raw, queue, logits, q_hat, q_inv, k_hat, b, c, r, float(T))
        ctx.save_for_backward(k_hat, queue if queue_stable else queue.clone(), q_hat, q_inv)
        ctx.T = float(T)
        ctx.mark_non_differentiable(k_hat)
        ctx.set_materialize_grads(False)        # (no zeros(B, C) launch for the key output's absent gradient)
        return logits, k_hat

    @staticmethod
    def backward(ctx, dl, _dk):
        if dl is None:
            return None, None, None, None, None
        k_hat, queue, q_hat, q_inv = ctx.saved_tensors
        b, c = k_hat.shape
        r = queue.shape[1]
        dq = torch.empty_like(k_hat)
        L.call("mi_moco_logits_bwd", dl.contiguous(), k_hat, queue, dq, b, c, r, ctx.T)
        dx = torch.empty_like(dq)
        L.call("mi_l2norm_bwd", dq, q_hat, q_inv, dx, b, c)
        return dx, None, None, None, None


def moco_logits_normalized(q_raw, k_raw, queue, T, queue_stable=False):
    """models/moco.py:113-138 from the encoders' raw outputs; returns (logits, normalize(k))."""
    return _MocoLogitsNormFn.apply(_f32c(q_raw, "q"), _f32c(k_raw, "k"), _f32c(queue, "queue"), T, bool(queue_stable))


_CE0_COUNTERS = {}       # device -> (int32 tensor of 64 self-resetting arrival counters, {stream id: slot})


def _ce0_counter(device):
    """The arrival counter of this stream's cross-entropy launches: one 4-byte word per stream out of a per-device table that
    is zeroed ONCE, when it is created (a per-stream workspace would be created - and its clearing pass captured - inside a
    hipGraph capture, whose capture stream is a new one: a fill launch in every replay).  Launches on different streams never
    share a word; the kernel leaves its word zero."""
    key = (device.type, device.index)
    ent = _CE0_COUNTERS.get(key)
    if ent is None:
        ent = (torch.zeros(64 * 64, dtype=torch.int32, device=device), {})      # 64 words, 256 bytes apart
        _CE0_COUNTERS[key] = ent
    table, slots = ent
    sid = torch.cuda.current_stream(device).cuda_stream
    slot = slots.get(sid)
    if slot is None:
        if len(slots) >= 64:
            # never alias: two live streams on one arrival word mix their tickets (a wrong or missing loss write)
            raise L.HipExtensionError("cross_entropy_label0 has been launched on 64 distinct HIP streams of %s; "
                                    "hipops.reset_ce0_counters() releases the words of streams that no longer exist" % (device,))
        slot = len(slots)
        slots[sid] = slot
    return table[slot * 64:]


def reset_ce0_counters(device=None):
    """Forget the stream -> arrival-word table (all devices, or one).  Call it only with no cross-entropy launch in flight
    and outside a hipGraph capture; graphs captured before keep the addresses of the old table alive through their tensors."""
    for key in list(_CE0_COUNTERS):
        if device is None or key == (device.type, device.index):
            del _CE0_COUNTERS[key]


class _CELabel0Fn(torch.autograd.Function):
    """forward = one launch (a workgroup per row, the last one takes the mean) that also drops the loss into `out` (the
    engine's loss buffer: no copy afterwards); backward = one launch that reads the upstream gradient on the device."""

    @staticmethod
    def forward(ctx, logits, out):
        b, n = logits.shape
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        rows = torch.empty(3 * b, dtype=torch.float32, device=logits.device)          # row losses | row maxima | log row sums
        word = _ce0_counter(logits.device)
        try:
            L.call("mi_ce_label0_fwd", logits, loss, out, rows, rows[b:], b, n, word)
        except L.HipExtensionError:
            if not torch.cuda.is_current_stream_capturing():
                word[:1].zero_()                       # a launch that failed midway must not leave its tickets behind
            raise
        ctx.save_for_backward(logits, rows)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, rows = ctx.saved_tensors
        b, n = logits.shape
        dl = torch.empty_like(logits)
        L.call("mi_ce_label0_bwd", logits, rows[b:], g.contiguous(), dl, b, n)
        return dl, None


def cross_entropy_label0(logits, out=None):
    """nn.CrossEntropyLoss()(logits, zeros) (trains/tomo_moco_trainer.py:52,73).  `out`: a 0-d fp32 device tensor that
    receives the loss (and is returned)."""
    return _CELabel0Fn.apply(_f32c(logits, "logits"), out)


class _RowDotMeanFn(torch.autograd.Function):
    """mean_b(a_b . b_b); gradient w.r.t. a only (b is the detached target)."""

    @staticmethod
    def forward(ctx, a, b):
        bsz, c = a.shape
        out = torch.empty((), dtype=torch.float32, device=a.device)
        L.call("mi_rowdot_mean_fwd", a, b, out, bsz, c)
        ctx.save_for_backward(b)
        return out

    @staticmethod
    def backward(ctx, g):
        (b,) = ctx.saved_tensors
        da = torch.empty_like(b)
        L.call("mi_rowdot_mean_bwd", b, g.contiguous(), da, b.shape[0], b.shape[1])
        return da, None


def rowdot_mean(a, b):
    return _RowDotMeanFn.apply(_f32c(a, "a"), _f32c(b, "b"))


def column_std_mean(x):
    """torch.std(x, 0).mean() (the SimSiam `output_std` monitor).  A single row (B = 1) has no spread: the result is 0,
    where torch.std gives NaN; a column whose variance rounds below zero counts as 0."""
    out = torch.empty((), dtype=torch.float32, device=x.device)
    L.call("mi_column_std_mean", _f32c(x, "x"), out, x.shape[0], x.shape[1])
    return out


# ------------------------------------------------------------------------------------------------
# optimiser-side passes
# ------------------------------------------------------------------------------------------------
def ema_update_(k_flat, q_flat, m):
    _bump_weight_epoch()                 # a raw-pointer write: torch's version counters do not see it
    L.call("mi_ema_update", k_flat, q_flat, float(m), k_flat.numel())


def sgd_step_(p_flat, g_flat, lr, weight_decay=0.0, lr_dev=None, grad_scale=1.0):
    """p -= lr * (grad_scale * g + wd * p); grad_scale = 1 / world when g is the SUM of the ranks' gradients."""
    _bump_weight_epoch()
    L.call("mi_sgd_step", p_flat, g_flat, lr_dev, float(lr), float(weight_decay), float(grad_scale), p_flat.numel())


def sgd_step2_(p_flat, g_flat, g2_flat, lr, weight_decay=0.0, lr_dev=None, grad_scale=1.0):
    """p -= lr * (grad_scale * (g + g2) + wd * p): two gradient arenas (one per view of a two-view model)."""
    _bump_weight_epoch()
    L.call("mi_sgd_step2", p_flat, g_flat, g2_flat, lr_dev, float(lr), float(weight_decay), float(grad_scale), p_flat.numel())


def scalar_accumulate_(sums, *scalars):
    """sums[i] += scalars[i] (0-d / 1-element f32 device tensors, at most four) in one launch."""
    if len(scalars) > 4 or sums.numel() < len(scalars):
        raise L.HipExtensionError("scalar_accumulate_: at most four scalars, sums at least as long")
    L.call("mi_scalar_accumulate", sums, *[_f32c(t, "scalar") for t in scalars], *[None] * (4 - len(scalars)))


def copy_pair_(dst0, src0, dst1, src1):
    """dst0.copy_(src0); dst1.copy_(src1) - as ONE launch when the four are contiguous f32 device tensors of one size."""
    ts = (dst0, src0, dst1, src1)
    if (all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ts) and src0.shape == dst0.shape
            and src1.shape == dst1.shape and dst0.numel() == dst1.numel() and dst0.numel() % 4 == 0
            and all(t.data_ptr() % 16 == 0 for t in ts)):
        L.call("mi_copy_pair_f32", dst0, src0, dst1, src1, dst0.numel())
        return
    dst0.copy_(src0)
    dst1.copy_(src1)


def queue_enqueue_(queue, queue_ptr, keys):
    c, r = queue.shape
    b = keys.shape[0]
    if r % b != 0:
        raise AssertionError("queue size must be a multiple of the batch (models/moco.py:47)")
    L.call("mi_queue_enqueue", queue, queue_ptr, keys, b, c, r)


# ------------------------------------------------------------------------------------------------
# detector network glue (models/networks/unet.py): ceil-mode max-pool, 2x2 transposed conv, concat, bias, z head
# ------------------------------------------------------------------------------------------------
class _MaxPool2dCeilFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        n, h, w, c = x.shape
        ho, wo = (h + k - 1) // k, (w + k - 1) // k
        y = torch.empty((n, ho, wo, c), dtype=torch.float32, device=x.device)
        arg = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device) if x.requires_grad else None
        L.call("mi_maxpool2d_ceil_fwd", x, y, arg, n, h, w, c, k)
        ctx.save_for_backward(arg)
        ctx.geom = (x.shape, k)
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        shape, k = ctx.geom
        n, h, w, c = shape
        dx = torch.empty(shape, dtype=torch.float32, device=dy.device)
        L.call("mi_maxpool2d_ceil_bwd", dy.contiguous(), arg, dx, n, h, w, c, k)
        return dx, None


def maxpool2d_ceil(x, k=2):
    """nn.MaxPool2d(k, ceil_mode=True) on (N,H,W,C)."""
    return _MaxPool2dCeilFn.apply(_f32c(x, "x"), k)


def _colsum_job(dy2d, param):
    """The launch `param.grad (+)= column sums of dy2d (M, C)` as a closure: the gradient's target is bound here, the launch runs
    when the closure is called (now, or from the side-stream batch: _side_or_now)."""
    dest = _GradInto(param)
    def launch():
        m, c = dy2d.shape
        lib = L.lib()
        ws = _ws(lib.mi_colreduce_workspace_bytes(m, c), dy2d.device, "colreduce")
        sums = torch.empty(2 * c, dtype=torch.float64, device=dy2d.device)
        with dest as tgt:
            L.call("mi_colsum", dy2d, m, c, tgt, sums, ws, ws.numel())
    return launch


def _colsum_into(dy2d, param):
    """param.grad (+)= column sums of dy2d (M, C)."""
    _colsum_job(dy2d, param)()


class _ConvT2x2Fn(torch.autograd.Function):
    """nn.ConvTranspose2d(ci, co, 2, stride=2) cropped to (ho, wo): 1x1 implicit GEMM to 4*co columns + pixel shuffle."""

    @staticmethod
    def forward(ctx, x, w, bias, mod, ho, wo, inference=False):
        n, h, wd, ci = x.shape
        co = mod.co
        t = conv_fwd(x, mod.gemm_view(), 1, 1, 0, owner=mod.weight, inference=inference)
        y = torch.empty((n, ho, wo, co), dtype=torch.float32, device=x.device)
        L.call("mi_shuffle2x2_fwd", t, bias, y, n, h, wd, co, ho, wo)
        ctx.save_for_backward(x)
        ctx.mod, ctx.out_hw = mod, (ho, wo)
        ctx.x_needs_grad = x.requires_grad
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        mod = ctx.mod
        n, h, wd, ci = x.shape
        co = mod.co
        ho, wo = ctx.out_hw
        dy = dy.contiguous()
        dt = torch.empty((n, h, wd, 4 * co), dtype=torch.float32, device=dy.device)
        L.call("mi_shuffle2x2_bwd", dy, dt, n, h, wd, co, ho, wo)
        if mod.bias is not None and mod.bias.requires_grad:
            _colsum_into(dy.view(-1, co), mod.bias)
        if mod.weight.requires_grad:
            # the gradient tensor has the parameter's strides, i.e. the GEMM layout [ci][4*co]
            geom = _Geom((n, 1, h, wd, ci), 4 * co, (1, 1, 1), 1, (0, 0, 0))
            ws = geom.workspace(x.device)
            with _GradInto(mod.weight) as tgt:
                L.call("mi_conv_wgrad_f32", x, dt, tgt, geom.ref, ws, ws.numel(), None)
        dx = conv_dgrad(dt, mod.gemm_view(), x.shape, 1, 1, 0) if ctx.x_needs_grad else None
        return dx, None, None, None, None, None, None


class HipConvTranspose2x2(nn.Module):
    """nn.ConvTranspose2d(ci, co, kernel_size=2, stride=2): weight logical (ci, co, 2, 2) over storage [ci][a][b][co]."""

    def __init__(self, ci, co):
        super().__init__()
        self.ci, self.co = ci, co
        self.weight = nn.Parameter(torch.empty(ci, 2, 2, co).permute(0, 3, 1, 2))
        self.bias = nn.Parameter(torch.zeros(co))
        with torch.no_grad():
            bound = 1.0 / (co * 4) ** 0.5             # torch's fan_in of a transposed conv weight = size(1) * k*k
            self.weight.uniform_(-bound, bound)
            self.bias.uniform_(-bound, bound)

    def gemm_view(self):
        """the same storage as a (4*co, ci, 1, 1) convolution weight in kernel layout"""
        return torch.as_strided(self.weight, (4 * self.co, self.ci, 1, 1), (1, 4 * self.co, 4 * self.co * self.ci,
                                                                            4 * self.co * self.ci))

    def forward(self, x, ho=None, wo=None):
        n, h, w, _ = x.shape
        return _ConvT2x2Fn.apply(_f32c(x, "x"), self.weight, self.bias, self, 2 * h if ho is None else ho,
                                 2 * w if wo is None else wo, inference_mode())


class _ConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ca, cb = a.shape[-1], b.shape[-1]
        m = a.numel() // ca
        out = torch.empty(a.shape[:-1] + (ca + cb,), dtype=torch.float32, device=a.device)
        L.call("mi_concat_channels", a, ca, b, cb, out, m)
        ctx.shapes = (a.shape, b.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        sa, sb = ctx.shapes
        da = torch.empty(sa, dtype=torch.float32, device=dout.device)
        db = torch.empty(sb, dtype=torch.float32, device=dout.device)
        L.call("mi_split_channels", dout.contiguous(), da, sa[-1], db, sb[-1], da.numel() // sa[-1])
        return da, db


def concat_channels(a, b):
    """torch.cat((a, b), 1) of the reference (channel axis) on channels-last tensors."""
    return _ConcatFn.apply(_f32c(a, "a"), _f32c(b, "b"))


class _BiasAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, holder):
        y = x.clone()
        c = x.shape[-1]
        L.call("mi_bias_add", y, bias, y.numel() // c, c)
        ctx.holder = holder
        return y

    @staticmethod
    def backward(ctx, dy):
        b = ctx.holder.bias
        if b.requires_grad:
            _colsum_into(dy.contiguous().view(-1, dy.shape[-1]), b)
        return dy, None, None


def bias_add(x, holder):
    """x + holder.bias over the channel axis; the bias gradient goes to holder.bias.grad."""
    return _BiasAddFn.apply(_f32c(x, "x"), holder.bias, holder)


class _ZHeadFn(torch.autograd.Function):
    """nn.Conv3d(C, K, (3,1,1), padding=(1,0,0), bias=False) with K <= 4 on (N,D,H,W,C)."""

    @staticmethod
    def forward(ctx, x, w, mod):
        n, d, h, wd, c = x.shape
        k = mod.k_out
        y = torch.empty((n, d, h, wd, k), dtype=torch.float32, device=x.device)
        L.call("mi_zhead_fwd", x, w, y, n, d, h * wd, c, k)
        ctx.save_for_backward(x)
        ctx.mod = mod
        ctx.x_needs_grad = x.requires_grad
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        mod = ctx.mod
        n, d, h, wd, c = x.shape
        k = mod.k_out
        lib = L.lib()
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.x_needs_grad else None
        ws = _ws(lib.mi_zhead_bwd_workspace_bytes(n, d, h * wd, c, k), x.device, "zhead")
        with _GradInto(mod.weight if mod.weight.requires_grad else None) as tgt:
            L.call("mi_zhead_bwd", x, mod.weight, dy, dx, tgt, n, d, h * wd, c, k, ws, ws.numel())
        return dx, None, None


class HipZHead(nn.Module):
    """The (3,1,1) head with <= 4 outputs: weight logical (K, C, 3, 1, 1) over storage [3][C][K]."""

    def __init__(self, c, k_out):
        super().__init__()
        self.c, self.k_out = c, k_out
        self.weight = nn.Parameter(torch.empty(3, 1, 1, c, k_out).permute(4, 3, 0, 1, 2))
        with torch.no_grad():
            self.weight.normal_(std=0.001)

    def forward(self, x):
        # mi_zhead_fwd takes any C % 4 == 0, mi_zhead_bwd only a C that divides 256 (its weight-gradient block is 256 / C row groups):
        # say so here, where the graph is built, not as a bad-argument code out of the middle of backward()
        if 256 % self.c and torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad):
            raise L.HipExtensionError("HipZHead(%d, %d) runs at inference only (under torch.no_grad()): its backward kernels take a "
                                      "channel count that divides 256 (4, 8, ..., 256)" % (self.c, self.k_out))
        return _ZHeadFn.apply(_f32c(x, "x"), self.weight, self)



# ---- k-means over the exploration embeddings (csrc/kmeans.hip) -----------------------------------------------------------

def _km_x(x, name="x"):
    x = L.require_cuda(x, name)
    if x.dim() != 2 or not x.is_contiguous():
        raise L.HipExtensionError("%s must be a contiguous (N, d) tensor, got %s" % (name, tuple(x.shape)))
    return x


def kmeans_workspace(n, d, k, device):
    nbytes = L.lib().mi_kmeans_workspace_bytes(n, d, k)
    if nbytes == 0:
        L.check(-3, "mi_kmeans_workspace_bytes(n=%d, d=%d, k=%d)" % (n, d, k))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def kmeans_prep(centroids, image=None):
    """The centroids' operand image for kmeans_assign (once per iteration)."""
    c = _km_x(centroids, "centroids")
    k, d = c.shape
    nbytes = L.lib().mi_kmeans_image_bytes(d, k)
    if nbytes == 0:
        L.check(-3, "mi_kmeans_image_bytes(d=%d, k=%d)" % (d, k))
    if image is None:
        image = torch.empty(nbytes, dtype=torch.uint8, device=c.device)
    L.call("mi_kmeans_prep", c, d, k, image)
    return image


def kmeans_xnorm(x, out=None):
    x = _km_x(x)
    if out is None:
        out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    L.call("mi_kmeans_xnorm", x, x.shape[0], x.shape[1], out)
    return out


def kmeans_assign(x, xnorm, image, k, labels=None, dist=None, ws=None):
    """labels (N,) int32 = nearest centroid (lowest index on ties), dist (N,) fp32 = squared distance to it."""
    x = _km_x(x)
    n, d = x.shape
    L.require_cuda(xnorm, "xnorm")
    L.require_cuda(image, "image", torch.uint8)
    if ws is None:
        ws = kmeans_workspace(n, d, k, x.device)
    if labels is None:
        labels = torch.empty(n, dtype=torch.int32, device=x.device)
    if dist is None:
        dist = torch.empty(n, dtype=torch.float32, device=x.device)
    L.call("mi_kmeans_assign", x, xnorm, image, n, d, k, labels, dist, ws, ws.numel())
    return labels, dist


def kmeans_update(x, labels, centroids, counts=None, obj=None, nsplit=None, ws=None):
    """centroids (k, d), in place: the mean of the rows of each label, then the empty-cluster rule; counts (k,) int32.
    obj (1,) fp32 / nsplit (1,) int32: device slots for the objective of the preceding kmeans_assign on `ws` and the running
    number of empty clusters served."""
    x = _km_x(x)
    c = _km_x(centroids, "centroids")
    n, d = x.shape
    k = c.shape[0]
    if c.shape[1] != d:
        raise L.HipExtensionError("centroids are %s, x is %s" % (tuple(c.shape), tuple(x.shape)))
    L.require_cuda(labels, "labels", torch.int32)
    if ws is None:
        ws = kmeans_workspace(n, d, k, x.device)
    if counts is None:
        counts = torch.empty(k, dtype=torch.int32, device=x.device)
    L.call("mi_kmeans_update", x, labels, n, d, k, c, counts, obj, nsplit, ws, ws.numel())
    return counts


# ---- k-nearest-neighbour search over embeddings (csrc/knn.hip) -----------------------------------------------------------

KNN_METRICS = {"ip": 0, "l2": 1}          # MI_KNN_IP, MI_KNN_L2


def knn_search(q, x, k, metric="ip", exclude_self=False, n_split=0, out=None):
    """(index (M, k) int32, value (M, k) fp32): the k best rows of x (N, d) for every row of q (M, d), best first, the lowest
    index first among equal values.  metric "ip": value q.x, larger is better; "l2": value |q|^2 + (|x|^2 - 2 q.x) clamped
    at 0, smaller is better.  exclude_self leaves column j out for query row j.  n_split: parts the database is divided
    into (0: chosen by the library); the result does not depend on it."""
    q, x = _km_x(q, "q"), _km_x(x)
    if metric not in KNN_METRICS:
        raise L.HipExtensionError("metric must be 'ip' or 'l2', got %r" % (metric,))
    (m, d), n = q.shape, x.shape[0]
    k, n_split, excl = int(k), int(n_split), int(bool(exclude_self))
    if x.shape[1] != d or x.device != q.device:
        raise L.HipExtensionError("q is %s on %s, x is %s on %s" % (tuple(q.shape), q.device, tuple(x.shape), x.device))
    what = "(M=%d, N=%d, d=%d, k=%d, exclude_self=%d, n_split=%d)" % (m, n, d, k, excl, n_split)
    nbytes = L.lib().mi_knn_workspace_bytes(m, n, d, k, excl, n_split)
    if nbytes == 0:
        L.check(-3, "mi_knn_workspace_bytes" + what)
    if out is None:
        out = (torch.empty(m, k, dtype=torch.int32, device=q.device), torch.empty(m, k, dtype=torch.float32, device=q.device))
    index, value = L.require_cuda(out[0], "out[0]", torch.int32), L.require_cuda(out[1], "out[1]")
    if tuple(index.shape) != (m, k) or tuple(value.shape) != (m, k) or not index.is_contiguous() or not value.is_contiguous():
        raise L.HipExtensionError("out must be contiguous (%d, %d) tensors" % (m, k))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    L.call("mi_knn_search", q, x, m, n, d, k, KNN_METRICS[metric], excl, n_split, index, value, ws, ws.numel())
    return index, value


def embed_pool(x, out=None):
    """(n, dim) unit rows from the (n, P, dim) embeddings of P poses of every pick (csrc/crop_pose.hip): F.normalize of every
    row, the mean over P, F.normalize again.  P == 1 is F.normalize(x[:, 0], dim=1): the rows the k-NN search and the
    memory bank take."""
    L.require_cuda(x, "x")
    if x.dim() != 3 or not x.is_contiguous():
        raise L.HipExtensionError("x must be a contiguous (n, P, dim) tensor, got %s" % (tuple(x.shape),))
    n, p, d = x.shape
    if out is None:
        out = torch.empty(n, d, dtype=torch.float32, device=x.device)
    elif tuple(L.require_cuda(out, "out").shape) != (n, d) or not out.is_contiguous():
        raise L.HipExtensionError("out must be a contiguous (%d, %d) tensor" % (n, d))
    L.call("mi_embed_pool", x, n, p, d, out)
    return out


# ---- the neighbour graph of the t-SNE, UMAP and spectral kernels (csrc/knn_graph.h) ----------------------------------------

def _table(t, name, shape, dtype=torch.float32):
    L.require_cuda(t, name, dtype)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise L.HipExtensionError("%s must be a contiguous %s tensor, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t


def _graph_tables(index, rev_ptr=None, rev_edge=None, n=None, transpose=True, **tables):
    """(N, k) of the graph index (N, k) int32 (N = n where given), after checking it, its transpose (rev_ptr (N + 1,), rev_edge
    (N k,) int32: utils/graph.reverse_graph; transpose=False for an entry that takes none), and the per-edge tables (N, k),
    each passed as name=(tensor, dtype)."""
    L.require_cuda(index, "index", torch.int32)
    if index.dim() != 2 or (n is not None and index.shape[0] != n):
        raise L.HipExtensionError("index must be (N, k)%s, got %s" % ("" if n is None else " with N = %d" % n, tuple(index.shape)))
    n, k = index.shape
    _table(index, "index", (n, k), torch.int32)
    for name, (t, dtype) in tables.items():
        _table(t, name, (n, k), dtype)
    if transpose:
        _table(rev_ptr, "rev_ptr", (n + 1,), torch.int32)
        _table(rev_edge, "rev_edge", (n * k,), torch.int32)
    return n, k


# ---- t-SNE over the neighbour graph (csrc/tsne.hip) ------------------------------------------------------------------------


def tsne_affinities(dist, perplexity):
    """(p (N, K) fp32, beta (N,) fp32): the conditional affinities exp(-beta d) / sum of every row of dist (N, K), the row's
    beta found by sklearn's binary search for the entropy ln(perplexity); p is evaluated at the fp32 beta returned."""
    dist = _km_x(dist, "dist")
    n, k = dist.shape
    p = torch.empty(n, k, dtype=torch.float32, device=dist.device)
    beta = torch.empty(n, dtype=torch.float32, device=dist.device)
    L.call("mi_tsne_affinities", dist, n, k, float(perplexity), p, beta)
    return p, beta


def tsne_workspace(n, k, n_split, device):
    nbytes = L.lib().mi_tsne_workspace_bytes(n, k, n_split)
    if nbytes == 0:
        L.check(-3, "mi_tsne_workspace_bytes(N=%d, K=%d, n_split=%d)" % (n, k, n_split))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def tsne_gradient(y, index, p, rev_ptr, rev_edge, exaggeration=1.0, n_split=0, kl=True, out=None, ws=None):
    """(grad (N, 2) fp32, z (1,) fp32, kl (1,) fp32 or None): the exact t-SNE gradient of y (N, 2) for the graph index (N, K)
    int32 with conditional affinities p (N, K) and its transpose (rev_ptr, rev_edge: utils/graph.reverse_graph); z = the sum
    of q over i != j; kl (kl=True) the divergence without the exaggeration.  n_split: parts of the all-pairs sum (0: from N)."""
    y = _km_x(y, "y")
    n = y.shape[0]
    if y.shape[1] != 2:
        raise L.HipExtensionError("y must be (N, 2), got %s" % (tuple(y.shape),))
    n, k = _graph_tables(index, rev_ptr, rev_edge, n=n, p=(p, torch.float32))
    n_split = int(n_split)
    if ws is None:
        ws = tsne_workspace(n, k, n_split, y.device)
    if out is None:
        out = (torch.empty(n, 2, dtype=torch.float32, device=y.device), torch.empty(1, dtype=torch.float32, device=y.device),
               torch.empty(1, dtype=torch.float32, device=y.device) if kl else None)
    grad, z, klt = _table(out[0], "out[0]", (n, 2)), _table(out[1], "out[1]", (1,)), out[2] if kl else None
    if klt is not None:
        _table(klt, "out[2]", (1,))
    L.call("mi_tsne_gradient", y, index, p, rev_ptr, rev_edge, n, k, float(exaggeration), n_split, grad, z, klt, ws, ws.numel())
    return grad, z, klt


def tsne_update(y, grad, velocity, gains, momentum, lr, min_gain=0.01):
    """sklearn's gradient-descent step with gains, in place on y, velocity and gains (all (N, 2) fp32)."""
    y = _km_x(y, "y")
    for t, name in ((grad, "grad"), (velocity, "velocity"), (gains, "gains")):
        _table(t, name, tuple(y.shape))
    if y.shape[1] != 2:
        raise L.HipExtensionError("y must be (N, 2), got %s" % (tuple(y.shape),))
    L.call("mi_tsne_update", y, grad, velocity, gains, y.shape[0], float(momentum), float(lr), float(min_gain))
    return y


# ---- UMAP over the neighbour graph (csrc/umap.hip) -------------------------------------------------------------------------

def umap_smooth_knn(dist2, mean_all):
    """(rho (N,), sigma (N,), w (N, k)) fp32 of the squared distances dist2 (N, k) to the k = n_neighbors - 1 nearest other
    points: umap-learn's smooth_knn_dist and membership weights.  mean_all: sum of all sqrt(dist2) / (N (k + 1))."""
    dist2 = _km_x(dist2, "dist2")
    n, k = dist2.shape
    rho = torch.empty(n, dtype=torch.float32, device=dist2.device)
    sigma, w = torch.empty_like(rho), torch.empty_like(dist2)
    L.call("mi_umap_smooth_knn", dist2, n, k, float(mean_all), rho, sigma, w)
    return rho, sigma, w


def umap_union(index, w, rev_ptr, rev_edge, n_epochs, wmax=None, out=None):
    """(wsym (N, k) fp32, mutual (N, k) uint8, eps (N, k) float64) of the graph index (N, k) int32 with membership weights w and
    its transpose (utils/graph.reverse_graph).  wmax: a (1,) fp32 device tensor holding the largest wsym; without it eps is not
    written (the first of the two launches: wsym, its maximum by torch, then the spacings)."""
    n, k = _graph_tables(index, rev_ptr, rev_edge, w=(w, torch.float32))
    if wmax is not None:
        _table(wmax, "wmax", (1,))
    if out is None:
        out = (torch.empty(n, k, dtype=torch.float32, device=w.device), torch.empty(n, k, dtype=torch.uint8, device=w.device),
               torch.empty(n, k, dtype=torch.float64, device=w.device))
    wsym, mutual, eps = _table(out[0], "out[0]", (n, k)), _table(out[1], "out[1]", (n, k), torch.uint8), \
        _table(out[2], "out[2]", (n, k), torch.float64)
    L.call("mi_umap_union", index, w, rev_ptr, rev_edge, n, k, wmax, int(n_epochs), wsym, mutual, eps)
    return wsym, mutual, eps


def umap_rowmax(index, wsym, label, rev_ptr, rev_edge, f_far, f_unknown):
    """rowmax (N,) float64 of the label-supervised map: the largest wsym f over the pairs of every vertex (its forward edges and
    its reverse list), f = f_unknown where an end has a negative label (N,) int32, f_far where the labels differ, else 1."""
    n, k = _graph_tables(index, rev_ptr, rev_edge, wsym=(wsym, torch.float32))
    _table(label, "label", (n,), torch.int32)
    rowmax = torch.empty(n, dtype=torch.float64, device=wsym.device)
    L.call("mi_umap_rowmax", index, wsym, label, rev_ptr, rev_edge, n, k, float(f_far), float(f_unknown), rowmax)
    return rowmax


def umap_supervise(index, wsym, label, rowmax, f_far, f_unknown, n_epochs, wmax=None, out=None):
    """(wsup (N, k) fp32, eps (N, k) float64): umap-learn's categorical intersection and reset_local_connectivity per directed
    edge, wsup = p + q - p q with p = wsym f / rowmax_i, q = wsym f / rowmax_j, and the spacings of wsup.  wmax: a (1,) fp32
    device tensor holding the largest wsup; without it eps is not written (the two launches of umap_union)."""
    n, k = _graph_tables(index, transpose=False, wsym=(wsym, torch.float32))
    _table(label, "label", (n,), torch.int32)
    _table(rowmax, "rowmax", (n,), torch.float64)
    if wmax is not None:
        _table(wmax, "wmax", (1,))
    if out is None:
        out = (torch.empty(n, k, dtype=torch.float32, device=wsym.device), torch.empty(n, k, dtype=torch.float64, device=wsym.device))
    wsup, eps = _table(out[0], "out[0]", (n, k)), _table(out[1], "out[1]", (n, k), torch.float64)
    L.call("mi_umap_supervise", index, wsym, label, rowmax, n, k, float(f_far), float(f_unknown), wmax, int(n_epochs), wsup, eps)
    return wsup, eps


def umap_epoch(y_in, y_out, index, rev_ptr, rev_edge, mutual, eps, epoch, n_epochs, a, b, seed):
    """y_out = y_in + alpha (the attractions and negatives of the incident pairs that fire at `epoch` of n_epochs), every vertex
    from y_in alone (the epoch-synchronous form of umap-learn's loop); y_in, y_out (N, 2) fp32, two different buffers."""
    y_in = _km_x(y_in, "y_in")
    n = y_in.shape[0]
    if y_in.shape[1] != 2:
        raise L.HipExtensionError("y_in must be (N, 2), got %s" % (tuple(y_in.shape),))
    _table(y_out, "y_out", (n, 2))
    if y_out.data_ptr() == y_in.data_ptr():
        raise L.HipExtensionError("y_out may not alias y_in")
    n, k = _graph_tables(index, rev_ptr, rev_edge, n=n, mutual=(mutual, torch.uint8), eps=(eps, torch.float64))
    L.call("mi_umap_epoch", y_in, y_out, index, rev_ptr, rev_edge, mutual, eps, n, k, int(epoch), int(n_epochs), float(a), float(b),
           int(seed) & (2 ** 64 - 1))
    return y_out


# ---- the spectral start of the UMAP map (csrc/spectral.hip) ----------------------------------------------------------------

def graph_components(index, eps, mutual, rev_ptr, rev_edge):
    """(label (N,) int32, sweeps): the smallest vertex id of every vertex's connected component in the graph the UMAP epochs walk
    (forward edges and lone reverse edges, finite eps only).  One launch per sweep; the device flag is read between launches."""
    n, k = _graph_tables(index, rev_ptr, rev_edge, eps=(eps, torch.float64), mutual=(mutual, torch.uint8))
    a = torch.arange(n, dtype=torch.int32, device=index.device)
    b, flag = torch.empty_like(a), torch.zeros(1, dtype=torch.int32, device=index.device)
    sweeps = 0
    while True:
        flag.zero_()
        L.call("mi_graph_components", index, eps, mutual, rev_ptr, rev_edge, n, k, a, b, flag)
        a, b = b, a
        sweeps += 1
        if int(flag.item()) == 0:
            return a, sweeps


def spectral_degree(index, wsym, eps, mutual, rev_ptr, rev_edge):
    """(deg (N,), dis (N,)) float64: the sum of every vertex's incident weights and 1 / sqrt of it (0 for an isolated vertex)."""
    n, k = _graph_tables(index, rev_ptr, rev_edge, eps=(eps, torch.float64), mutual=(mutual, torch.uint8),
                         wsym=(wsym, torch.float32))
    deg = torch.empty(n, dtype=torch.float64, device=index.device)
    dis = torch.empty_like(deg)
    L.call("mi_spectral_degree", index, wsym, eps, mutual, rev_ptr, rev_edge, n, k, deg, dis)
    return deg, dis


def spectral_spmv(index, wsym, eps, mutual, rev_ptr, rev_edge, dis, x, y=None, row0=0):
    """y = A x, A = D^-1/2 W D^-1/2 restricted to the rows [row0, row0 + len(x)); x, y float64 vectors of that range."""
    n, k = _graph_tables(index, rev_ptr, rev_edge, eps=(eps, torch.float64), mutual=(mutual, torch.uint8),
                         wsym=(wsym, torch.float32))
    _table(dis, "dis", (n,), torch.float64)
    L.require_cuda(x, "x", torch.float64)
    if x.dim() != 1 or not x.is_contiguous():
        raise L.HipExtensionError("x must be a contiguous vector, got %s" % (tuple(x.shape),))
    nrows = x.shape[0]
    if y is None:
        y = torch.empty_like(x)
    _table(y, "y", (nrows,), torch.float64)
    if y.data_ptr() == x.data_ptr():
        raise L.HipExtensionError("y may not alias x")
    L.call("mi_spectral_spmv", index, wsym, eps, mutual, rev_ptr, rev_edge, n, k, dis, x, y, int(row0), nrows)
    return y


def _sp_basis(Q, w, c):
    L.require_cuda(Q, "Q", torch.float64)
    if Q.dim() != 2 or Q.stride(1) != 1 or Q.shape[0] < 1 or (Q.shape[0] > 1 and Q.stride(0) < Q.shape[1]):
        raise L.HipExtensionError("Q must be (m, n) float64 with contiguous rows, got %s" % (tuple(Q.shape),))
    m, n = Q.shape
    _table(w, "w", (n,), torch.float64)
    if c is None:
        c = torch.empty(m, dtype=torch.float64, device=Q.device)
    _table(c, "c", (m,), torch.float64)
    return m, n, (Q.stride(0) if m > 1 else n), c


def _sp_ws(m, n, device):
    nbytes = L.lib().mi_spectral_workspace_bytes(m, n)
    if nbytes == 0:
        L.check(-3, "mi_spectral_workspace_bytes(m=%d, n=%d)" % (m, n))
    return L.workspace(nbytes, device, "spectral")


def spectral_dots(Q, w, c=None):
    """c = Q^T w (m,) float64 for the m rows of Q (m, n); a fixed summation order (a norm: Q = w[None])."""
    m, n, ldq, c = _sp_basis(Q, w, c)
    ws = _sp_ws(m, n, Q.device)
    L.call("mi_spectral_dots", Q, ldq, m, n, w, c, ws, ws.numel())
    return c


def spectral_orth(Q, w, c=None):
    """c = Q^T w, then w -= Q c in place (one Gram-Schmidt pass against the rows of Q; two passes are `twice is enough`)."""
    m, n, ldq, c = _sp_basis(Q, w, c)
    ws = _sp_ws(m, n, Q.device)
    L.call("mi_spectral_orth", Q, ldq, m, n, w, c, ws, ws.numel())
    return c


def spectral_combine(Q, c, w, beta=0.0):
    """w = beta w - Q c in place (beta = 0: w is only written), the rows of Q taken in order."""
    m, n, ldq, c = _sp_basis(Q, w, c)
    L.call("mi_spectral_combine", Q, ldq, m, n, c, w, float(beta))
    return w


# ---- optimal matching of picks to target centres (csrc/match.hip) -----------------------------------------------------------

MATCH_MAX_POINTS = 4096      # picks and targets per image (mi_match_coordinates refuses more)


def match_coordinates(preds, targets, pred_off, targ_off, radius):
    """One launch for a whole split: preds (sumP, 3) and targets (sumT, 3) float64 on the device, image i owning the rows
    [pred_off[i], pred_off[i + 1]) and [targ_off[i], targ_off[i + 1]) (host sequences of n_img + 1 ascending ints).
    Returns (pred_to_target (sumP,) int32: the matched target's index inside its image or -1, dist (sumP,) float64: the matched
    pair's distance, 0 where unmatched, total_cost (n_img,) float64) of the minimum-cost assignment under
    cost = min(d2 - radius ** 3, 0), the reference's cube.  Raises beyond MATCH_MAX_POINTS picks or targets per image."""
    import numpy as np
    po = np.ascontiguousarray(np.asarray(pred_off, dtype=np.int64))
    to = np.ascontiguousarray(np.asarray(targ_off, dtype=np.int64))
    if po.ndim != 1 or to.ndim != 1 or len(po) != len(to) or len(po) < 1:
        raise L.HipExtensionError("pred_off and targ_off must be two sequences of n_img + 1 offsets")
    n_img = len(po) - 1
    if po[0] != 0 or to[0] != 0 or (np.diff(po) < 0).any() or (np.diff(to) < 0).any() or max(po[-1], to[-1]) >= 2 ** 31:
        raise L.HipExtensionError("offsets must start at 0, ascend and fit an int")
    for t, name, n in ((preds, "preds", int(po[-1])), (targets, "targets", int(to[-1]))):
        L.require_cuda(t, name, torch.float64)
        if t.dim() != 2 or tuple(t.shape) != (n, 3) or not t.is_contiguous():
            raise L.HipExtensionError("%s must be a contiguous (%d, 3) tensor, got %s" % (name, n, tuple(t.shape)))
    dev = preds.device
    p2t = torch.empty(int(po[-1]), dtype=torch.int32, device=dev)
    dist = torch.empty(int(po[-1]), dtype=torch.float64, device=dev)
    total = torch.empty(n_img, dtype=torch.float64, device=dev)
    if n_img == 0:
        return p2t, dist, total
    max_p, max_t = int(np.diff(po).max()), int(np.diff(to).max())
    what = "mi_match_coordinates(%d images, at most %d picks x %d targets)" % (n_img, max_p, max_t)
    nbytes = L.lib().mi_match_workspace_bytes(n_img, max_p, max_t)
    if nbytes == 0:
        L.check(-3, what + ": more than %d picks or targets in one image" % MATCH_MAX_POINTS)
    ws = L.workspace(nbytes, dev, "match")
    po32, to32 = po.astype(np.int32), to.astype(np.int32)
    L.call("mi_match_coordinates", preds, targets, po32.ctypes.data_as(ctypes.c_void_p), to32.ctypes.data_as(ctypes.c_void_p), n_img,
           float(radius), p2t, dist, total, ws, ws.numel())
    return p2t, dist, total


# ---- grouping and tracing the picks, --spike / --fiber (csrc/pick_groups.hip) --------------------------------------------------

PICK_MAX_POINTS = 4096       # points per call (mi_pick_components and mi_pick_fiber_fit refuse more)


def _pick_points(pts, what):
    """The checks both entries share; the size limit comes first and needs no device."""
    if not isinstance(pts, torch.Tensor) or pts.dim() != 2 or pts.shape[1] != 3:
        raise L.HipExtensionError("%s: pts must be an (n, 3) tensor" % what)
    n = int(pts.shape[0])
    if n > PICK_MAX_POINTS or L.lib().mi_pick_workspace_bytes(n) == 0:
        L.check(-3, "%s(%d points): more than %d points in one call" % (what, n, PICK_MAX_POINTS))
    L.require_cuda(pts, "pts", torch.float64)
    if not pts.is_contiguous():
        raise L.HipExtensionError("%s: pts must be contiguous" % what)
    return n


def pick_components(pts, cutoff):
    """Connected components of the graph that joins the rows i, j of pts (n, 3) float64 (device) where sqrt(d2) <= cutoff, d2 summed
    as numpy sums it.  Returns (label (n,) int32: the smallest index of the row's component, size (n,) int32: its member count),
    on the device.  Raises beyond PICK_MAX_POINTS rows."""
    n = _pick_points(pts, "mi_pick_components")
    label = torch.empty(n, dtype=torch.int32, device=pts.device)
    size = torch.empty(n, dtype=torch.int32, device=pts.device)
    if n == 0:
        return label, size
    ws = L.workspace(L.lib().mi_pick_workspace_bytes(n), pts.device, "pick")
    L.call("mi_pick_components", pts, n, float(cutoff), label, size, ws, ws.numel())
    return label, size


def pick_fiber_fit(pts, label, size, res_cutoff, curvature_cutoff, scale, cap_rows):
    """The quadratic fits u(t), v(t) (t, u, v = columns 0, 1, 2 of pts) of every component of more than 6 members and the resampled
    rows of the accepted ones (include/cetpick_hip.h has the rules).  label, size as pick_components returned them for the same pts.
    Returns (comp (n // 7, 16) float64: one record per such component in ascending label order, the rest zero; rows (cap_rows, 3)
    int32 [int(y), int(v_fit), int(u_fit)]; n_rows (1,) int32), on the device.  Raises where the rows do not fit cap_rows."""
    n = _pick_points(pts, "mi_pick_fiber_fit")
    for t, name in ((label, "label"), (size, "size")):
        L.require_cuda(t, name, torch.int32)
        if tuple(t.shape) != (n,) or not t.is_contiguous():
            raise L.HipExtensionError("%s must be a contiguous (%d,) tensor, got %s" % (name, n, tuple(t.shape)))
    cap_rows = int(cap_rows)
    if cap_rows < 0 or cap_rows >= 2 ** 31 // 3:
        raise L.HipExtensionError("cap_rows must be in [0, 2^31 / 3), got %d" % cap_rows)
    dev = pts.device
    comp = torch.zeros(n // 7, 16, dtype=torch.float64, device=dev)
    rows = torch.empty(cap_rows, 3, dtype=torch.int32, device=dev)
    n_rows = torch.zeros(1, dtype=torch.int32, device=dev)
    if n == 0:
        return comp, rows, n_rows
    ws = L.workspace(L.lib().mi_pick_workspace_bytes(n), dev, "pick")
    L.call("mi_pick_fiber_fit", pts, n, label, size, float(res_cutoff), float(curvature_cutoff), float(scale), comp, rows, cap_rows,
           n_rows, ws, ws.numel())
    return comp, rows, n_rows


# ---- the class gallery of plot_2d --class_gallery (csrc/class_gallery.hip) -------------------------------------

GALLERY_MAX_EXEMPLARS = 64   # m of gallery_exemplars (the running best sits in LDS)
GALLERY_MAX_CLASSES = 4096
GALLERY_MAX_PICKS = 1 << 24
GALLERY_PAD, GALLERY_TEXT_W, GALLERY_TEXT_H = 4, 94, 32          # the fixed sizes of the picture, in pixels


def _gallery_tensor(t, name, dtype, shape):
    """A refusal of this kind is the caller's mistake and needs no device: ValueError."""
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a tensor, got %s" % (name, type(t).__name__))
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if len(shape) != t.dim() or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError("%s must be %s, got %s" % (name, tuple("*" if s is None else s for s in shape), tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _gallery_range(t, name, hi):
    """Every element of the int32 tensor t in [0, hi): looked at on a host copy, so that no kernel starts for a bad input."""
    v = t.detach().cpu().numpy()
    if v.size and (int(v.min()) < 0 or int(v.max()) >= hi):
        bad = int(v.min()) if int(v.min()) < 0 else int(v.max())
        raise ValueError("%s holds %d, outside [0, %d)" % (name, bad, hi))


def _gallery_sizes(n, k_classes, m=1):
    if n == 0:
        raise ValueError("the class gallery needs at least one pick (n == 0)")
    if n > GALLERY_MAX_PICKS:
        raise ValueError("at most %d picks, got %d" % (GALLERY_MAX_PICKS, n))
    if not 1 <= int(k_classes) <= GALLERY_MAX_CLASSES:
        raise ValueError("k_classes must be in 1..%d, got %d" % (GALLERY_MAX_CLASSES, k_classes))
    if not 1 <= int(m) <= GALLERY_MAX_EXEMPLARS:
        raise ValueError("m must be in 1..%d, got %d" % (GALLERY_MAX_EXEMPLARS, m))


def gallery_moments(patches, labels, k_classes):
    """Per class of labels (n,) int32 in [0, k_classes): (mean (k, h, w) fp32, std (k, h, w) fp32, count (k,) int32) of the patches
    (n, h, w) fp32 - the per-pixel mean and population deviation in float64, two passes, members in ascending pick index.  A class
    without members has count 0 and zeros.  The same input gives the same bytes.  Raises ValueError for a label outside the range,
    a non-contiguous input and n == 0, before any launch."""
    patches = _gallery_tensor(patches, "patches", torch.float32, (None, None, None))
    n, h, w = (int(s) for s in patches.shape)
    labels = _gallery_tensor(labels, "labels", torch.int32, (n,))
    k = int(k_classes)
    _gallery_sizes(n, k)
    if h * w == 0 or h * w > 1 << 20:
        raise ValueError("a patch has 1..2^20 pixels, got %d x %d" % (h, w))
    _gallery_range(labels, "labels", k)
    L.require_cuda(patches, "patches")
    L.require_cuda(labels, "labels", torch.int32)
    dev = patches.device
    mean = torch.empty((k, h, w), dtype=torch.float32, device=dev)
    std = torch.empty((k, h, w), dtype=torch.float32, device=dev)
    count = torch.empty((k,), dtype=torch.int32, device=dev)
    ws = L.workspace(L.lib().mi_gallery_workspace_bytes(n, k, h * w, 1), dev, "gallery")
    L.call("mi_gallery_moments", patches, labels, n, h, w, k, mean, std, count, ws, ws.numel())
    return mean, std, count


def gallery_exemplars(emb, centroids, assign, labels, k_classes, m):
    """Per class the m members nearest to the centroid they are assigned to: (idx (k, m) int32, d2 (k, m) float64), ascending by
    (d2, pick index), padded with -1 and +inf.  emb (n, dim) fp32, centroids (k_centroids, dim) fp32, assign (n,) int32 in
    [0, k_centroids), labels (n,) int32 in [0, k_classes); d2 = sum_j (emb - centroid)^2 in float64, j ascending.  Raises
    ValueError for m outside 1..64, a label or an assignment outside its range, a non-contiguous input and n == 0, before any
    launch."""
    emb = _gallery_tensor(emb, "emb", torch.float32, (None, None))
    n, dim = (int(s) for s in emb.shape)
    centroids = _gallery_tensor(centroids, "centroids", torch.float32, (None, dim))
    assign = _gallery_tensor(assign, "assign", torch.int32, (n,))
    labels = _gallery_tensor(labels, "labels", torch.int32, (n,))
    k, kc, m = int(k_classes), int(centroids.shape[0]), int(m)
    _gallery_sizes(n, k, m)
    if dim == 0 or dim > 65536 or kc == 0:
        raise ValueError("emb (n, dim) and centroids (k_centroids, dim) need 1 <= dim <= 65536 and a centroid")
    _gallery_range(labels, "labels", k)
    _gallery_range(assign, "assign", kc)
    for t, name in ((emb, "emb"), (centroids, "centroids")):
        L.require_cuda(t, name)
    for t, name in ((assign, "assign"), (labels, "labels")):
        L.require_cuda(t, name, torch.int32)
    dev = emb.device
    idx = torch.empty((k, m), dtype=torch.int32, device=dev)
    d2 = torch.empty((k, m), dtype=torch.float64, device=dev)
    ws = L.workspace(L.lib().mi_gallery_workspace_bytes(n, k, 0, m), dev, "gallery")
    L.call("mi_gallery_exemplars", emb, centroids, assign, labels, n, dim, kc, k, m, idx, d2, ws, ws.numel())
    return idx, d2


def gallery_canvas(k_classes, h, w, m_show, scale):
    """(H, W) of the picture gallery_raster draws (include/cetpick_hip.h has the layout)."""
    row = max(h * scale, GALLERY_TEXT_H)
    return (GALLERY_PAD + k_classes * (row + GALLERY_PAD),
            2 * GALLERY_PAD + GALLERY_TEXT_W + (2 + m_show) * (w * scale + GALLERY_PAD))


def gallery_raster(mean, std, count, idx, patches, glyphs, m_show=None, scale=2):
    """The picture of the gallery: (rgb (H, W, 3) uint8, order (k,) int32 - the class of every row: descending count, ascending
    class among equal counts), both on the device.  mean, std (k, h, w) fp32 and count (k,) int32 as gallery_moments returns them,
    idx (k, m) int32 as gallery_exemplars does, patches (n, h, w) fp32, glyphs (10, 7) uint8 (utils/plot2d.DIGITS_5X7).  The first
    m_show (default: all m) exemplars are drawn, every patch enlarged `scale` times."""
    mean = _gallery_tensor(mean, "mean", torch.float32, (None, None, None))
    k, h, w = (int(s) for s in mean.shape)
    std = _gallery_tensor(std, "std", torch.float32, (k, h, w))
    count = _gallery_tensor(count, "count", torch.int32, (k,))
    idx = _gallery_tensor(idx, "idx", torch.int32, (k, None))
    patches = _gallery_tensor(patches, "patches", torch.float32, (None, h, w))
    glyphs = _gallery_tensor(glyphs, "glyphs", torch.uint8, (10, 7))
    n, m = int(patches.shape[0]), int(idx.shape[1])
    m_show = m if m_show is None else int(m_show)
    scale = int(scale)
    _gallery_sizes(n, k, m)
    if not 0 <= m_show <= m or not 1 <= scale <= 64 or h * w == 0 or h * w > 1 << 20 or max(h, w) * scale > 65536:
        raise ValueError("m_show must be in 0..%d and scale in 1..64 (patches of at most 2^20 pixels, 65536 enlarged), got %d and %d"
                         % (m, m_show, scale))
    H_, W_ = gallery_canvas(k, h, w, m_show, scale)
    if H_ * W_ > 0x3fffffff:
        raise ValueError("a picture of %d x %d pixels is too large" % (H_, W_))
    for t, name, dt in ((mean, "mean", torch.float32), (std, "std", torch.float32), (count, "count", torch.int32),
                        (idx, "idx", torch.int32), (patches, "patches", torch.float32), (glyphs, "glyphs", torch.uint8)):
        L.require_cuda(t, name, dt)
    dev = mean.device
    rgb = torch.empty((H_, W_, 3), dtype=torch.uint8, device=dev)
    order = torch.empty((k,), dtype=torch.int32, device=dev)
    ws = L.workspace(L.lib().mi_gallery_raster_workspace_bytes(k, m_show), dev, "gallery_raster")
    L.call("mi_gallery_raster", mean, std, count, idx, patches, n, h, w, k, m, m_show, scale, glyphs, order, rgb, H_, W_, ws,
           ws.numel())
    return rgb, order


# ---- the SCAN loss over all heads and the class assignment (csrc/scan_loss.hip) -----------------------------

SCAN_CHUNK = 256             # MI_SCAN_CHUNK: rows per partial sum of mi_scan_loss_fwd
SCAN_MAX_CLASSES, SCAN_MAX_HEADS, SCAN_MAX_ROWS = 64, 16, 65536


def _scan_logits(t, name, nheads, max_rows=None):
    """(rows, classes per head) of the logits t (rows, nheads C) fp32, after every check the kernels rely on: ValueError before any
    launch for a wrong rank, dtype, layout, head or class count, or no rows."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError("%s must be a (rows, nheads x nclusters) tensor" % name)
    if t.dtype != torch.float32:
        raise ValueError("%s must be torch.float32, got %s" % (name, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    nheads = int(nheads)
    if not 1 <= nheads <= SCAN_MAX_HEADS:
        raise ValueError("nheads must be in 1..%d, got %d" % (SCAN_MAX_HEADS, nheads))
    rows, width = (int(s) for s in t.shape)
    if width == 0 or width % nheads or width // nheads > SCAN_MAX_CLASSES:
        raise ValueError("%s has %d columns: %d heads need the same 1..%d classes each" % (name, width, nheads, SCAN_MAX_CLASSES))
    if rows == 0 or (max_rows is not None and rows > max_rows):
        raise ValueError("%s must have 1..%s rows, got %d" % (name, max_rows if max_rows is not None else "any", rows))
    return rows, width // nheads


def _scan_logits_pair(first, second, names, differ, nheads):
    """(rows, classes per head) of the two logits tensors of one training batch: the same shape (else ValueError(differ % both
    shapes)), each through _scan_logits, both on the device."""
    b, c = _scan_logits(first, names[0], nheads, SCAN_MAX_ROWS)
    if second.shape != first.shape:
        raise ValueError(differ % (tuple(first.shape), tuple(second.shape)))
    _scan_logits(second, names[1], nheads, SCAN_MAX_ROWS)
    L.require_cuda(first, names[0])
    L.require_cuda(second, names[1])
    return b, c


class _ScanLossFn(torch.autograd.Function):
    """mi_scan_loss_fwd / _bwd: (sum of the heads' totals, stats (H, 3) = total, consistency, entropy per head)."""

    @staticmethod
    def forward(ctx, anchors, neighbours, nheads, entropy_weight):
        b, c = _scan_logits_pair(anchors, neighbours, ("anchors", "neighbours"), "anchors are %s, neighbours %s", nheads)
        h, dev = int(nheads), anchors.device
        ws = L.workspace(L.lib().mi_scan_loss_workspace_bytes(b, c, h), dev, "scanloss")
        stats = torch.empty((h, 3), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        mean = torch.empty((h, c), dtype=torch.float64, device=dev)
        L.call("mi_scan_loss_fwd", anchors, neighbours, b, c, h, float(entropy_weight), stats, loss, mean, ws, ws.numel())
        ctx.save_for_backward(anchors, neighbours, mean)
        ctx.dims, ctx.entropy_weight = (b, c, h), float(entropy_weight)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        anchors, neighbours, mean = ctx.saved_tensors
        b, c, h = ctx.dims
        dl = dloss.contiguous().float()                    # read on the device: no host sync
        da, db = torch.empty_like(anchors), torch.empty_like(neighbours)
        L.call("mi_scan_loss_bwd", anchors, neighbours, b, c, h, ctx.entropy_weight, mean, dl, da, db)
        return da, db, None, None


def scan_loss(anchors, neighbours, nheads=1, entropy_weight=2.0):
    """The SCAN loss of every head at once: anchors, neighbours (B, nheads C) fp32 logits, contiguous, head h in columns
    h C .. h C + C - 1, 1 <= C <= 64, nheads <= 16, B <= 65536.  -> (loss (): the sum over the heads of total_h, differentiable with
    respect to both logits tensors; stats (nheads, 3): total, consistency, entropy of every head, no gradient).  The same input
    gives the same bytes, forward and backward.  ValueError, before any launch, outside the limits or for non-contiguous logits."""
    return _ScanLossFn.apply(anchors, neighbours, int(nheads), float(entropy_weight))


def scan_assign(logits, nheads=1, with_prob=False):
    """Per row and head of logits (N, nheads C) fp32, any N >= 1: (label (N, nheads) int32, the argmax with the lowest index on an
    exact tie; conf (N, nheads) fp32, its softmax probability; counts (nheads, C) int32, the rows per class; prob (N, nheads C) fp32
    with with_prob, else None)."""
    n, c = _scan_logits(logits, "logits", nheads)
    L.require_cuda(logits, "logits")
    h, dev = int(nheads), logits.device
    label = torch.empty((n, h), dtype=torch.int32, device=dev)
    conf = torch.empty((n, h), dtype=torch.float32, device=dev)
    counts = torch.empty((h, c), dtype=torch.int32, device=dev)
    prob = torch.empty((n, h * c), dtype=torch.float32, device=dev) if with_prob else None
    L.call("mi_scan_assign", logits.detach(), n, c, h, label, conf, prob, counts)
    return label, conf, counts, prob


# ---- the heads scored over the whole graph, and the self-labelling loss (csrc/scan_selflabel.hip) ------------

SCAN_MAX_NEIGHBOURS = 64


def scan_graph_eval(logits, index, nheads=1, with_self=True, validate=True):
    """The reference's scan_evaluate on the device: logits (N, nheads C) fp32 of every pick, index (N, k) int32 graph neighbours,
    1 <= k <= 64, entries in 0..N-1; with_self adds the pick itself in front of its row ([self, neighbour 1..k]: the table
    utils/scan.draw_neighbours draws from).  -> (stats (nheads, 3) fp32: total = consistency - entropy, consistency over every
    (pick, entry) pair, entropy of the mean distribution; best (1,) int32: the head with the lowest total, the lowest index on an
    exact tie).  The kernel does not check the table: `validate` does here, with one host read (a caller that has checked passes
    False)."""
    n, c = _scan_logits(logits, "logits", nheads)
    L.require_cuda(logits, "logits")
    L.require_cuda(index, "index", torch.int32)
    if index.dim() != 2 or index.shape[0] != n or not index.is_contiguous():
        raise ValueError("index must be a contiguous (%d, k) tensor, got %s" % (n, tuple(index.shape)))
    k = int(index.shape[1])
    if not 1 <= k <= SCAN_MAX_NEIGHBOURS:
        raise ValueError("index must have 1..%d columns, got %d" % (SCAN_MAX_NEIGHBOURS, k))
    if validate:
        lo, hi = (int(v) for v in torch.aminmax(index))
        if lo < 0 or hi >= n:
            raise ValueError("the graph names a pick outside 0..%d" % (n - 1))
    h, dev = int(nheads), logits.device
    ws = L.workspace(L.lib().mi_scan_graph_eval_workspace_bytes(n, c, h), dev, "scangraph")
    stats = torch.empty((h, 3), dtype=torch.float32, device=dev)
    best = torch.empty((1,), dtype=torch.int32, device=dev)
    L.call("mi_scan_graph_eval", logits.detach(), n, c, h, index, k, int(bool(with_self)), stats, best, ws, ws.numel())
    return stats, best


class _ScanSelflabelFn(torch.autograd.Function):
    """mi_scan_selflabel_fwd / _bwd: (loss, info (3,), count (C,), target (B,), mask (B,)); the gradient goes to `strong` alone."""

    @staticmethod
    def forward(ctx, weak, strong, threshold, balance):
        b, c = _scan_logits_pair(weak, strong, ("weak", "strong"), "weak is %s, strong %s", 1)
        dev = strong.device
        ws = L.workspace(L.lib().mi_scan_selflabel_workspace_bytes(b, c), dev, "scanselflabel")
        loss = torch.empty((), dtype=torch.float32, device=dev)
        info = torch.empty((3,), dtype=torch.int32, device=dev)
        count = torch.empty((c,), dtype=torch.int32, device=dev)
        target = torch.empty((b,), dtype=torch.int32, device=dev)
        mask = torch.empty((b,), dtype=torch.uint8, device=dev)
        denom = torch.empty((), dtype=torch.float64, device=dev)
        L.call("mi_scan_selflabel_fwd", weak, strong, b, c, float(threshold), int(bool(balance)), loss, info, count, target, mask,
               denom, ws, ws.numel())
        ctx.save_for_backward(strong, info, count, target, mask, denom)
        ctx.dims, ctx.balance = (b, c), int(bool(balance))
        ctx.mark_non_differentiable(info, count, target, mask)
        return loss, info, count, target, mask

    @staticmethod
    def backward(ctx, dloss, *_):
        strong, info, count, target, mask, denom = ctx.saved_tensors
        b, c = ctx.dims
        dl = dloss.contiguous().float()                    # read on the device: no host sync
        ds = torch.empty_like(strong)
        L.call("mi_scan_selflabel_bwd", strong, b, c, ctx.balance, info, count, target, mask, denom, dl, ds)
        return None, ds, None, None


def scan_selflabel(weak, strong, threshold, balance=True):
    """scan_selflabel_loss with the rows' targets and mask as well: -> (loss, info, count, target (B,) int32, mask (B,) uint8)."""
    return _ScanSelflabelFn.apply(weak.detach(), strong, float(threshold), bool(balance))


def scan_selflabel_loss(weak, strong, threshold, balance=True):
    """SCAN's self-labelling loss of one head (the reference's ConfidenceBasedCE): weak, strong (B, C) fp32 logits, contiguous,
    1 <= C <= 64, B <= 65536.  A row whose largest softmax(weak) probability exceeds `threshold` is confident; its target is that
    class; the loss is the cross-entropy of softmax(strong) against the targets over the confident rows, each weighted - with
    `balance` - by the inverse share of its class among them, divided by the sum of the weights.
    -> (loss (), differentiable with respect to `strong` only; info (3,) int32 = confident rows, classes present, B; count (C,)
    int32 = confident rows per class).  No confident row: loss 0 and a zero gradient, nothing raised (the module
    models.loss.ConfidenceBasedCE raises as the reference does).  The same input gives the same bytes, forward and backward."""
    return scan_selflabel(weak, strong, threshold, balance)[:3]


# ---- how good a clustering is: exact silhouette and contingency table (csrc/cluster_quality.hip) -------------

SILHOUETTE_MAX_K = 1024                   # fine clusters of silhouette_sums, classes of silhouette_finalise


def _quality_labels(t, name, n, device, hi, validate):
    """labels (n,) int32, contiguous, on `device`; with `validate` their range [0, hi) is checked on the device (one host read)."""
    L.require_cuda(t, name, torch.int32)
    if t.dim() != 1 or t.shape[0] != n or not t.is_contiguous() or t.device != device:
        raise L.HipExtensionError("%s must be a contiguous (%d,) int32 tensor on %s, got %s on %s"
                                  % (name, n, device, tuple(t.shape), t.device))
    if validate and n:
        lo, top = (int(v) for v in torch.aminmax(t))
        if lo < 0 or top >= hi:
            raise ValueError("%s holds %d, outside 0..%d" % (name, lo if lo < 0 else top, hi - 1))
    return t


def silhouette_sums(x, labels, k, validate=True):
    """sums (N, k) float64 on the device: sums[i][c] = the sum over the members j != i of fine cluster c of |x_i - x_j|, the
    squared distance formed as knn_search's "l2" value (bf16x3 on the matrix cores), its square root and the sums in float64; the
    N x N distances are never stored.  x (N, d) fp32 contiguous, labels (N,) int32 in [0, k), k <= 1024.  `validate` checks the
    labels' range here, with one host read: a label outside it is a ValueError that names it (the kernel would leave such a pick
    out).  The same input gives the same bytes."""
    x = _km_x(x)
    n, d = x.shape
    k = int(k)
    labels = _quality_labels(labels, "labels", n, x.device, k, validate)
    what = "(N=%d, d=%d, k=%d)" % (n, d, k)
    nbytes = L.lib().mi_silhouette_workspace_bytes(n, d, k)
    if nbytes == 0:
        L.check(-3, "mi_silhouette_workspace_bytes" + what)
    order = torch.sort(labels, stable=True)[1].to(torch.int32)          # plumbing: picks by label, ascending index within one
    sums = torch.empty((n, k), dtype=torch.float64, device=x.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    L.call("mi_silhouette_sums", x, labels, order, n, d, k, sums, ws, ws.numel())
    return sums


def silhouette_finalise(sums, labels, class_of=None):
    """The silhouette of every pick from silhouette_sums' table: sums (N, k) float64, labels (N,) int32 fine labels in [0, k),
    class_of (k,) int32 -> [0, C) the class of every fine cluster (None: the identity, C = k).  -> dict of device tensors: s, a,
    b (N,) float64 (a: mean distance to the own class, b: to the nearest other non-empty class, s = (b - a) / max(a, b); a = s =
    0 for the only member of a class), nearest (N,) int32 (the class attaining b, the lowest on a tie), class_mean (C,) float64
    (NaN for a class without members), class_count (C,) int32, mean () float64, confusion (C, C) int32 [own][nearest].  Fewer than
    two non-empty classes, or no class with two members, is a ValueError (sklearn raises there too); this reads three integers
    from the device."""
    L.require_cuda(sums, "sums", torch.float64)
    if sums.dim() != 2 or not sums.is_contiguous():
        raise L.HipExtensionError("sums must be a contiguous (N, k) float64 tensor, got %s" % (tuple(sums.shape),))
    n, k = sums.shape
    dev = sums.device
    labels = _quality_labels(labels, "labels", n, dev, k, True)
    if class_of is None:
        class_of, c = torch.arange(k, dtype=torch.int32, device=dev), k
    else:
        class_of = _quality_labels(class_of, "class_of", k, dev, SILHOUETTE_MAX_K, True)
        c = int(class_of.max()) + 1
    if c < 2:
        raise ValueError("the silhouette needs at least 2 classes, got %d" % c)
    nbytes = L.lib().mi_silhouette_finalise_workspace_bytes(n, k, c)
    if nbytes == 0:
        L.check(-3, "mi_silhouette_finalise_workspace_bytes(N=%d, k=%d, C=%d)" % (n, k, c))
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    out = dict(s=torch.empty(n, **f64), a=torch.empty(n, **f64), b=torch.empty(n, **f64), nearest=torch.empty(n, **i32),
               class_mean=torch.empty(c, **f64), class_count=torch.empty(c, **i32), mean=torch.empty((), **f64),
               confusion=torch.empty((c, c), **i32))
    info = torch.empty(3, **i32)
    ws = L.workspace(nbytes, dev, "silhouette")
    L.call("mi_silhouette_finalise", sums, labels, class_of, n, k, c, out["s"], out["a"], out["b"], out["nearest"],
           out["class_mean"], out["class_count"], out["mean"], out["confusion"], info, ws, ws.numel())
    nonempty, largest, status = (int(v) for v in info.cpu())
    if status:
        raise ValueError("the silhouette needs 2 classes with members and one class with 2 members: %d classes have members, the "
                         "largest has %d" % (nonempty, largest))
    return out


def label_contingency(a, b, ca, cb):
    """table (ca, cb) int64 on the device: the picks with labels (a_i, b_i); a, b (N,) int32 in [0, ca) and [0, cb)."""
    L.require_cuda(a, "a", torch.int32)
    n, ca, cb = a.shape[0] if a.dim() == 1 else -1, int(ca), int(cb)
    if n < 1 or not isinstance(b, torch.Tensor) or tuple(b.shape) != (n,):
        raise ValueError("a and b must be (N,) label arrays of one length, N >= 1, got %s and %s"
                         % (tuple(a.shape), tuple(getattr(b, "shape", ()))))
    a = _quality_labels(a, "a", n, a.device, ca, True)
    b = _quality_labels(b, "b", n, a.device, cb, True)
    table = torch.empty((ca, cb), dtype=torch.int64, device=a.device)
    L.call("mi_label_contingency", a, b, n, ca, cb, table)
    return table


# ---- label spreading over the neighbour graph and the seed matching (csrc/label_spread.hip) ------------------

SPREAD_MAX_C = 64                         # classes of spread_step and spread_decide, 2 at least


def _spread_table(t, name, shape, dtype, device=None):
    L.require_cuda(t, name, dtype)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous() or (device is not None and t.device != device):
        raise L.HipExtensionError("%s must be a contiguous %s %s tensor%s, got %s on %s"
                                  % (name, tuple(shape), dtype, "" if device is None else " on %s" % device, tuple(t.shape), t.device))
    return t


def spread_weights(index, dist=None, mode=1):
    """w (N, K) fp32 on the device, the weight of every forward edge of index (N, K) int32: mode 0 is 1 per valid edge, mode 1 the
    self-tuning Gaussian exp(-d2 / sqrt(s_i s_j)) of dist (N, K) fp32 squared L2, s_i the largest finite dist of row i; 0 for an edge
    that points at its own row or outside [0, N).  -> (w, scale (N,) fp32 or None)."""
    L.require_cuda(index, "index", torch.int32)
    if index.dim() != 2 or not index.is_contiguous():
        raise L.HipExtensionError("index must be a contiguous (N, K) int32 tensor, got %s" % (tuple(index.shape),))
    n, k = index.shape
    mode = int(mode)
    scale = None
    if mode == 1:
        if dist is None:
            raise ValueError("the Gaussian edge weight needs the graph's distances")
        _spread_table(dist, "dist", (n, k), torch.float32, index.device)
        scale = torch.empty(n, dtype=torch.float32, device=index.device)
    w = torch.empty((n, k), dtype=torch.float32, device=index.device)
    L.call("mi_spread_weights", index, dist if mode == 1 else None, n, k, mode, scale, w)
    return w, scale


def spread_csr(index, rev_ptr, rev_edge, w):
    """The symmetric, degree-normalised graph of label spreading in CSR form, on the device: row i lists its valid forward edges
    in column order, then the edges that end in i and have no opposite edge; val = w_sym / sqrt(deg_i deg_j), w_sym = max(w_ij,
    w_ji).  index (N, K) int32, (rev_ptr, rev_edge) = utils.graph.reverse_graph(index) on the device, w (N, K) fp32.
    -> row_ptr (N + 1,) int64, col (nnz,) int32, val (nnz,) float64, deg (N,) float64.  One host read (nnz).  The same input gives
    the same bytes."""
    L.require_cuda(index, "index", torch.int32)
    if index.dim() != 2 or not index.is_contiguous():
        raise L.HipExtensionError("index must be a contiguous (N, K) int32 tensor, got %s" % (tuple(index.shape),))
    n, k = index.shape
    dev = index.device
    _spread_table(rev_ptr, "rev_ptr", (n + 1,), torch.int32, dev)
    _spread_table(rev_edge, "rev_edge", (n * k,), torch.int32, dev)
    _spread_table(w, "w", (n, k), torch.float32, dev)
    count = torch.empty(n, dtype=torch.int64, device=dev)
    deg = torch.empty(n, dtype=torch.float64, device=dev)
    L.call("mi_spread_csr_count", index, rev_ptr, rev_edge, w, n, k, count, deg)
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    row_ptr[1:] = torch.cumsum(count, 0)                                 # plumbing: the exclusive scan
    nnz = int(row_ptr[-1])
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float64, device=dev)
    if nnz:
        L.call("mi_spread_csr_fill", index, rev_ptr, rev_edge, w, n, k, row_ptr, deg, nnz, col, val)
    return row_ptr, col, val, deg


def spread_step(row_ptr, col, val, alpha, f_in, y, f_out, residual=None):
    """One sweep of label spreading: f_out[i] = alpha sum_e val_e f_in[col_e] + (1 - alpha) y[i].  f_in, y, f_out (N, C) float64,
    2 <= C <= 64, f_out another buffer than f_in and y.  residual: a (1,) int64 device tensor that receives the bits of the
    float64 max |f_out - f_in| (read it with .view(torch.float64)); None skips that."""
    L.require_cuda(f_in, "f_in", torch.float64)
    if f_in.dim() != 2 or not f_in.is_contiguous():
        raise L.HipExtensionError("f_in must be a contiguous (N, C) float64 tensor, got %s" % (tuple(f_in.shape),))
    n, c = f_in.shape
    dev = f_in.device
    _spread_table(y, "y", (n, c), torch.float64, dev)
    _spread_table(f_out, "f_out", (n, c), torch.float64, dev)
    _spread_table(row_ptr, "row_ptr", (n + 1,), torch.int64, dev)
    nnz = col.shape[0] if isinstance(col, torch.Tensor) and col.dim() == 1 else -1
    _spread_table(col, "col", (nnz,), torch.int32, dev)
    _spread_table(val, "val", (nnz,), torch.float64, dev)
    if residual is not None:
        _spread_table(residual, "residual", (1,), torch.int64, dev)
    L.call("mi_spread_step", row_ptr, col, val, n, c, float(alpha), f_in, y, f_out, residual)
    return f_out


def spread_decide(f, min_conf):
    """label (N,) int32 = argmax_c f[i, c] (ties to the lowest c), -1 where the row's mass is 0 or its confidence below min_conf;
    conf (N,) float64 = f[i, label] / mass; mass (N,) float64 = sum_c f[i, c].  f (N, C) float64, 2 <= C <= 64."""
    L.require_cuda(f, "f", torch.float64)
    if f.dim() != 2 or not f.is_contiguous():
        raise L.HipExtensionError("f must be a contiguous (N, C) float64 tensor, got %s" % (tuple(f.shape),))
    n, c = f.shape
    label = torch.empty(n, dtype=torch.int32, device=f.device)
    conf = torch.empty(n, dtype=torch.float64, device=f.device)
    mass = torch.empty(n, dtype=torch.float64, device=f.device)
    L.call("mi_spread_decide", f, n, c, float(min_conf), label, conf, mass)
    return label, conf, mass


def seed_nearest(picks, pick_tomo, seeds, seed_tomo, radius):
    """For every seed the nearest pick of its tomogram: picks (N, 3), seeds (M, 3) float64, pick_tomo (N,), seed_tomo (M,) int32.
    -> pick (M,) int32 (-1: none within radius), dist (M,) float64 (the least distance, +inf where the tomogram has no pick)."""
    L.require_cuda(picks, "picks", torch.float64)
    L.require_cuda(seeds, "seeds", torch.float64)
    if picks.dim() != 2 or picks.shape[1] != 3 or seeds.dim() != 2 or seeds.shape[1] != 3:
        raise L.HipExtensionError("picks and seeds must be (N, 3) and (M, 3), got %s and %s" % (tuple(picks.shape), tuple(seeds.shape)))
    n, m = picks.shape[0], seeds.shape[0]
    dev = picks.device
    _spread_table(picks, "picks", (n, 3), torch.float64, dev)
    _spread_table(seeds, "seeds", (m, 3), torch.float64, dev)
    _spread_table(pick_tomo, "pick_tomo", (n,), torch.int32, dev)
    _spread_table(seed_tomo, "seed_tomo", (m,), torch.int32, dev)
    pick = torch.empty(m, dtype=torch.int32, device=dev)
    dist = torch.empty(m, dtype=torch.float64, device=dev)
    L.call("mi_seed_nearest", picks, pick_tomo, n, seeds, seed_tomo, m, float(radius), pick, dist)
    return pick, dist
