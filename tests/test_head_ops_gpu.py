"""The small kernels at the end of csrc/train_ops.hip - the contrastive head, the scalar reductions, the flat-arena optimiser
passes and the queue - each against a plain float64 restatement of the same operation, at shapes that are no multiple of a
wave, a workgroup or a float4 and on both sides of every threshold between two code paths.

Numeric results go through conftest.f32_equivalent (the GPU may lie as far from float64 as twice a CPU float32 evaluation of
the same formula does, plus the default floor); copies and selects are compared bit for bit.  No reference calls hipops,
except where a fused form is compared bit for bit with the separate kernels - and those cases carry a float64 check too."""
import functools
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

T = 0.07
EPS32 = float(np.finfo(np.float32).eps)
LONG = 4 * (2048 * 256) + 4 * 300 + 3      # past the 2048-workgroup cap: the grid-stride loop runs twice, the scalar tail is live
LONG4 = LONG - LONG % 4
ERRORS = {}                                # group -> [largest GPU-vs-float64, largest CPU-fp32-vs-float64]


def _H():
    from cet_pick_amd import hipops
    return hipops


def _err():
    from cet_pick_amd._lib import HipExtensionError
    return HipExtensionError


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _eq(group, got, cpu32, ref64, what):
    from conftest import f32_equivalent
    e_g, e_c = f32_equivalent(_np(got), _np(cpu32), _np(ref64), what=what)
    print("%-14s %-44s GPU %.3e  CPU fp32 %.3e" % (group, what, e_g, e_c))
    rec = ERRORS.setdefault(group, [0.0, 0.0])
    rec[0], rec[1] = max(rec[0], e_g), max(rec[1], e_c)
    return e_g, e_c


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for group, (e_g, e_c) in sorted(ERRORS.items()):
        print("\nlargest error, %-14s GPU %.3e  CPU fp32 %.3e" % (group, e_g, e_c))


def _cancelled(got, scale, what):
    """A gradient that is zero in exact arithmetic (a one-element row: normalize(x) = +-1 whatever x is): what is left of
    dy - y (y . dy) is rounding.  y = x * (1 / |x|) carries two fp32 roundings (2u, u = eps/2), it enters squared (4u) and
    the two products round once each (6u = 3 eps): |dx| <= 4 eps |dy| / |x|.  The float64 reference of such an entry is
    itself rounding noise, so no relative comparison means anything here."""
    got, scale = np.abs(_np(got).astype(np.float64)), np.abs(_np(scale).astype(np.float64))
    assert np.all(got <= 4 * EPS32 * scale), (what, got.max(), scale.max())


# ------------------------------------------------------------------------------------------------
# 1. normalise and logits
# ------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(1, 1, 1), (3, 48, 100), (5, 128, 257), (4, 100, 513), (4, 102, 513), (2, 1024, 300)]
L2_SHAPES = sorted({(b, c) for b, c, _ in HEAD_SHAPES}) + [(4099, 32), (4100, 16)]


def _row_scales(b):
    return (10.0 ** torch.linspace(-3.0, 3.0, b)).float()[:, None]


@functools.lru_cache(maxsize=None)
def _head_inputs(b, c, r):
    g = _gen(1000 * b + c + r)
    q = torch.randn(b, c, generator=g) * _row_scales(b)
    k = torch.randn(b, c, generator=g) * _row_scales(b).flip(0)
    queue = F.normalize(torch.randn(c, r, generator=g), dim=0)
    dl = torch.randn(b, r + 1, generator=g)
    return q, k, queue, dl


def _logits_formula(q, k, queue, dl, normalize):
    """(logits, k_hat, d/dq of sum(logits * dl)) by torch in the dtype of the arguments"""
    q = q.clone().requires_grad_(True)
    qn, kn = (F.normalize(q, dim=1), F.normalize(k, dim=1)) if normalize else (q, k)
    logits = torch.cat([(qn * kn).sum(1, keepdim=True), qn @ queue], 1) / T
    torch.autograd.backward(logits, dl)
    return logits.detach(), kn, q.grad


@functools.lru_cache(maxsize=None)
def _head_reference(b, c, r, normalize):
    q, k, queue, dl = _head_inputs(b, c, r)
    if not normalize:
        q, k = F.normalize(q, dim=1), F.normalize(k, dim=1)         # the fp32 rows that all three evaluations start from
    return (q, k, _logits_formula(q, k, queue, dl, normalize),
            _logits_formula(q.double(), k.double(), queue.double(), dl.double(), normalize))


def _dq64(k_hat, queue, dl):
    return (dl[:, :1].double() * k_hat.double() + dl[:, 1:].double() @ queue.double().t()) / T


@pytest.mark.parametrize("b,c", L2_SHAPES)
def test_l2_normalize(b, c):
    H = _H()
    g = _gen(17 * b + c)
    x = torch.randn(b, c, generator=g) * _row_scales(b)
    dy = torch.randn(b, c, generator=g)
    live = torch.ones(b, dtype=torch.bool)
    if b >= 3:
        x[1] = 0.0
        live[1] = False
    ref = {}
    for dt in (torch.float32, torch.float64):
        xr = x.to(dt).clone().requires_grad_(True)
        y = F.normalize(xr, dim=1)
        y.backward(dy.to(dt))
        ref[dt] = (y.detach(), xr.grad)
    xg = x.cuda().requires_grad_(True)
    y = H.l2_normalize(xg)
    y.backward(dy.cuda())
    what = "l2_normalize (%d, %d)" % (b, c)
    _eq("l2_normalize", y, ref[torch.float32][0], ref[torch.float64][0], what + " y")
    dx = xg.grad.cpu()
    if c == 1:
        _cancelled(dx, dy / x.abs(), what + " dx")
    else:
        _eq("l2_normalize", dx[live], ref[torch.float32][1][live], ref[torch.float64][1][live], what + " dx")
    if b >= 3:
        # torch's eps clamp: a zero row stays zero and its gradient is dy / 1e-12
        assert torch.equal(y[1].detach().cpu(), torch.zeros(c))
        np.testing.assert_allclose(_np(ref[torch.float64][1][1]), _np(dy[1].double() * 1e12), rtol=1e-12)
        _eq("l2_normalize", dx[1], ref[torch.float32][1][1], dy[1].double() * 1e12, what + " dx of the zero row")


@pytest.mark.parametrize("b,c,r", HEAD_SHAPES)
def test_moco_logits(b, c, r):
    H = _H()
    _, _, queue, dl = _head_inputs(b, c, r)
    q, k, (l32, _, g32), (l64, _, g64) = _head_reference(b, c, r, False)
    qg = q.cuda().requires_grad_(True)
    logits = H.moco_logits(qg, k.cuda(), queue.cuda(), T)
    assert logits.shape == (b, r + 1)
    torch.autograd.backward(logits, dl.cuda())
    what = "moco_logits (%d, %d, %d)" % (b, c, r)
    _eq("moco_logits", logits, l32, l64, what + " logits")
    _eq("moco_logits", qg.grad, g32, g64, what + " dq")
    np.testing.assert_allclose(_np(g64), _np(_dq64(k, queue, dl)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("b,c,r", HEAD_SHAPES)
def test_moco_logits_normalized(b, c, r):
    H = _H()
    _, _, queue, dl = _head_inputs(b, c, r)
    q, k, (l32, k32, g32), (l64, k64, g64) = _head_reference(b, c, r, True)
    queue_d, dl_d = queue.cuda(), dl.cuda()
    qg = q.cuda().requires_grad_(True)
    logits, k_hat = H.moco_logits_normalized(qg, k.cuda(), queue_d, T)
    assert logits.shape == (b, r + 1) and k_hat.shape == (b, c) and not k_hat.requires_grad
    torch.autograd.backward(logits, dl_d)
    what = "moco_logits_normalized (%d, %d, %d)" % (b, c, r)
    _eq("moco_fused", logits, l32, l64, what + " logits")
    _eq("moco_fused", k_hat, k32, k64, what + " k_hat")
    if c == 1:
        _cancelled(qg.grad, _dq64(k64, queue, dl) / q.double().abs(), what + " dq_raw")
    else:
        _eq("moco_fused", qg.grad, g32, g64, what + " dq_raw")
    # the kernel's promise: rows bit-identical to l2_normalize followed by moco_logits
    q2 = q.cuda().requires_grad_(True)
    kn = H.l2_normalize(k.cuda())
    logits2 = H.moco_logits(H.l2_normalize(q2), kn, queue_d, T)
    torch.autograd.backward(logits2, dl_d)
    assert torch.equal(logits.detach(), logits2.detach()), what + ": logits differ from the two-step form"
    assert torch.equal(k_hat, kn), what + ": k_hat differs from l2_normalize(k)"
    assert torch.equal(qg.grad, q2.grad), what + ": gradient differs from the two-step form"


def test_moco_logits_normalized_key_has_no_gradient():
    H = _H()
    q, k, queue, _ = _head_inputs(3, 48, 100)
    qg = q.cuda().requires_grad_(True)
    z = torch.zeros((), device="cuda", requires_grad=True)
    _, k_hat = H.moco_logits_normalized(qg, k.cuda(), queue.cuda(), T)
    assert not k_hat.requires_grad
    gq, gz = torch.autograd.grad(k_hat.sum() + z, [qg, z], allow_unused=True)
    torch.cuda.synchronize()
    assert gq is None and float(gz) == 1.0


def test_queue_lifetime():
    """An enqueue between forward and backward must not change the gradient: moco_logits and queue_stable=False keep a copy
    of the queue; queue_stable=True (no enqueue in between) gives the same bits without the copy."""
    H = _H()
    b, c, r = 4, 100, 260
    q, k, queue, dl = _head_inputs(b, c, r)
    new_keys = F.normalize(torch.randn(b, c, generator=_gen(5)), dim=1).cuda()
    g64_raw = _logits_formula(q.double(), k.double(), queue.double(), dl.double(), True)[2]
    g32_raw = _logits_formula(q, k, queue, dl, True)[2]
    qn, kn = F.normalize(q, dim=1), F.normalize(k, dim=1)
    g64_hat = _logits_formula(qn.double(), kn.double(), queue.double(), dl.double(), False)[2]
    g32_hat = _logits_formula(qn, kn, queue, dl, False)[2]

    def run(fused, stable, enqueue):
        queue_d = queue.cuda()
        ptr = torch.zeros(1, dtype=torch.long, device="cuda")
        qg = (q if fused else qn).cuda().requires_grad_(True)
        if fused:
            logits, _ = H.moco_logits_normalized(qg, k.cuda(), queue_d, T, queue_stable=stable)
        else:
            logits = H.moco_logits(qg, kn.cuda(), queue_d, T)
        if enqueue:
            H.queue_enqueue_(queue_d, ptr, new_keys)
            assert not torch.equal(queue_d.cpu(), queue) and int(ptr) == b
        torch.autograd.backward(logits, dl.cuda())
        return qg.grad

    for fused, g32, g64 in ((True, g32_raw, g64_raw), (False, g32_hat, g64_hat)):
        kept = run(fused, False, False)
        moved = run(fused, False, True)
        _eq("moco_fused" if fused else "moco_logits", moved, g32, g64, "gradient after an enqueue, fused=%s" % fused)
        assert torch.equal(moved, kept), "the enqueue between forward and backward changed the gradient (fused=%s)" % fused
    assert torch.equal(run(True, True, False), run(True, False, False))


def test_head_guards():
    H, L = _H(), _H().L
    g = _gen(3)
    for c, fused in ((1025, True), (8193, False)):
        b, r = 2, 3
        q, k, queue = (torch.randn(b, c, generator=g).cuda(), torch.randn(b, c, generator=g).cuda(),
                       torch.randn(c, r, generator=g).cuda())
        before = [t.clone() for t in (q, k, queue)]
        with pytest.raises(_err()):
            if fused:
                H.moco_logits_normalized(q, k, queue, T)
            else:
                H.moco_logits(q, k, queue, T)
        # the entry point itself: refused before anything is launched, the outputs keep their sentinels
        outs = [torch.full(s, -7.0, device="cuda") for s in ((b, r + 1), (b, c), (b,), (b, c))]
        if fused:
            rc = L.lib().mi_moco_logits_norm_fwd(L.ptr(q), L.ptr(k), L.ptr(queue), *[L.ptr(t) for t in outs], b, c, r, T, L.stream())
        else:
            rc = L.lib().mi_moco_logits_fwd(L.ptr(q), L.ptr(k), L.ptr(queue), L.ptr(outs[0]), b, c, r, T, L.stream())
        torch.cuda.synchronize()
        assert rc == -1
        assert all(bool((t == -7.0).all()) for t in outs)
        assert all(torch.equal(a, z) for a, z in zip((q, k, queue), before))
    q, k, queue, _ = [t.cuda() for t in _head_inputs(3, 48, 100)]
    qt, kt, queue_t = q.t().contiguous().t(), k.t().contiguous().t(), queue.t().contiguous().t()
    assert not qt.is_contiguous() and not queue_t.is_contiguous()
    for args in ((qt, k, queue), (q, kt, queue), (q, k, queue_t)):
        with pytest.raises(_err()):
            H.moco_logits(*args, T)
        with pytest.raises(_err()):
            H.moco_logits_normalized(*args, T)
    with pytest.raises(_err()):
        H.l2_normalize(qt)


# ------------------------------------------------------------------------------------------------
# 2. cross-entropy against label 0
# ------------------------------------------------------------------------------------------------
CE_SHAPES = [(1, 1), (1, 2), (3, 255), (5, 256), (7, 257), (130, 70), (64, 1025)]


@functools.lru_cache(maxsize=None)
def _ce_case(b, n, offset):
    """logits at the workload's scale (unit dot products / 0.07), optionally with +-offset added per row; the loss, and the
    gradient of 2.5 x loss, in float32 and float64 from the same fp32 inputs"""
    g = _gen(100 * b + n)
    l = (torch.rand(b, n, generator=g) * 2.0 - 1.0) / T
    if offset:
        l = l + offset * (1.0 - 2.0 * (torch.arange(b) % 2).float())[:, None]
    out = []
    for dt in (torch.float32, torch.float64):
        x = l.to(dt)
        onehot = torch.zeros_like(x)
        onehot[:, 0] = 1.0
        out.append(((torch.logsumexp(x, 1) - x[:, 0]).mean(), 2.5 * (torch.softmax(x, 1) - onehot) / b))
    return l, out[0], out[1]


@pytest.mark.parametrize("offset", [0.0, 40.0, 1e4], ids=["plain", "offset40", "offset1e4"])     # 40: just past the kernel's |lse| = 32
@pytest.mark.parametrize("b,n", CE_SHAPES)
def test_cross_entropy_label0(b, n, offset):
    H = _H()
    l, (loss32, g32), (loss64, g64) = _ce_case(b, n, offset)
    lg = l.cuda().requires_grad_(True)
    out = torch.full((), float("nan"), device="cuda")
    loss = H.cross_entropy_label0(lg, out=out)
    (2.5 * loss).backward()
    what = "cross_entropy_label0 (%d, %d)%s" % (b, n, " + offset %g" % offset if offset else "")
    _eq("cross_entropy", loss, loss32, loss64, what + " loss")
    assert torch.equal(out, loss.detach()), what + ": out= holds another value than the returned loss"
    _eq("cross_entropy", lg.grad, g32, g64, what + " dlogits")
    assert int(H._ce0_counter(lg.device)[:1]) == 0


CE_SEQUENCE = [(5, 257), (3, 70), (64, 1025), (1, 2), (5, 257)]


def _swap_ce0_tables():
    """Start from an empty stream -> word table (the process may have used many streams already); the caller restores it."""
    H = _H()
    saved = dict(H._CE0_COUNTERS)
    H.reset_ce0_counters()
    return saved


def _restore_ce0_tables(saved):
    H = _H()
    torch.cuda.synchronize()
    H._CE0_COUNTERS.clear()
    H._CE0_COUNTERS.update(saved)


def test_cross_entropy_ticket_back_to_back():
    """The arrival word must reset itself: launches of different B back to back on one stream, nothing in between."""
    H = _H()
    saved = _swap_ce0_tables()
    try:
        cases = [_ce_case(b, n, 0.0) for b, n in CE_SEQUENCE]
        inputs = [c[0].cuda() for c in cases]
        torch.cuda.synchronize()
        losses = [H.cross_entropy_label0(x) for x in inputs]
        word = H._ce0_counter(inputs[0].device)[:1]
        torch.cuda.synchronize()
        for (b, n), c, loss in zip(CE_SEQUENCE, cases, losses):
            _eq("cross_entropy", loss, c[1][0], c[2][0], "back to back (%d, %d)" % (b, n))
        assert int(word) == 0
    finally:
        _restore_ce0_tables(saved)


def test_cross_entropy_ticket_two_streams():
    H = _H()
    saved = _swap_ce0_tables()
    try:
        cases = [_ce_case(b, n, 0.0) for b, n in CE_SEQUENCE]
        on_side = [c[0].cuda() for c in cases]
        on_main = [c[0].cuda() for c in reversed(cases)]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        got_side, got_main = [], []
        for xs, xm in zip(on_side, on_main):
            with torch.cuda.stream(side):
                got_side.append(H.cross_entropy_label0(xs))
            got_main.append(H.cross_entropy_label0(xm))
        with torch.cuda.stream(side):
            word_side = H._ce0_counter(xs.device)[:1]
        word_main = H._ce0_counter(xs.device)[:1]
        torch.cuda.synchronize()
        assert word_side.data_ptr() != word_main.data_ptr()
        assert int(word_side) == 0 and int(word_main) == 0
        for (b, n), c, loss in zip(CE_SEQUENCE, cases, got_side):
            _eq("cross_entropy", loss, c[1][0], c[2][0], "side stream (%d, %d)" % (b, n))
        for (b, n), c, loss in zip(reversed(CE_SEQUENCE), reversed(cases), got_main):
            _eq("cross_entropy", loss, c[1][0], c[2][0], "default stream (%d, %d)" % (b, n))
    finally:
        _restore_ce0_tables(saved)


def test_cross_entropy_stream_table_limit():
    """64 words per device and never an alias: the 65th stream is refused until reset_ce0_counters() - on the Python table
    alone, with placeholder stream ids."""
    H = _H()
    l, (loss32, _), (loss64, _) = _ce_case(3, 255, 0.0)
    x = l.cuda()
    saved = _swap_ce0_tables()
    try:
        H.cross_entropy_label0(x)
        torch.cuda.synchronize()
        (_, slots), = H._CE0_COUNTERS.values()
        slots.clear()
        slots.update({-(i + 1): i for i in range(64)})
        with pytest.raises(_err()):
            H.cross_entropy_label0(x)
        assert len(slots) == 64
        H.reset_ce0_counters()
        assert not H._CE0_COUNTERS
        _eq("cross_entropy", H.cross_entropy_label0(x), loss32, loss64, "after reset_ce0_counters")
    finally:
        _restore_ce0_tables(saved)


# ------------------------------------------------------------------------------------------------
# 3. scalar reductions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,c", [(1, 1), (3, 5), (37, 100), (64, 2048)])
def test_rowdot_mean(b, c):
    H = _H()
    g = _gen(7 * b + c)
    a = F.normalize(torch.randn(b, c, generator=g), dim=1)
    t = F.normalize(torch.randn(b, c, generator=g), dim=1)
    ag, tg = a.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
    out = H.rowdot_mean(ag, tg)
    (-0.5 * out).backward()
    what = "rowdot_mean (%d, %d)" % (b, c)
    _eq("rowdot_mean", out, (a * t).sum(1).mean(), (a.double() * t.double()).sum(1).mean(), what)
    _eq("rowdot_mean", ag.grad, -0.5 * t / b, -0.5 * t.double() / b, what + " da")
    assert tg.grad is None


def _std_input(b, c, kind):
    g = _gen(31 * b + c)
    if kind == "near1000":
        return 1000.0 + 0.01 * (2.0 * torch.randint(0, 2, (b, c), generator=g).float() - 1.0)
    x = torch.randn(b, c, generator=g)
    if kind == "constant_column":
        x[:, c // 2] = 1000.01
    return x


@pytest.mark.parametrize("kind", ["randn", "constant_column", "near1000"])
@pytest.mark.parametrize("b,c", [(2, 1), (3, 257), (5, 300), (64, 2048)])
def test_column_std_mean(b, c, kind):
    H = _H()
    x = _std_input(b, c, kind)
    got = H.column_std_mean(x.cuda())
    _eq("column_std", got, x.std(0).mean(), x.double().std(0).mean(), "column_std_mean (%d, %d) %s" % (b, c, kind))


@pytest.mark.parametrize("b,c", [(2, 1), (5, 300), (64, 2048)])
def test_column_std_mean_of_constant_columns_is_zero(b, c):
    """A constant column's one-pass variance may round below zero; the clamp makes it exactly 0."""
    H = _H()
    x = (torch.randn(1, c, generator=_gen(c)) * _row_scales(c).t()).expand(b, c).contiguous()
    assert float(x.double().std(0).max()) == 0.0
    assert float(H.column_std_mean(x.cuda())) == 0.0


def test_column_std_mean_single_row():
    """B = 1: the kernel's documented choice is 0 (torch.std gives NaN)."""
    H = _H()
    x = torch.randn(1, 300, generator=_gen(2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # (torch warns about the zero degrees of freedom)
        assert bool(torch.isnan(x.std(0).mean()))
    assert float(H.column_std_mean(x.cuda())) == 0.0


def test_scalar_accumulate():
    H = _H()
    sentinels = np.array([10.0, 20.0, 30.0, 40.0, 50.0, 60.0], np.float32)
    vals = np.array([0.1, 0.2, 0.3, 0.7], np.float32)
    scalars = [torch.tensor(float(v)).cuda() if i % 2 == 0 else torch.tensor([float(v)]).cuda() for i, v in enumerate(vals)]
    for count in (0, 1, 3, 4):
        sums = torch.from_numpy(sentinels).cuda()
        H.scalar_accumulate_(sums, *scalars[:count])
        want = sentinels.copy()
        want[:count] += vals[:count]
        np.testing.assert_array_equal(_np(sums), want)
    sums = torch.from_numpy(sentinels).cuda()
    want = sentinels.copy()
    for _ in range(20):
        H.scalar_accumulate_(sums, *scalars[:3])
        want[:3] += vals[:3]                       # the float32 running sum
    np.testing.assert_array_equal(_np(sums), want)
    with pytest.raises(_err()):
        H.scalar_accumulate_(sums, *(scalars + scalars[:1]))
    with pytest.raises(_err()):
        H.scalar_accumulate_(sums[:2], *scalars[:3])
    np.testing.assert_array_equal(_np(sums), want)


# ------------------------------------------------------------------------------------------------
# 4. flat-arena passes
# ------------------------------------------------------------------------------------------------
ARENA_LENGTHS = [1, 2, 3, 5, 4 * 257, 4003, LONG]


@functools.lru_cache(maxsize=None)
def _arena(n):
    g = _gen(n)
    return tuple(torch.randn(n, generator=g) for _ in range(3))


@pytest.mark.parametrize("n", ARENA_LENGTHS)
def test_ema_update(n):
    H = _H()
    k, q, _ = _arena(n)
    kd, qd = k.cuda(), q.cuda()
    H.ema_update_(kd, qd, 0.99)
    _eq("arena", kd, k * 0.99 + q * (1.0 - 0.99), k.double() * 0.99 + q.double() * (1.0 - 0.99), "ema_update_ n=%d" % n)
    assert torch.equal(qd.cpu(), q)


@pytest.mark.parametrize("n", ARENA_LENGTHS)
def test_sgd_step(n):
    H = _H()
    p, g1, g2 = _arena(n)
    p64, g64, h64 = p.double(), g1.double(), g2.double()
    lr_dev = torch.tensor([0.02], dtype=torch.float32).cuda()
    g1d, g2d = g1.cuda(), g2.cuda()

    pd = p.cuda()
    H.sgd_step_(pd, g1d, 0.05)
    _eq("arena", pd, p - 0.05 * g1, p64 - 0.05 * g64, "sgd_step_ n=%d" % n)
    pd = p.cuda()
    H.sgd_step_(pd, g1d, 0.05, weight_decay=1e-2, grad_scale=0.5)
    _eq("arena", pd, p - 0.05 * (0.5 * g1 + 1e-2 * p), p64 - 0.05 * (0.5 * g64 + 1e-2 * p64), "sgd_step_ wd gs n=%d" % n)
    pd = p.cuda()
    H.sgd_step_(pd, g1d, 123.0, weight_decay=1e-2, lr_dev=lr_dev, grad_scale=0.125)      # the device value overrides the host's
    _eq("arena", pd, p - 0.02 * (0.125 * g1 + 1e-2 * p), p64 - 0.02 * (0.125 * g64 + 1e-2 * p64), "sgd_step_ lr_dev n=%d" % n)

    pd = p.cuda()
    H.sgd_step2_(pd, g1d, g2d, 0.05)
    _eq("arena", pd, p - 0.05 * (g1 + g2), p64 - 0.05 * (g64 + h64), "sgd_step2_ n=%d" % n)
    pd = p.cuda()
    H.sgd_step2_(pd, g1d, g2d, 0.05, weight_decay=1e-2, grad_scale=0.5)
    _eq("arena", pd, p - 0.05 * (0.5 * (g1 + g2) + 1e-2 * p), p64 - 0.05 * (0.5 * (g64 + h64) + 1e-2 * p64),
        "sgd_step2_ wd gs n=%d" % n)
    pd = p.cuda()
    H.sgd_step2_(pd, g1d, g2d, 123.0, weight_decay=1e-2, lr_dev=lr_dev, grad_scale=0.125)
    _eq("arena", pd, p - 0.02 * (0.125 * (g1 + g2) + 1e-2 * p), p64 - 0.02 * (0.125 * (g64 + h64) + 1e-2 * p64),
        "sgd_step2_ lr_dev n=%d" % n)
    assert torch.equal(g1d.cpu(), g1) and torch.equal(g2d.cpu(), g2)


def test_arena_passes_refuse_misaligned():
    H = _H()
    n = 4003
    p, g1, g2 = _arena(n)
    whole = [torch.cat([torch.zeros(1), t]).cuda() for t in (p, g1, g2)]
    off = [w[1:] for w in whole]                 # 4 bytes past a 16-byte boundary
    ok = [t.cuda() for t in (p, g1, g2)]
    assert all(t.data_ptr() % 16 == 4 for t in off) and all(t.data_ptr() % 16 == 0 for t in ok)
    calls = [lambda a, b, c: H.ema_update_(a, b, 0.99), lambda a, b, c: H.sgd_step_(a, b, 0.05),
             lambda a, b, c: H.sgd_step2_(a, b, c, 0.05)]
    for i, call in enumerate(calls):
        for bad in range(2 if i < 2 else 3):
            args = [off[j] if j == bad else ok[j] for j in range(3)]
            with pytest.raises(_err()):
                call(*args)
            torch.cuda.synchronize()
            assert torch.equal(args[0].cpu(), p), "p was written by a refused call"


def _framed(n, lead, fill=-7.0):
    """a destination of n floats inside a larger parent, `lead` floats in: (parent, view)"""
    parent = torch.full((lead + n + 8,), fill, device="cuda")
    return parent, parent[lead:lead + n]


def _check_framed(parent, lead, n, want, fill=-7.0):
    got = _np(parent)
    np.testing.assert_array_equal(got[lead:lead + n], _np(want).ravel())
    np.testing.assert_array_equal(got[:lead], np.full(lead, fill, np.float32))
    np.testing.assert_array_equal(got[lead + n:], np.full(8, fill, np.float32))


@pytest.mark.parametrize("case", ["long", "four", "not_multiple_of_4", "unequal_sizes", "strided_source", "misaligned"])
def test_copy_pair(case):
    """One launch when the four are aligned, contiguous, equal in size and a multiple of four long; otherwise two copy_."""
    H = _H()
    n0 = n1 = {"long": LONG4, "four": 4, "not_multiple_of_4": 6}.get(case, 8)
    if case == "unequal_sizes":
        n1 = 12
    lead = 1 if case == "misaligned" else 4
    g = _gen(n0)
    s0, s1 = torch.randn(n0, generator=g).cuda(), torch.randn(n1, generator=g).cuda()
    if case == "strided_source":
        s0 = torch.randn(2 * n0, generator=g).cuda()[::2]
        assert not s0.is_contiguous()
    p0, d0 = _framed(n0, lead)
    p1, d1 = _framed(n1, 4)
    assert d0.data_ptr() % 16 == (4 if case == "misaligned" else 0)
    want0, want1 = s0.clone(), s1.clone()
    H.copy_pair_(d0, s0, d1, s1)
    _check_framed(p0, lead, n0, want0)
    _check_framed(p1, 4, n1, want1)
    assert torch.equal(s0, want0) and torch.equal(s1, want1)


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("n", [4, LONG4])
def test_relu_mask(n, with_add):
    H = _H()
    g = _gen(n)
    dy, y, add = (torch.randn(n, generator=g) for _ in range(3))
    y[0::7] = 0.0
    y[3::11] = -0.0
    y[1] = 0.0 if n == 4 else y[1]
    up = dy + add if with_add else dy
    want = torch.where(y > 0, up, torch.zeros_like(up))
    got = H.relu_mask(dy.cuda(), y.cuda(), add.cuda() if with_add else None)
    np.testing.assert_array_equal(_np(got), _np(want))


def test_relu_mask_refuses_a_ragged_length():
    H = _H()
    t = torch.ones(6, device="cuda")
    with pytest.raises(_err()):
        H.relu_mask(t, t)


class _BiasHolder(nn.Module):
    def __init__(self, bias):
        super().__init__()
        self.bias = nn.Parameter(bias)


@pytest.mark.parametrize("shape", [(5, 3), (4099, 32), (3, 7, 9, 16)])
def test_bias_add(shape):
    H = _H()
    g = _gen(sum(shape))
    x, dy, bias = torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.randn(shape[-1], generator=g)
    holder = _BiasHolder(bias.cuda())
    xg = x.cuda().requires_grad_(True)
    y = H.bias_add(xg, holder)
    y.backward(dy.cuda())
    what = "bias_add %s" % (shape,)
    _eq("bias_add", y, x + bias, x.double() + bias.double(), what)
    assert torch.equal(xg.grad.cpu(), dy)
    assert torch.equal(xg.detach().cpu(), x)
    c = shape[-1]
    _eq("bias_add", holder.bias.grad, dy.reshape(-1, c).sum(0), dy.double().reshape(-1, c).sum(0), what + " dbias")


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (3, 2, 3, 5, 48), (5, 4, 4, 4, 100)])
def test_global_avgpool(shape):
    H = _H()
    g = _gen(sum(shape))
    x, dy = torch.randn(shape, generator=g), torch.randn(shape[0], shape[-1], generator=g)
    ref = {}
    for dt in (torch.float32, torch.float64):
        xr = x.to(dt).clone().requires_grad_(True)
        y = xr.mean((1, 2, 3))
        y.backward(dy.to(dt))
        ref[dt] = (y.detach(), xr.grad)
    xg = x.cuda().requires_grad_(True)
    y = H.global_avgpool(xg)
    assert y.shape == (shape[0], shape[-1])
    y.backward(dy.cuda())
    what = "global_avgpool %s" % (shape,)
    _eq("avgpool", y, ref[torch.float32][0], ref[torch.float64][0], what)
    _eq("avgpool", xg.grad, ref[torch.float32][1], ref[torch.float64][1], what + " dx")


# ------------------------------------------------------------------------------------------------
# 5. queue
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,c,r,start", [(256, 256, 512, 0),        # B * C = 65536: the last size of the one-launch path
                                         (512, 256, 1024, 0),       # copy launch + pointer launch
                                         (300, 256, 900, 600)])     # B * C = 76800, three batches per lap, pointer at R - B
def test_queue_enqueue(b, c, r, start):
    H = _H()
    g = _gen(b + r)
    want = np.full((c, r), -7.0, np.float32)
    queue = torch.from_numpy(want.copy()).cuda()
    ptr = torch.tensor([start], dtype=torch.long).cuda()
    p = start
    for step in range(2 * (r // b) + 1):           # two laps and one more
        keys = torch.randn(b, c, generator=g)
        H.queue_enqueue_(queue, ptr, keys.cuda())
        want[:, p:p + b] = keys.numpy().T
        p = (p + b) % r
        np.testing.assert_array_equal(_np(queue), want, err_msg="step %d" % step)
        assert ptr.dtype == torch.long and int(ptr) == p, "step %d" % step


@pytest.mark.parametrize("b,c,r", [(3, 8, 10), (300, 256, 1000)])
def test_queue_enqueue_refuses_a_ragged_queue(b, c, r):
    H, L = _H(), _H().L
    queue = torch.full((c, r), -7.0, device="cuda")
    ptr = torch.zeros(1, dtype=torch.long, device="cuda")
    keys = torch.ones(b, c, device="cuda")
    with pytest.raises((AssertionError, _err())):
        H.queue_enqueue_(queue, ptr, keys)
    assert L.lib().mi_queue_enqueue(L.ptr(queue), L.ptr(ptr), L.ptr(keys), b, c, r, L.stream()) == -1
    torch.cuda.synchronize()
    assert bool((queue == -7.0).all()) and int(ptr) == 0
