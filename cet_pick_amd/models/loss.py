"""Detector-training losses on the MI355X: mirror of the reference's `cet_pick/models/loss.py` for the classes the
semi-supervised trainer uses (trains/tomo_cr_semi_trainer.py:23-41): `_neg_loss` / `FocalLoss` (:378-411),
`_pu_neg_loss` / `PULoss` (:255-324), `_pu_ge_loss` / `PUGELoss` (:215-253, :327-337, the trainer's --ge),
`ConsistencyLoss` (:701-712), `UnbiasedConLoss` (:571-699), `SupConLossV2_more` (:759-818, the trainer's --pn).

The voxel losses are single fused reductions (csrc/loss_ops.hip, csrc/loss_ge.hip) with hand-written backward kernels; the
data-dependent branch of the PU risk is taken on the device, and so is the count sum of the GE penalty.  `UnbiasedConLoss` never builds the (2N)^2 similarity
matrix: an MFMA kernel streams its tiles and returns the four row sums the loss is a function of; the O(N) tail
(clamps, logs, masked means) is ordinary tensor arithmetic on those vectors.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _lib as L
from .. import hipops as H


def _flat(t, name):
    L.require_cuda(t, name)
    return t.contiguous().view(-1)


class _VoxelLossFn(torch.autograd.Function):
    """mode: 'pu' | 'focal' | 'mse'."""

    @staticmethod
    def forward(ctx, pred, gt, mode, tau, beta):
        p, g = _flat(pred, "pred"), _flat(gt, "gt")
        if p.numel() != g.numel():
            raise ValueError("pred and gt differ in size: %s vs %s" % (tuple(pred.shape), tuple(gt.shape)))
        n = p.numel()
        if n == 0:
            raise ValueError("voxel loss of an empty tensor: pred %s, gt %s" % (tuple(pred.shape), tuple(gt.shape)))
        ws = L.workspace(L.lib().mi_voxel_loss_workspace_bytes(n), p.device, "voxloss")
        sums = torch.empty(11, dtype=torch.float64, device=p.device)
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        if mode == "pu":
            L.call("mi_pu_focal_loss_fwd", p, g, n, float(tau), float(beta), sums, loss, ws, ws.numel())
        elif mode == "focal":
            L.call("mi_focal_loss_fwd", p, g, n, sums, loss, ws, ws.numel())
        else:
            L.call("mi_mse_loss_fwd", p, g, n, sums, loss, ws, ws.numel())
        ctx.save_for_backward(p, g, sums)
        ctx.mode, ctx.tau, ctx.shape_p, ctx.shape_g = mode, float(tau), pred.shape, gt.shape
        ctx.g_needs = gt.requires_grad
        ctx.sums = sums
        return loss

    @staticmethod
    def backward(ctx, dloss):
        p, g, sums = ctx.saved_tensors
        n = p.numel()
        dl = dloss.contiguous().float()
        dp = torch.empty_like(p)
        dg = None
        if ctx.mode == "pu":
            L.call("mi_pu_focal_loss_bwd", p, g, n, ctx.tau, sums, dl, dp)
        elif ctx.mode == "focal":
            L.call("mi_focal_loss_bwd", p, g, n, sums, dl, dp)
        else:
            dg = torch.empty_like(g) if ctx.g_needs else None
            L.call("mi_mse_loss_bwd", p, g, n, sums, dl, dp, dg)
        return dp.view(ctx.shape_p), (dg.view(ctx.shape_g) if dg is not None else None), None, None, None


_NO_POS = ("Num of true positive is zero, please check tomogram size of input coordinates order or use smaller "
           "translation ratio")


def _neg_loss(pred, gt):
    """loss.py:378-411."""
    return _VoxelLossFn.apply(pred, gt, "focal", 0.0, 0.0)


def _pu_neg_loss(pred, gt, tau, beta, gamma, check_positives=True):
    """loss.py:255-308.  check_positives: the reference's ValueError on zero positives (one host sync)."""
    if check_positives and not bool((gt == 1).any()):
        raise ValueError(_NO_POS)
    return _VoxelLossFn.apply(pred, gt, "pu", tau, beta)


class FocalLoss(nn.Module):
    def forward(self, out, target):
        return _neg_loss(out, target)


class PULoss(nn.Module):
    """loss.py:310-324.  Labels without an unlabeled (-1) voxel make the negative risk 0 / 0: the loss is NaN, as the reference's
    is.  The gradient is then unspecified - the reference's is NaN everywhere, this one's is finite (no voxel takes the 1 / 0
    coefficient)."""

    def __init__(self, tau, beta=0, gamma=1):
        super().__init__()
        self.tau, self.beta, self.gamma = tau, beta, gamma
        self.puloss = _pu_neg_loss

    def forward(self, pred, gt):
        return self.puloss(pred, gt, self.tau, self.beta, self.gamma)


def _check_tau(tau):
    if not 0.0 < float(tau) < 1.0:           # log Binom(k; N, tau) is infinite at the ends
        raise ValueError("PUGELoss needs 0 < tau < 1, got %r" % (tau,))


class _PUGELossFn(torch.autograd.Function):
    """mi_pu_ge_loss_fwd / _bwd; `grad_fn.sums` is the 16-double record of include/cetpick_hip.h."""

    @staticmethod
    def forward(ctx, pred, gt, tau, slack, entropy_penalty):
        _check_tau(tau)
        p, g = _flat(pred, "pred"), _flat(gt, "gt")
        if p.numel() != g.numel():
            raise ValueError("pred and gt differ in size: %s vs %s" % (tuple(pred.shape), tuple(gt.shape)))
        n = p.numel()
        if n == 0:
            raise ValueError("voxel loss of an empty tensor: pred %s, gt %s" % (tuple(pred.shape), tuple(gt.shape)))
        ws = L.workspace(L.lib().mi_pu_ge_loss_workspace_bytes(n), p.device, "geloss")
        sums = torch.empty(16, dtype=torch.float64, device=p.device)
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        L.call("mi_pu_ge_loss_fwd", p, g, n, float(tau), float(slack), float(entropy_penalty), sums, loss, ws, ws.numel())
        ctx.save_for_backward(p, g, sums)
        ctx.slack, ctx.shape_p = float(slack), pred.shape
        ctx.sums = sums
        return loss

    @staticmethod
    def backward(ctx, dloss):
        p, g, sums = ctx.saved_tensors
        dl = dloss.contiguous().float()
        dp = torch.empty_like(p)
        L.call("mi_pu_ge_loss_bwd", p, g, p.numel(), ctx.slack, sums, dl, dp)
        return dp.view(ctx.shape_p), None, None, None, None


class PUGELoss(nn.Module):
    """loss.py:215-253, :327-337: the generalised-expectation form of the positive-unlabeled objective - the focal loss on the
    labelled voxels (gt >= 0) + slack x a penalty that ties the expected particle count among the unlabeled voxels (gt == -1) to a
    Binomial(N, tau) prior (csrc/loss_ge.hip has the formula).  The classifier part is the fused focal loss: `criteria` is None or
    a `FocalLoss` (what the trainer passes, tomo_cr_semi_trainer.py:27-29), anything else is refused.  Labels without an unlabeled
    voxel give the focal loss alone.  With entropy_penalty > 0 and v = sum p (1 - p) = 0 over the unlabeled voxels the loss is
    -inf, as the reference's is."""

    def __init__(self, tau, criteria=None, slack=1, entropy_penalty=0):
        super().__init__()
        _check_tau(tau)
        if criteria is not None and not isinstance(criteria, FocalLoss):
            raise L.HipExtensionError("PUGELoss runs its classifier part fused with the penalty: criteria must be None or a "
                                      "FocalLoss, got %s" % type(criteria).__name__)
        self.tau, self.slack, self.entropy_penalty = tau, slack, entropy_penalty
        self.criteria = criteria

    def forward(self, pred, gt):
        return _PUGELossFn.apply(pred, gt, self.tau, self.slack, self.entropy_penalty)


class ConsistencyLoss(nn.Module):
    def forward(self, out_prob, out_prob_cr):
        return _VoxelLossFn.apply(out_prob, out_prob_cr, "mse", 0.0, 0.0)


class _UclRowSumsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, cls, inv_T):
        if feat.dim() != 2 or feat.shape[0] < 2 or feat.shape[0] % 2 or feat.shape[1] not in (32, 64):
            raise L.HipExtensionError("mi_ucl_rowsums takes (2N, 32) or (2N, 64) features with N >= 1, got %s" % (tuple(feat.shape),))
        L.require_cuda(feat, "features")
        L.require_cuda(cls, "class bytes", dtype=torch.uint8)
        if not feat.is_contiguous() or not cls.is_contiguous() or tuple(cls.shape) != (feat.shape[0],):
            raise L.HipExtensionError("mi_ucl_rowsums takes contiguous features %s and one contiguous class byte per row, got %s"
                                      % (tuple(feat.shape), tuple(cls.shape)))
        n2, dim = feat.shape
        dev = feat.device
        outs = [torch.empty(n2, dtype=torch.float32, device=dev) for _ in range(5)]
        L.call("mi_ucl_rowsums_fwd", feat, cls, n2, dim, float(inv_T), *outs)
        ctx.save_for_backward(feat, cls, outs[0])
        ctx.inv_T = float(inv_T)
        ctx.mark_non_differentiable(outs[0])
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_max, g_all, g_pos, g_other, g_pair):
        feat, cls, rowmax = ctx.saved_tensors
        n2, dim = feat.shape
        z = lambda g: torch.zeros(n2, dtype=torch.float32, device=feat.device) if g is None else g.contiguous().float()
        g_all, g_pos, g_other, g_pair = z(g_all), z(g_pos), z(g_other), z(g_pair)
        dfeat = torch.empty_like(feat)
        rng = torch.empty(2, dtype=torch.float32, device=feat.device)      # (largest row maximum, fast-path flag): decided on the device
        L.call("mi_ucl_rowsums_bwd_ranged", feat, cls, n2, dim, ctx.inv_T, rowmax, g_all, g_pos, g_other, g_pair, dfeat, rng)
        return dfeat, None, None


def _pad_features(feat):
    """(2N, dim) -> contiguous (2N, 32) or (2N, 64): the kernel widths; zero columns do not change any inner product"""
    dim = feat.shape[1]
    if dim not in (32, 64):
        pad = (32 if dim < 32 else 64) - dim
        if pad < 0:
            raise L.HipExtensionError("feature dim %d > 64 is not supported by mi_ucl_rowsums" % dim)
        feat = torch.nn.functional.pad(feat, (0, pad))
    return L.require_cuda(feat, "features").contiguous()


class _SupConPNFn(torch.autograd.Function):
    """The scalar of `SupConLossV2_more` from (2N, 32 | 64) features and one class byte per row: mi_ucl_rowsums_fwd (m_i, Z_i), then
    mi_supcon_pn_rows_fwd (the linear terms, log Z, the two masked means).  Backward: mi_ucl_rowsums_bwd_ranged with
    g_all = d loss / d Z alone, then mi_supcon_pn_rows_bwd.  `grad_fn.sums` is the 72-double record of include/cetpick_hip.h."""

    @staticmethod
    def forward(ctx, feat, cls, inv_T):
        if feat.dim() != 2 or feat.shape[0] < 2 or feat.shape[0] % 2 or feat.shape[1] not in (32, 64):
            raise L.HipExtensionError("mi_supcon_pn_rows takes (2N, 32) or (2N, 64) features with N >= 1, got %s" % (tuple(feat.shape),))
        L.require_cuda(feat, "features")
        L.require_cuda(cls, "class bytes", dtype=torch.uint8)
        if not feat.is_contiguous() or not cls.is_contiguous() or tuple(cls.shape) != (feat.shape[0],):
            raise L.HipExtensionError("mi_supcon_pn_rows takes contiguous features %s and one contiguous class byte per row, got %s"
                                      % (tuple(feat.shape), tuple(cls.shape)))
        n2, dim = feat.shape
        dev = feat.device
        rowmax, s_all, s_pos, s_other, e_pair, g_all = (torch.empty(n2, dtype=torch.float32, device=dev) for _ in range(6))
        L.call("mi_ucl_rowsums_fwd", feat, cls, n2, dim, float(inv_T), rowmax, s_all, s_pos, s_other, e_pair)
        ws = L.workspace(L.lib().mi_supcon_pn_rows_workspace_bytes(n2), dev, "supconpn")
        sums = torch.empty(72, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        L.call("mi_supcon_pn_rows_fwd", feat, cls, n2, dim, float(inv_T), rowmax, s_all, g_all, sums, loss, ws, ws.numel())
        ctx.save_for_backward(feat, cls, rowmax, g_all, sums)
        ctx.inv_T = float(inv_T)
        ctx.sums = sums
        return loss

    @staticmethod
    def backward(ctx, dloss):
        feat, cls, rowmax, g_all, sums = ctx.saved_tensors
        n2, dim = feat.shape
        dl = dloss.contiguous().float()
        zero = torch.zeros(n2, dtype=torch.float32, device=feat.device)
        dfeat = torch.empty_like(feat)
        rng = torch.empty(2, dtype=torch.float32, device=feat.device)
        L.call("mi_ucl_rowsums_bwd_ranged", feat, cls, n2, dim, ctx.inv_T, rowmax, g_all, zero, zero, zero, dfeat, rng)
        L.call("mi_supcon_pn_rows_bwd", feat, cls, n2, dim, ctx.inv_T, sums, dl, dfeat)
        return dfeat, None, None


class SupConLossV2_more(nn.Module):
    """loss.py:759-818, the contrastive term of the fully annotated trainer (--pn): ONE scalar over the 2N stacked rows,

        -mean_{i pos} [sum_{j pos} log E_ij / P2 - log Z_i]  -  mean_{i un} [log E_i,pair(i) - log Z_i]

    with E, Z as in `UnbiasedConLoss`, pos = label > thresh, un = label < thresh (a label equal to thresh is in neither), P2 = |pos|.
    log E is linear in the similarities, so only Z needs the (2N)^2 walk.  The heat-map arguments are unused, as in the
    reference.  No positive row: the package's "no positives" ValueError; no un row: a ValueError (the reference returns NaN)."""

    def __init__(self, base_temperature, contrast_mode="all"):
        super().__init__()
        self.base_temperature = base_temperature
        self.contrast_mode = contrast_mode

    def forward(self, labels, out_labels, out_labels_cr, all_features, all_features_cr, opt):
        labels = labels.reshape(-1)
        all_labels = torch.cat([labels, labels], dim=0)
        pos = all_labels.gt(opt.thresh)
        un = all_labels.lt(opt.thresh)
        n_pos, n_un = (int(v) for v in torch.stack([pos.sum(), un.sum()]).tolist())      # one host read, as the reference's checks
        if n_pos == 0:
            raise ValueError(_NO_POS)
        if n_un == 0:
            raise ValueError("SupConLossV2_more: no label lies below --thresh %g, the mean over the negative rows is empty"
                             % opt.thresh)
        feat = _pad_features(torch.cat([all_features, all_features_cr], dim=0).float())
        cls = (pos.to(torch.uint8) | (un.to(torch.uint8) << 1)).contiguous()
        return _SupConPNFn.apply(feat, cls, 1.0 / self.base_temperature)


class SCANLoss(nn.Module):
    """loss.py:87-119, one head: forward(anchors, neighbors) -> (total, consistency, entropy) from two (b, num_classes) logits
    tensors, 1 <= num_classes <= 64, b <= 65536 (csrc/scan_loss.hip).  `total` carries the gradient; the other two
    are figures to log, as the reference's trainer uses them."""

    def __init__(self, entropy_weight=2.0):
        super().__init__()
        self.entropy_weight = entropy_weight

    def forward(self, anchors, neighbors):
        total, stats = H.scan_loss(anchors, neighbors, 1, self.entropy_weight)
        return total, stats[0, 1], stats[0, 2]


class MultiHeadSCANLoss(nn.Module):
    """The reference's TomoSCANLoss over a ClusteringModel's list of heads, in one launch: anchors, neighbors (b, nheads x
    num_classes), head h in columns h num_classes .. -> (the sum of the heads' totals - the scalar that is differentiated -, stats
    (nheads, 3): total, consistency, entropy per head, no gradient)."""

    def __init__(self, nheads, entropy_weight=2.0):
        super().__init__()
        self.nheads, self.entropy_weight = int(nheads), entropy_weight

    def forward(self, anchors, neighbors):
        return H.scan_loss(anchors, neighbors, self.nheads, self.entropy_weight)


class MaskedCrossEntropyLoss(nn.Module):
    """loss.py:55-66: forward(input, target, mask, weight, reduction='mean') - the cross-entropy of the rows of `input` (b,
    num_classes) where `mask` is set against `target`, each row weighted by weight[target] (None: 1) and the sum divided by the sum
    of the weights; ValueError on an all-zero mask, as the reference (one host read).  On the device this is the self-label kernel
    fed with logits that reproduce the given target and mask (csrc/scan_selflabel.hip); `weight` may only be the
    reference's own: None, or the inverse class shares ConfidenceBasedCE forms - any other weight vector is refused."""

    def forward(self, input, target, mask, weight, reduction="mean"):
        if reduction != "mean":
            raise ValueError("MaskedCrossEntropyLoss is built for reduction='mean', got %r" % (reduction,))
        L.require_cuda(input, "input")
        if not bool((mask != 0).any()):
            raise ValueError("Mask in MaskedCrossEntropyLoss is all zeros.")
        b, c = input.shape
        # weak logits whose softmax has the given target and mask: 100 on the target of a masked row (probability 1 > 0.5 in
        # float64 for c <= 64), 0 everywhere on an unmasked row (probability 1 / c <= 0.5, or c = 1: handled by the bias below)
        weak = torch.zeros((b, c), dtype=torch.float32, device=input.device)
        rows = torch.nonzero(mask.reshape(-1) != 0).reshape(-1)
        weak[rows, target.reshape(-1)[rows].long()] = 100.0
        if c == 1 and not bool((mask != 0).all()):
            raise ValueError("MaskedCrossEntropyLoss with one class needs every row masked")
        loss, info, count, got_target, _ = H.scan_selflabel(weak, input.contiguous(), 0.5, weight is not None)
        if weight is not None:
            n = int(info[0])                               # (the reference's own weights: 1 / (counts.float() / n), else 1)
            want = torch.ones(c, dtype=torch.float32, device=input.device)
            present = count > 0
            want[present] = 1 / (count[present].float() / n)
            if not torch.allclose(want, weight.to(want), rtol=1e-6, atol=0):
                raise ValueError("MaskedCrossEntropyLoss takes the class-balancing weights of ConfidenceBasedCE or None")
        return loss


class ConfidenceBasedCE(nn.Module):
    """loss.py:15-53, SCAN's self-labelling loss: forward(anchors_weak, anchors_strong) -> the cross-entropy of the strong logits
    against the classes the weak logits are confident of (largest probability above `threshold`), with `apply_class_balancing`
    each class weighted by its inverse share among the confident rows.  ValueError when no row is confident, as the reference
    (one host read); hipops.scan_selflabel_loss is the form that never reads the host and gives loss 0 there."""

    def __init__(self, threshold, apply_class_balancing):
        super().__init__()
        self.threshold = threshold
        self.apply_class_balancing = apply_class_balancing

    def forward(self, anchors_weak, anchors_strong):
        loss, info, _ = H.scan_selflabel_loss(anchors_weak, anchors_strong, self.threshold, self.apply_class_balancing)
        if int(info[0]) == 0:
            raise ValueError("Mask in MaskedCrossEntropyLoss is all zeros.")
        return loss


class UnbiasedConLoss(nn.Module):
    """loss.py:571-699: debiased contrastive regularisation; returns (supervised, unsupervised) terms."""

    def __init__(self, base_temperature, class_prob):
        super().__init__()
        self.base_temperature = base_temperature
        self.tau_plus = class_prob

    def calc_g(self, pos_mean, neg_mean, class_prob):
        Ng = (neg_mean - class_prob * pos_mean) / (1 - class_prob)
        return torch.clamp(Ng, min=np.e ** (-1 / self.base_temperature))

    def forward(self, labels, out_labels, out_labels_cr, all_features, all_features_cr, opt):
        labels = labels.reshape(-1)
        n = all_features.shape[0]
        pos1 = labels.gt(opt.thresh) if opt.thresh < 1 else labels.eq(1)
        num_of_positives = pos1.sum()
        if num_of_positives == 0:            # the reference's host-side check (loss.py:607-608)
            raise ValueError(_NO_POS)
        num_of_negatives = 2 * (n - num_of_positives)
        feat = _pad_features(torch.cat([all_features, all_features_cr], dim=0).float())
        all_labels = torch.cat([labels, labels], dim=0)
        all_out_preds = torch.cat([out_labels.reshape(-1), out_labels_cr.reshape(-1)], dim=0)
        pos = all_labels.gt(opt.thresh) if opt.thresh < 1 else all_labels.eq(1)
        other = all_labels.lt(opt.thresh)
        un = all_labels.lt(0)
        cls = (pos.to(torch.uint8) | (other.to(torch.uint8) << 1)).contiguous()
        _, s_all, s_pos, s_other, e_pair = _UclRowSumsFn.apply(feat, cls, 1.0 / self.base_temperature)

        posf, unf = pos.float(), un.float()
        # supervised term over the positive anchors (loss.py:644-650)
        pos_feat_mean = s_pos / (posf.sum() - 1)
        rem_feat_mean = s_other / other.float().sum()
        Ng = self.calc_g(pos_feat_mean, rem_feat_mean, self.tau_plus)
        sup_rows = -torch.log(pos_feat_mean / (pos_feat_mean + Ng))
        debiased_loss_sup = (torch.where(pos, sup_rows, torch.zeros_like(sup_rows))).sum() / posf.sum()

        # unsupervised term over the unlabeled anchors (loss.py:653-694); masked means instead of boolean indexing
        up = e_pair
        urem = (s_all - e_pair) / num_of_negatives
        Ng_pos = self.calc_g(up, urem, self.tau_plus)
        Ng_neg = self.calc_g(up, urem, 1 - self.tau_plus)
        lpos = -torch.log(up / (up + Ng_pos)) * all_out_preds
        lneg = -torch.log(up / (up + Ng_neg)) * (1 - all_out_preds)

        def masked_mean(v, m):
            cnt = m.float().sum()
            s = torch.where(m, v, torch.zeros_like(v)).sum()
            return torch.where(cnt > 0, s / cnt.clamp(min=1), torch.zeros_like(s))

        m_hi = un & all_out_preds.gt(0.99)
        m_lo = un & all_out_preds.lt(0.01)
        m_mid = un & all_out_preds.gt(0.01) & all_out_preds.lt(0.99)
        debiased_loss_unsup = masked_mean(lpos, m_hi) + masked_mean(lneg, m_lo) + masked_mean(lpos, m_mid) + \
            masked_mean(lneg, m_mid)
        return debiased_loss_sup, debiased_loss_unsup
