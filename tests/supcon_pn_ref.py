"""`SupConLossV2_more` (the contrastive term of --pn) restated twice in float64 torch, for tests/test_supcon_pn.py (CPU) and
tests/test_supcon_pn_gpu.py:

  dense_loss    the definition: E = exp((S - m)(1 - I)) over the 2N stacked rows, log-probabilities, the two masked means
  closed_form   what the device evaluates: only m_i and Z_i come from the (2N)^2 matrix, the log E terms are
                linear in the features; with the three pieces of d loss / d features

and the seeded inputs both test files share."""
import functools

import torch


def masks(labels, thresh):
    """pos, un over the 2N rows (the labels stacked twice); a label equal to thresh is in neither"""
    al = torch.cat([labels.reshape(-1), labels.reshape(-1)])
    return al > thresh, al < thresh


def dense_loss(f, f_cr, labels, thresh, T):
    F = torch.cat([f, f_cr], 0)
    n2 = F.shape[0]
    S = F @ F.t() / T
    m = S.max(1, keepdim=True)[0].detach()
    E = torch.exp((S - m) * (1 - torch.eye(n2, dtype=F.dtype)))
    logp = torch.log(E) - torch.log(E.sum(1, keepdim=True))
    pos, un = masks(labels, thresh)
    pair = (torch.arange(n2) + n2 // 2) % n2
    pos_rows = (logp[pos][:, pos]).sum(1) / pos.sum()
    un_rows = logp[torch.arange(n2), pair][un]
    return -pos_rows.mean() - un_rows.mean()


def closed_form(f, f_cr, labels, thresh, T):
    """-> loss, (d/dF of the pos linear term, of the un pair term, of the log Z part), each (2N, dim)"""
    F = torch.cat([f, f_cr], 0).detach()
    n2 = F.shape[0]
    pos, un = masks(labels, thresh)
    P2, U = pos.sum().to(F.dtype), un.sum().to(F.dtype)
    pair = (torch.arange(n2) + n2 // 2) % n2
    S = F @ F.t() / T
    m = S.max(1)[0]
    E = torch.exp(S - m[:, None]) * (1 - torch.eye(n2, dtype=F.dtype))
    Z = E.sum(1) + 1                                              # the diagonal's exp(0)
    G = F[pos].sum(0)
    t_pos = ((F @ G) / T - (F * F).sum(1) / T - (P2 - 1) * m) / P2 - torch.log(Z)
    t_un = (F * F[pair]).sum(1) / T - m - torch.log(Z)
    loss = -t_pos[pos].sum() / P2 - t_un[un].sum() / U
    g_pos = torch.where(pos[:, None], -(2 * G[None] - 2 * F) / (T * P2 * P2), torch.zeros_like(F))
    g_un = torch.where(un[:, None], -2 * F[pair] / (T * U), torch.zeros_like(F))
    w = torch.where(pos, 1 / P2, torch.where(un, 1 / U, torch.zeros_like(P2)))
    W = (w / Z)[:, None] * E                                      # d loss / d Z_i x d Z_i / d S_ij, the maximum held constant
    g_z = (W + W.t()) @ F / T
    return loss, (g_pos, g_un, g_z)


@functools.lru_cache(maxsize=None)
def case_inputs(n, dim, thresh, kind, seed=0):
    """f, f_cr (n, dim) float32 unit rows and labels (n,) in [0, 1].  kind 'binary': a few 1s, the rest 0; 'mixed': also soft values
    on both sides of thresh and some labels exactly equal to it"""
    g = torch.Generator().manual_seed(1000 * n + 10 * dim + int(100 * thresh) + seed)
    f = torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=1)
    f_cr = torch.nn.functional.normalize(f + 0.3 * torch.randn(n, dim, generator=g), dim=1)
    lab = torch.zeros(n)
    order = torch.randperm(n, generator=g)
    k = max(2, n // 8)
    lab[order[:k]] = 1.0
    if kind == "mixed":
        lab[order[k:2 * k]] = float(thresh)
        lab[order[2 * k:3 * k]] = torch.rand(k, generator=g) * 0.98 + 0.01
    return f, f_cr, lab


@functools.lru_cache(maxsize=None)
def case_reference(n, dim, thresh, kind, T):
    """float64 dense loss and its gradient w.r.t. both views, computed once per case"""
    f, f_cr, lab = case_inputs(n, dim, thresh, kind)
    a, b = f.double().requires_grad_(), f_cr.double().requires_grad_()
    loss = dense_loss(a, b, lab, thresh, T)              # (labels stay float32: `lab > thresh` is decided in the labels' own type)
    loss.backward()
    return float(loss.detach()), a.grad.clone(), b.grad.clone()
