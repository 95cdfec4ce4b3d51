"""The spectral start of the UMAP map on the MI355X (csrc/spectral.hip): what umap-learn's init="spectral" computes,
the eigenvectors 1..dim of the normalised Laplacian L = I - D^-1/2 W D^-1/2 of the fuzzy graph, component by component.

    Y, info = spectral_layout(index, wsym, eps, mutual, rev_ptr, rev_edge, dim=2, seed=42, tol=1e-6)

The graph is the one the epochs walk (utils/umap.UMAP.setup): forward edges and lone reverse edges with finite eps, weight wsym.
  components   min-label propagation with pointer jumping, one launch per sweep (hipops.graph_components); the vertices are then
               renumbered by (label, id) with torch so that every component is a contiguous row range, and numbered back at the end.
  eigenpairs   per component of n_c >= max(2 dim, dim + 2) vertices: the dim largest eigenpairs of A = D^-1/2 W D^-1/2 below the
               known top pair theta = 1, q0 = sqrt(deg) / |sqrt(deg)|, by thick-restart Lanczos.  q0 is never solved for: it is
               row 0 of the basis every new vector is orthogonalised against, twice (full re-orthogonalisation, hipops.spectral_orth).
               The projected matrix is assembled from those coefficients and solved on the host (numpy.linalg.eigh, float64); a
               restart keeps the best dim + 3 Ritz vectors (hipops.spectral_combine) and the residual direction.  Basis:
               max(2 dim + 1, ceil(sqrt(n_c))) vectors, umap-learn's count (never fewer than dim + 2, never more than n_c - 1).
               Start vector: numpy.random.RandomState(seed).standard_normal(n_c), deflated.  Converged: |A v - theta v|_2 <= tol for
               every wanted pair, the TRUE residual (one more product per pair at every restart), not the Lanczos estimate.
               RESTART CAP: max_restarts = 300 by default; past it the layout reports converged = False.
  sign, order  every eigenvector is turned so that its entry of largest magnitude is positive (ties: the lowest vertex id); the
               axes are in ascending eigenvalue of L.
  placement    one component: the eigenvectors as they are.  Several (umap-learn's multi_component_layout): centres for
               c <= 2 dim components the rows of vstack([base, -base])[:c], base = hstack([eye(ceil(c / 2)), zeros]); for more, the
               centroids of the components in data space (x), the affinity exp(-d^2) of their pairwise distances (diagonal
               included) and the eigenvectors 1..dim of its normalised Laplacian by numpy.linalg.eigh, the sign rule, divided by the
               largest magnitude - umap-learn runs sklearn's SpectralEmbedding there; the dense form is stated instead.  More than
               256 components: converged = False.  data_range of a component is half the distance from its centre to the nearest
               other one; a large component's eigenvectors are scaled by data_range / max|v| and moved to the centre, a small one
               gets RandomState(seed).uniform(-data_range, data_range) around it, one generator drawn from in ascending label.
  centroids    sums over each component's contiguous rows (a fixed order; an index_add_ on the device adds with atomics).
No norm, dot product or basis product goes through a torch reduction or rocBLAS: the layout is the same bytes from run to run.
info: converged, n_components, labels (N,) int64, sizes, centres, data_range, scale, eigenvalues (those of the largest component,
ascending, of L), residuals, steps, restarts, sweeps, basis.  Nothing is raised on non-convergence: the caller falls back.
"""
import math

import numpy as np
import torch

from .. import hipops as H
from .graph import reverse_graph

MAX_COMPONENTS = 256
MAX_RESTARTS = 300
KEEP_EXTRA = 3
BREAKDOWN = 1e-12            # |A| <= 1: a new direction shorter than this is rounding noise


def basis_size(n_c, dim, max_basis=None):
    m = max(2 * dim + 1, int(math.ceil(math.sqrt(n_c)))) if max_basis is None else int(max_basis)
    return min(max(m, dim + 2), n_c - 1)


def fixed_centres(c, dim):
    k = int(np.ceil(c / 2.0))
    base = np.hstack([np.eye(k), np.zeros((k, dim - k))])
    return np.vstack([base, -base])[:c]


def eigh_centres(centroids, dim):
    """The eigenvectors 1..dim of the normalised Laplacian of exp(-d^2) over the centroids, signed and scaled to max |.| = 1."""
    z = np.asarray(centroids, np.float64)
    d2 = ((z[:, None, :] - z[None, :, :]) ** 2).sum(2)
    aff = np.exp(-d2)
    dis = 1.0 / np.sqrt(aff.sum(1))
    lap = np.eye(len(z)) - aff * dis[:, None] * dis[None, :]
    e = np.linalg.eigh(lap)[1][:, 1:dim + 1].copy()
    for a in range(dim):
        if e[np.argmax(np.abs(e[:, a])), a] < 0:
            e[:, a] = -e[:, a]
    return e / np.abs(e).max()


def data_ranges(centres):
    d = np.sqrt(((centres[:, None, :] - centres[None, :, :]) ** 2).sum(2))
    np.fill_diagonal(d, np.inf)
    return d.min(1) / 2.0


def _norm(v):
    return math.sqrt(float(H.spectral_dots(v[None], v).item()))


def _sign(v):
    a = v.abs()
    first = int((a == a.max()).nonzero()[0])
    if float(v[first]) < 0:
        v.neg_()


def _solve(g, deg, dis, row0, n_c, dim, seed, tol, max_basis, max_restarts):
    """The dim largest eigenpairs of A on the rows [row0, row0 + n_c) below (1, q0): theta (dim,) descending, vectors (dim, n_c)
    on the device, and the counts."""
    dev = dis.device
    mmax = basis_size(n_c, dim, max_basis)
    V = torch.zeros(mmax + 2, n_c, dtype=torch.float64, device=dev)       # q0, then v_0 .. v_mmax
    w, r = torch.empty(n_c, dtype=torch.float64, device=dev), torch.empty(n_c, dtype=torch.float64, device=dev)
    c1, c2 = torch.empty(mmax + 2, dtype=torch.float64, device=dev), torch.empty(mmax + 2, dtype=torch.float64, device=dev)
    q0 = torch.sqrt(deg[row0:row0 + n_c])
    V[0] = q0 / _norm(q0)
    rs = np.random.RandomState(seed % 2 ** 32)

    def fresh(nv):
        """a random direction orthogonal to the first nv rows of V, in w; its length before it is normalised"""
        w.copy_(torch.from_numpy(rs.standard_normal(n_c)).to(dev))
        length = _norm(w)
        for _ in range(2):
            H.spectral_orth(V[:nv], w, c1[:nv])
        left = _norm(w)
        if left <= 1e-8 * length:
            return 0.0
        w.mul_(1.0 / left)
        return left

    fresh(1)
    V[1] = w
    T = np.zeros((mmax, mmax))
    done, steps, restarts, exhausted = 0, 0, 0, False
    while True:
        m, last_beta = mmax, 0.0
        for j in range(done, mmax):
            H.spectral_spmv(*g, dis, V[1 + j], w, row0=row0)
            steps += 1
            H.spectral_orth(V[:j + 2], w, c1[:j + 2])
            H.spectral_orth(V[:j + 2], w, c2[:j + 2])
            c = (c1[1:j + 2] + c2[1:j + 2]).cpu().numpy()
            T[:j + 1, j], T[j, :j + 1] = c, c
            beta = _norm(w)
            if beta > BREAKDOWN:
                w.mul_(1.0 / beta)
            else:                                  # an invariant subspace: go on from a fresh direction, if one is left
                beta = 0.0
                if fresh(j + 2) == 0.0:
                    m, exhausted = j + 1, True
                    break
            V[2 + j] = w
            if j + 1 < mmax:
                T[j + 1, j] = T[j, j + 1] = beta
            last_beta = beta
        theta, S = np.linalg.eigh(T[:m, :m])
        order = np.argsort(theta)[::-1]
        want = order[:dim]
        vecs = torch.empty(len(want), n_c, dtype=torch.float64, device=dev)
        res = []
        for a, i in enumerate(want):
            H.spectral_combine(V[1:1 + m], torch.from_numpy(-S[:, i].copy()).to(dev), vecs[a])
            H.spectral_spmv(*g, dis, vecs[a], r, row0=row0)
            r.add_(vecs[a], alpha=-float(theta[i]))
            res.append(_norm(r))
        converged = len(want) == dim and max(res) <= tol
        if converged or exhausted or restarts >= max_restarts:
            return dict(theta=theta[want], vectors=vecs, residuals=np.array(res), converged=converged, steps=steps,
                        restarts=restarts, basis=mmax)
        keep = min(max(dim, min(dim + KEEP_EXTRA, mmax - 2)), m - 1)
        kept = order[:keep]
        Y = torch.empty(keep, n_c, dtype=torch.float64, device=dev)
        for a, i in enumerate(kept):
            H.spectral_combine(V[1:1 + m], torch.from_numpy(-S[:, i].copy()).to(dev), Y[a])
        residual = V[1 + m].clone()
        V[1:1 + keep] = Y
        V[1 + keep] = residual
        T[:] = 0.0
        T[np.arange(keep), np.arange(keep)] = theta[kept]
        T[:keep, keep] = T[keep, :keep] = last_beta * S[m - 1, kept]
        done, restarts = keep, restarts + 1


def spectral_layout(index, wsym, eps, mutual, rev_ptr, rev_edge, dim=2, seed=42, tol=1e-6, max_basis=None, max_restarts=None, x=None):
    """(Y (N, dim) float64 on the device, info).  x (N, d) on the device: the data, needed only for the centres of more than
    2 dim components.  max_restarts: the restart cap, 300 unless given."""
    n, k = index.shape
    dev = index.device
    max_restarts = MAX_RESTARTS if max_restarts is None else int(max_restarts)
    label, sweeps = H.graph_components(index, eps, mutual, rev_ptr, rev_edge)
    lab = label.long()
    perm = torch.sort(lab * n + torch.arange(n, device=dev))[1]             # perm[new] = old, by (label, id)
    uniq, counts = torch.unique_consecutive(lab[perm], return_counts=True)
    sizes = counts.cpu().numpy().astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    c = len(sizes)
    info = dict(converged=False, n_components=c, labels=lab.cpu().numpy(), sizes=sizes, sweeps=sweeps, centres=None, data_range=None,
                scale=None, eigenvalues=None, residuals=None, steps=0, restarts=0, basis=None)
    Y = torch.zeros(n, dim, dtype=torch.float64, device=dev)
    if c > MAX_COMPONENTS:
        return Y, info
    if c > 1:
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(n, device=dev)
        index = inv[index[perm].long()].to(torch.int32).contiguous()
        wsym, eps, mutual = wsym[perm].contiguous(), eps[perm].contiguous(), mutual[perm].contiguous()
        rev_ptr, rev_edge = reverse_graph(index)
    g = (index, wsym, eps, mutual, rev_ptr, rev_edge)
    deg, dis = H.spectral_degree(*g)
    if c == 1:
        centres, ranges = np.zeros((1, dim)), np.array([np.inf])
    else:
        if c <= 2 * dim:
            centres = fixed_centres(c, dim)
        else:
            if x is None:
                raise ValueError("%d graph components: their centres are placed by the data's centroids, and x was not given" % c)
            xs = x.reshape(n, -1)[perm].double()
            centres = eigh_centres(np.stack([(xs[s:s + m].sum(0) / float(m)).cpu().numpy() for s, m in zip(starts, sizes)]), dim)
        ranges = data_ranges(centres)
    rs = np.random.RandomState(seed % 2 ** 32)
    large = max(2 * dim, dim + 2)
    biggest = int(np.argmax(sizes))
    Yn = torch.zeros(n, dim, dtype=torch.float64, device=dev)
    scale, ok = np.ones(c), True
    for a in range(c):
        s, m = int(starts[a]), int(sizes[a])
        if m < large:
            Yn[s:s + m] = torch.from_numpy(rs.uniform(-ranges[a], ranges[a], (m, dim)) + centres[a]).to(dev)
            continue
        sol = _solve(g, deg, dis, s, m, dim, seed, tol, max_basis, max_restarts)
        info["steps"] += sol["steps"]
        info["restarts"] += sol["restarts"]
        ok = ok and sol["converged"]
        if a == biggest:
            info["eigenvalues"], info["residuals"], info["basis"] = 1.0 - sol["theta"], sol["residuals"], sol["basis"]
        vec = sol["vectors"]
        for v in vec:
            _sign(v)
        if c > 1:
            scale[a] = ranges[a] / float(vec.abs().max())
            vec = vec * scale[a] + torch.from_numpy(centres[a]).to(dev)[:, None]
        Yn[s:s + m] = vec.t()
    Y[perm] = Yn
    info.update(converged=bool(ok), centres=centres, data_range=ranges, scale=scale)
    return Y, info


def umap_start(Y, seed):
    """umap-learn's simplicial_set_embedding on a spectral layout Y (N, dim) float64 numpy: Y 10 / max|Y| as fp32, plus
    RandomState(seed).normal(scale=1e-4) as fp32, then per axis 10 (y - min) / (max - min) as fp32."""
    Y = np.asarray(Y, np.float64)
    y = (Y * (10.0 / np.abs(Y).max())).astype(np.float32)
    y = y + np.random.RandomState(seed % 2 ** 32).normal(scale=1e-4, size=Y.shape).astype(np.float32)
    return (10.0 * (y - y.min(0)) / (y.max(0) - y.min(0))).astype(np.float32)
