"""Pure-PyTorch oracles for every aggregation rule (test oracles + CPU/gloo path).

These are the *definitions* the HIP kernels in ``csrc/kernels`` are checked against
(SURVEY.md §4.4 item 1). Everything here runs on any device in float32/float64 and favours
clarity over speed. There is no reference implementation to mirror: the reference's only
"consensus" is set intersection of per-model feature sets (`scripts/model_walkthrough.ipynb:1939`,
`composite_code/rnotebook/cml_targetaml_seanalysis.Rmd:627-633`), which is the ``vote`` rule below.

Conventions (shared with the kernels):
  * ``X`` is worker-major ``[n, d]``.
  * Non-finite entries sort as +inf in coordinate rules; a worker whose squared norm is
    non-finite gets score +inf / weight 0 in Gram-space rules.
  * Median of an even count is the mean of the two middle values.
  * Gram-space rules return a weight vector ``w`` (sum 1); the aggregate is ``w @ X``.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

# --------------------------------------------------------------------------- coordinate rules


def _sanitize(X: torch.Tensor) -> torch.Tensor:
    X = X.float()
    return torch.where(torch.isnan(X), torch.full_like(X, float("inf")), X)


def mean(X: torch.Tensor) -> torch.Tensor:
    return X.float().mean(0)


def coord_median(X: torch.Tensor) -> torch.Tensor:
    S, _ = torch.sort(_sanitize(X), dim=0)
    n = S.shape[0]
    if n % 2:
        return S[n // 2]
    return 0.5 * (S[n // 2 - 1] + S[n // 2])


def trimmed_mean(X: torch.Tensor, b: int) -> torch.Tensor:
    n = X.shape[0]
    if 2 * b >= n:
        raise ValueError(f"trimmed_mean needs n > 2b (n={n}, b={b})")
    S, _ = torch.sort(_sanitize(X), dim=0)
    return S[b:n - b].mean(0)


def median_window(n: int) -> Tuple[int, int]:
    """Sorted-rank window [lo, lo+cnt) of the median of n values."""
    return ((n - 1) // 2, 1) if n % 2 else (n // 2 - 1, 2)


def mean_around(X: torch.Tensor, lo: int, cnt: int, keep: int) -> torch.Tensor:
    """Mean of the ``keep`` values nearest to a robust centre, per coordinate (MeaMed / Phocas).

    The n values are sanitised (NaN -> +inf) and sorted, s_0 <= ... <= s_{n-1}. The centre c is
    the mean of ranks [lo, lo+cnt); the result is the mean of ranks [j, j+keep) with
    j = #{i in [0, n-keep) : (s_{i+keep} - c) < (c - s_i)}, strictly: the keep values nearest to c,
    ties to the lower rank (the left side does not decrease with i and the right side does not
    increase, so the true predicates are a prefix). All in fp32: c is the rank-order sum times
    the fp32 1/cnt, the result the rank-order sum of the window times the fp32 1/keep.
    s_{i+keep} = +inf makes its predicate false and s_i = -inf makes it true, so with a finite
    centre and at most n-keep non-finite values no non-finite value reaches the result.
    keep == n is the plain mean."""
    S, _ = torch.sort(_sanitize(X), dim=0)
    n = S.shape[0]
    if not (0 <= lo and cnt >= 1 and lo + cnt <= n and 1 <= keep <= n):
        raise ValueError(f"mean_around: window ({lo}, {cnt}) / keep {keep} out of range for n={n}")
    one = torch.tensor(1.0, dtype=torch.float32)
    c = torch.zeros_like(S[0])
    for i in range(lo, lo + cnt):
        c = c + S[i]
    c = c * (one / cnt)
    j = torch.zeros(S.shape[1:], dtype=torch.long, device=S.device)
    for i in range(n - keep):
        j = j + ((S[i + keep] - c) < (c - S[i])).long()
    out = torch.zeros_like(S[0])
    for i in range(n):
        inside = (j <= i) & (i < j + keep)
        out = torch.where(inside, out + S[i], out)
    return out * (one / keep)


def meamed(X: torch.Tensor, f: int) -> torch.Tensor:
    """Mean around median (Xie, Koyejo, Gupta 2018): the n - f values nearest to the median."""
    n = X.shape[0]
    if 2 * f >= n:
        raise ValueError(f"meamed needs n > 2f (n={n}, f={f})")
    lo, cnt = median_window(n)
    return mean_around(X, lo, cnt, n - f)


def phocas(X: torch.Tensor, f: int, trim: Optional[int] = None) -> torch.Tensor:
    """Phocas (Xie, Koyejo, Gupta 2018): the n - f values nearest to the trimmed mean."""
    n = X.shape[0]
    b = f if trim is None else trim
    if 2 * f >= n or 2 * b >= n:
        raise ValueError(f"phocas needs n > 2f and n > 2 trim (n={n}, f={f}, trim={b})")
    return mean_around(X, b, n - 2 * b, n - f)


def vote(X: torch.Tensor, thresh: float = 0.0) -> torch.Tensor:
    """Coordinate-wise count of workers with |x| > thresh (ConsensusML's selection consensus:
    count == n is the n-way intersection of `model_walkthrough.ipynb:1939`)."""
    return (X.float().abs() > thresh).sum(0).float()


# --------------------------------------------------------------------------- Gram-space rules


def gram(X: torch.Tensor) -> torch.Tensor:
    Xd = X.double()
    return Xd @ Xd.t()


def sq_dists_from_gram(G: torch.Tensor) -> torch.Tensor:
    d = torch.diagonal(G)
    D = d[:, None] + d[None, :] - 2.0 * G
    return D.clamp_min(0.0)


def _bad_rows(G: torch.Tensor) -> torch.Tensor:
    return ~torch.isfinite(torch.diagonal(G))


def gram_center(G: torch.Tensor) -> int:
    """Medoid of the finite rows (csrc/kernels/gram.hip:gram_center_kernel)."""
    d = torch.diagonal(G)
    ok = torch.isfinite(d)
    D = (d[:, None] + d[None, :] - 2.0 * G).clamp_min(0.0)
    D = torch.where(ok[None, :], D, torch.zeros_like(D))
    s = D.sum(1)
    s = torch.where(ok & torch.isfinite(s), s, torch.full_like(s, float("inf")))
    if not bool(torch.isfinite(s).any()):
        return 0
    best = float(s.min())
    return int(torch.nonzero(s == best)[0, 0])


def krum_scores(G: torch.Tensor, f: int) -> torch.Tensor:
    """score_i = sum of the n-f-2 smallest squared distances from i to the others."""
    n = G.shape[0]
    bad = _bad_rows(G)
    D = sq_dists_from_gram(G)
    D = torch.where(bad[:, None] | bad[None, :], torch.full_like(D, float("inf")), D)
    D = torch.where(torch.isnan(D), torch.full_like(D, float("inf")), D)
    # k = n - f - 2 neighbours, floored at 1 so small pools (Bulyan's last rounds, n = 2f+2)
    # still rank by the nearest neighbour instead of degenerating to index order
    k = min(max(n - f - 2, 1), n - 1)
    scores = torch.zeros(n, dtype=torch.float64, device=G.device)
    for i in range(n):
        others = torch.cat([D[i, :i], D[i, i + 1:]])
        if k > 0:
            scores[i] = torch.sort(others).values[:k].sum()
    scores = torch.where(bad, torch.full_like(scores, float("inf")), scores)
    return scores


def krum_weights(G: torch.Tensor, f: int, m: int = 1) -> torch.Tensor:
    """Krum (m=1) / Multi-Krum (m>1): average of the m lowest-score workers (ties -> lower index)."""
    n = G.shape[0]
    s = krum_scores(G, f)
    idx = sorted(range(n), key=lambda i: (s[i].item(), i))[:m]
    w = torch.zeros(n, dtype=torch.float64, device=G.device)
    w[idx] = 1.0 / m
    return w


def weiszfeld_weights(G: torch.Tensor, iters: int = 8, eps: float = 1e-6,
                      tol: float = 0.0) -> torch.Tensor:
    """Smoothed Weiszfeld entirely in Gram space.

    z_t = sum_j a_j x_j, so ||x_i - z_t||^2 = G_ii - 2 (G a)_i + a^T G a. Each iteration
    sets b_i = 1 / max(||x_i - z_t||, eps), a <- b / sum(b). Starts from the mean.
    """
    n = G.shape[0]
    bad = _bad_rows(G)
    good = (~bad).double()
    Gs = torch.where(bad[:, None] | bad[None, :], torch.zeros_like(G), G)
    a = good / good.sum().clamp_min(1.0)
    for _ in range(iters):
        Ga = Gs @ a
        d2 = (torch.diagonal(Gs) - 2.0 * Ga + a @ Ga).clamp_min(0.0)
        b = good / torch.sqrt(d2).clamp_min(eps)
        a_new = b / b.sum()
        delta = (a_new - a).abs().max().item()
        a = a_new
        if tol > 0 and delta < tol:
            break
    return a


def geomed_direct(X: torch.Tensor, iters: int = 8, eps: float = 1e-6) -> torch.Tensor:
    """Weiszfeld on the raw vectors (independent oracle for the Gram-space version)."""
    Xd = X.double()
    z = Xd.mean(0)
    for _ in range(iters):
        d = torch.sqrt(((Xd - z) ** 2).sum(1)).clamp_min(eps)
        b = 1.0 / d
        z = (b[:, None] * Xd).sum(0) / b.sum()
    return z.float()


def centered_clip_weights(G_aug: torch.Tensor, tau: float, iters: int) -> torch.Tensor:
    """Centered clipping (Karimireddy et al. 2021) in Gram space.

    ``G_aug`` is the (n+1)x(n+1) Gram of [x_1..x_n, v0] where v0 is the previous aggregate.
    v <- v + (1/n) sum_i clip_tau(x_i - v), with v = sum_j c_j y_j over the n+1 rows.
    Workers with a non-finite squared norm are excluded (clip scale 0).
    Returns the n+1 coefficients c (the last multiplies v0).
    """
    n = G_aug.shape[0] - 1
    bad = _bad_rows(G_aug)
    bad[n] = False
    Gs = torch.where(bad[:, None] | bad[None, :], torch.zeros_like(G_aug), G_aug)
    c = torch.zeros(n + 1, dtype=torch.float64, device=G_aug.device)
    c[n] = 1.0
    for _ in range(iters):
        Gc = Gs @ c
        d2 = (torch.diagonal(Gs)[:n] - 2.0 * Gc[:n] + c @ Gc).clamp_min(0.0)
        d = torch.sqrt(d2)
        s = torch.clamp(tau / d.clamp_min(1e-30), max=1.0) / n   # clip scale per worker
        s = torch.where(bad[:n], torch.zeros_like(s), s)
        # v_new = v + sum_i s_i (x_i - v) = (1 - sum s) v + sum s_i x_i
        c_new = c * (1.0 - s.sum())
        c_new[:n] += s
        c = c_new
    return c


def bulyan_select(G: torch.Tensor, f: int) -> torch.Tensor:
    """Bulyan's selection phase: iterated Krum picks theta = n - 2f workers (indices, sorted)."""
    n = G.shape[0]
    theta = n - 2 * f
    remaining = list(range(n))
    chosen = []
    for _ in range(theta):
        sub = G[remaining][:, remaining]
        s = krum_scores(sub, f)
        j = min(range(len(remaining)), key=lambda i: (s[i].item(), i))
        chosen.append(remaining.pop(j))
    return torch.tensor(sorted(chosen), dtype=torch.long)


def bulyan(X: torch.Tensor, f: int) -> torch.Tensor:
    """Bulyan = Krum selection of n-2f workers, then coordinate trimmed mean (trim f)."""
    sel = bulyan_select(gram(X), f)
    return trimmed_mean(X[sel.to(X.device)], f)


def nnm_matrix(G: torch.Tensor, n: int, f: int) -> torch.Tensor:
    """Nearest-neighbour mixing (Allouah et al. 2023) from the Gram matrix: float64 [n, n],
    row-stochastic. Row i averages worker i with its nearest rows, k = n - f in all (itself
    included, ties -> lower index), by d_ij = max(G_ii + G_jj - 2 G_ij, 0) (NaN -> +inf).
    A row with a non-finite G_ii is bad: it is nobody's neighbour and keeps M_i = e_i, so the
    rules' own handling of non-finite rows applies to it unchanged. With fewer than k good rows
    every good row averages all of them. Only the leading n x n block of G is read."""
    G = G[:n, :n].double()
    d = torch.diagonal(G)
    bad = ~torch.isfinite(d)
    D = (d[:, None] + d[None, :] - 2.0 * G).clamp_min(0.0)
    D = torch.where(torch.isnan(D), torch.full_like(D, float("inf")), D)
    good = [j for j in range(n) if not bool(bad[j])]
    take = min(max(n - f, 1), len(good))
    M = torch.zeros(n, n, dtype=torch.float64, device=G.device)
    for i in range(n):
        if bool(bad[i]):
            M[i, i] = 1.0
            continue
        # i itself ranks first whatever duplicates of it exist
        order = sorted(good, key=lambda j: (-1.0 if j == i else D[i, j].item(), j))
        M[i, order[:take]] = 1.0 / take
    return M


def mix_rows(M: torch.Tensor, X: torch.Tensor, dtype: torch.dtype = torch.float64
             ) -> torch.Tensor:
    """Y = M X, summed in ``dtype`` and returned as fp32 rows. A zero entry of M contributes
    nothing even where X is NaN / inf (the weighted combine's convention); a non-finite x_j
    under a non-zero M_ij propagates as in IEEE arithmetic."""
    M = M.to(dtype)
    Xd = X.to(dtype)
    fin = torch.isfinite(Xd)
    Y = M @ torch.where(fin, Xd, torch.zeros_like(Xd))
    pos, neg = (M > 0).to(dtype), (M < 0).to(dtype)
    xp, xn = (Xd == float("inf")).to(dtype), (Xd == float("-inf")).to(dtype)
    pinf = (pos @ xp + neg @ xn) > 0
    ninf = (pos @ xn + neg @ xp) > 0
    nan = (((M != 0).to(dtype) @ torch.isnan(Xd).to(dtype)) > 0) | (pinf & ninf)
    Y = torch.where(pinf, torch.full_like(Y, float("inf")), Y)
    Y = torch.where(ninf, torch.full_like(Y, float("-inf")), Y)
    return torch.where(nan, torch.full_like(Y, float("nan")), Y).float()


def nnm_extend(M: torch.Tensor, rows: int) -> torch.Tensor:
    """M extended by the identity to ``rows`` rows (centered clipping's previous aggregate)."""
    n = M.shape[0]
    if rows == n:
        return M
    E = torch.eye(rows, dtype=M.dtype, device=M.device)
    E[:n, :n] = M
    return E


def nnm_gram(G: torch.Tensor, M: torch.Tensor) -> torch.Tensor:
    """Gram of the mixed rows Y = M X from the Gram of X: M G M^T for a mixing matrix whose rows
    are uniform on their support (``nnm_matrix``). Summed over each support in index order, as
    weights.hip does: mixed rows with the same neighbours (common with NNM -- a tight cluster
    mixes to one point) then get bit-identical Gram rows, so their scores tie exactly and the
    rules' lower-index tie-break decides, on every device alike. A zero entry contributes
    nothing, so a bad row's non-finite entries stay in its own row and column."""
    G = G.double()
    r = G.shape[0]
    sup = [torch.nonzero(M[i]).flatten().tolist() for i in range(r)]
    inv = [1.0 / len(s) for s in sup]
    T = torch.zeros_like(G)          # T = G M^T
    for j in range(r):
        acc = torch.zeros(r, dtype=torch.float64, device=G.device)
        for b in sup[j]:
            acc = acc + G[:, b]
        T[:, j] = acc * inv[j]
    Gm = torch.zeros_like(G)         # G' = M T
    for i in range(r):
        acc = torch.zeros(r, dtype=torch.float64, device=G.device)
        for a in sup[i]:
            acc = acc + T[a, :]
        Gm[i, :] = acc * inv[i]
    return Gm


# --------------------------------------------------------------------------- full rules


def aggregate(X: torch.Tensor, rule: str, f: int = 0, trim: Optional[int] = None,
              m: Optional[int] = None, iters: int = 8, eps: float = 1e-6,
              tau: float = 10.0, clip_iters: int = 3,
              v0: Optional[torch.Tensor] = None, pre: str = "none") -> torch.Tensor:
    n = X.shape[0]
    if pre == "nnm":
        # the rule on the mixed rows Y = M X (the previous aggregate of centered clipping is
        # not a worker row and stays unmixed)
        if rule in ("mean", "bulyan"):
            raise ValueError(f"pre='nnm' is not defined for rule {rule!r}")
        X = mix_rows(nnm_matrix(gram(X), n, f), X)
    elif pre != "none":
        raise ValueError(f"unknown pre-aggregation {pre!r}")
    if rule == "mean":
        return mean(X)
    if rule == "median":
        return coord_median(X)
    if rule == "trimmed_mean":
        return trimmed_mean(X, f if trim is None else trim)
    if rule == "meamed":
        return meamed(X, f)
    if rule == "phocas":
        return phocas(X, f, trim)
    if rule == "krum":
        w = krum_weights(gram(X), f, 1)
        return (w.float() @ _zero_bad(X)).float()
    if rule == "multi_krum":
        w = krum_weights(gram(X), f, m if m is not None else n - f)
        return (w.float() @ _zero_bad(X)).float()
    if rule == "geomed":
        w = weiszfeld_weights(gram(X), iters, eps)
        return (w.float() @ _zero_bad(X)).float()
    if rule == "bulyan":
        return bulyan(X, f)
    if rule == "centered_clip":
        v0 = torch.zeros(X.shape[1], device=X.device) if v0 is None else v0
        Y = torch.cat([X.float(), v0.float()[None]], 0)
        c = centered_clip_weights(gram(Y), tau, clip_iters)
        return (c.float() @ _zero_bad(Y)).float()
    raise ValueError(f"unknown rule {rule!r}")


def _zero_bad(X: torch.Tensor) -> torch.Tensor:
    X = X.float()
    ok = torch.isfinite(X).all(1, keepdim=True)
    return torch.where(ok, X, torch.zeros_like(X))


# --------------------------------------------------------------------------- optimizers


def sgd_update(p: torch.Tensor, g: torch.Tensor, buf: torch.Tensor, lr: float, momentum: float,
               weight_decay: float = 0.0, nesterov: bool = False, first: bool = False
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """torch.optim.SGD semantics on fp32 master ``p`` and momentum ``buf`` (returns new copies)."""
    g = g.float()
    if weight_decay:
        g = g + weight_decay * p
    if momentum:
        buf = g.clone() if first else momentum * buf + g
        g = g + momentum * buf if nesterov else buf
    return p - lr * g, buf


def adam_update(p, g, m, v, step: int, lr: float, beta1: float, beta2: float, eps: float,
                weight_decay: float = 0.0, decoupled: bool = True):
    g = g.float()
    if weight_decay and not decoupled:
        g = g + weight_decay * p
    if weight_decay and decoupled:
        p = p * (1.0 - lr * weight_decay)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (v / bc2).sqrt() + eps
    p = p - (lr / bc1) * m / denom
    return p, m, v


def _clipped_delta(d: torch.Tensor, clip: float) -> torch.Tensor:
    """c d with c = min(1, clip / ||d||); exactly zero at every coordinate where the fp32 squared
    distance is not finite (a NaN, an Inf or an overflowing sum: the neighbour is dropped)."""
    s = (d * d).sum().item()
    if not math.isfinite(s):
        return torch.zeros_like(d)
    return d * min(1.0, clip / max(math.sqrt(s), 1e-30))


def gossip_mix(x: torch.Tensor, left: torch.Tensor, right: torch.Tensor, w0: float, w1: float,
               w2: float, clip: float = 0.0) -> torch.Tensor:
    """The ring (k = 2) form of ``gossip_mix_k``, with the same rule for non-finite neighbours."""
    x = x.float()
    dl = left.float() - x
    dr = right.float() - x
    if clip > 0:
        dl = _clipped_delta(dl, clip)
        dr = _clipped_delta(dr, clip)
    # w0 x + w1 (x + dl) + w2 (x + dr)
    return (w0 + w1 + w2) * x + w1 * dl + w2 * dr


def gossip_mix_k(x: torch.Tensor, nbrs, w, w0: float, clip: float = 0.0) -> torch.Tensor:
    """x <- (w0 + sum w_k) x + sum_k w_k c_k (nb_k - x), c_k = min(1, clip / ||nb_k - x||).

    With clip > 0 a neighbour whose squared distance (summed in fp32) is not finite -- it holds a
    NaN or an Inf, or the sum overflows -- has c_k = 0: its term is exactly zero at every
    coordinate and its weight stays with x. A non-finite x drops every neighbour. clip == 0
    gives no protection: a NaN propagates."""
    x = x.float()
    out = (w0 + sum(w)) * x
    for nb, wk in zip(nbrs, w):
        d = nb.float() - x
        if clip > 0:
            d = _clipped_delta(d, clip)
        out = out + wk * d
    return out


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def is_pow2(n: int) -> bool:
    return n > 0 and (n & (n - 1)) == 0


# --------------------------------------------------------------------------- worker momentum


def worker_momentum(rows: torch.Tensor, mom: torch.Tensor, beta: float) -> None:
    """Worker-side momentum in place: mom <- beta * mom + rows (fp32), rows <- mom rounded to the
    rows' dtype (``optim.worker_momentum``; the definition of csrc/kernels/worker_momentum.hip)."""
    mom.mul_(beta).add_(rows.float())
    rows.copy_(mom.to(rows.dtype))


# --------------------------------------------------------------------------- global-norm clipping

CLIP_STATS = 4   # [norm, coef, count of non-finite norms, squared norm] (fp64)


def sq_norm(segments, scale: float = 1.0) -> torch.Tensor:
    """fp64 scalar: sum over every element x of every segment of (float(x) * scale)^2. The product
    is rounded to fp32 (what the update's fp32 multiply gives), the square and the sum are fp64
    (the definition of ``sq_norm_partial``, csrc/kernels/clip_norm.hip)."""
    sc = torch.tensor(scale, dtype=torch.float32)
    tot = torch.zeros((), dtype=torch.float64)
    for s in segments:
        v = (s.detach().reshape(-1).float().cpu() * sc).double()
        tot = tot + (v * v).sum()
    return tot


def clip_coef(norm2: torch.Tensor, max_norm: float, base: float = 1.0):
    """(w, norm, coef, bad) of global-norm clipping from the squared norm (fp64 arithmetic):
    norm = sqrt(norm2), coef = min(1, max_norm / (norm + 1e-6)) -- the arithmetic of
    ``torch.nn.utils.clip_grad_norm_`` -- and w = fp32(fp32(base) * coef), the weight the update
    multiplies the gradient by. A non-finite norm2 gives coef = 0 and bad = 1 (a zero gradient
    instead of a poisoned state; ``clip_finalize``, csrc/kernels/clip_norm.hip)."""
    s = norm2.detach().double().reshape(-1)[0].cpu()
    ok = bool(torch.isfinite(s)) and float(s) >= 0.0
    norm = s.sqrt() if ok else s
    coef = torch.zeros((), dtype=torch.float64)
    if ok:
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    w = (torch.tensor(base, dtype=torch.float32).double() * coef).float()
    return w, norm, coef, int(not ok)


# --------------------------------------------------------------------------- LARS

LARS_STATS = 4   # per tensor: [wn, gn, q, count of steps with a non-finite norm] (fp64)


def seg_sq_norm(master: torch.Tensor, g: torch.Tensor, scale: float, starts, numels
                ) -> torch.Tensor:
    """fp64 [T, 2]: per tensor t over exactly its elements [starts[t], starts[t] + numels[t]) of
    the state vector, (sum p^2, sum (float(x) * scale)^2) with p the fp32 master and x the
    co-indexed gradient row. The product is rounded to fp32 as ``sq_norm`` defines it, squares and
    sums are fp64 (the definition of ``seg_sq_norm_partial``, csrc/kernels/lars.hip). Alignment
    padding between tensors never enters a norm."""
    sc = torch.tensor(scale, dtype=torch.float32)
    p = master.detach().reshape(-1).cpu()
    x = g.detach().reshape(-1).cpu()
    out = torch.zeros(len(numels), 2, dtype=torch.float64)
    for t, (s, n) in enumerate(zip(starts, numels)):
        pw = p[s:s + n].double()
        gv = (x[s:s + n].float() * sc).double()
        out[t, 0] = (pw * pw).sum()
        out[t, 1] = (gv * gv).sum()
    return out


def lars_ratio(pairs: torch.Tensor, adapt, trust: float, weight_decay: float, eps: float):
    """(q fp32 [T], stats fp64 [T, 3] = (wn, gn, q), bad int64 [T]) of LARS from pairs[t] = (sw,
    sg) = (sum p^2, sum g^2), all in fp64 (``lars_finalize``, csrc/kernels/lars.hip):

      sw or sg not finite              q = 0 and bad = 1: the tensor takes a zero gradient
      adapt[t], wn > 0 and gn > 0      q = fp32(trust * wn / (gn + weight_decay * wn + eps))
      otherwise                        q = 1
    with wn = sqrt(sw), gn = sqrt(sg) (a non-finite sum is reported as it is)."""
    pr = pairs.detach().double().cpu().reshape(-1, 2)
    T = pr.shape[0]
    fin = torch.isfinite(pr) & (pr >= 0)
    nrm = torch.where(fin, pr.clamp_min(0).sqrt(), pr)
    wn, gn = nrm[:, 0], nrm[:, 1]
    ok = fin.all(1)
    ad = torch.as_tensor(adapt, dtype=torch.bool).reshape(T)
    ratio = trust * wn / (gn + weight_decay * wn + eps)
    q = torch.ones(T, dtype=torch.float64)
    q = torch.where(ok & ad & (wn > 0) & (gn > 0), ratio, q)
    q = torch.where(ok, q, torch.zeros_like(q)).float()
    return q, torch.stack([wn, gn, q.double()], 1), (~ok).long()


def lars_update(p: torch.Tensor, g: torch.Tensor, buf: Optional[torch.Tensor], q: torch.Tensor,
                starts, scale: float, lr: float, momentum: float, weight_decay: float = 0.0,
                nesterov: bool = False, first: bool = False
                ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The LARS step over a whole state vector (returns new copies of master and buffer): per
    element of tensor t, g = float(x) * scale; g += weight_decay * p; g = q[t] * g -- exactly 0
    where q[t] == 0, so a NaN gradient poisons no state -- then ``sgd_update``'s momentum,
    Nesterov and p - lr * g. ``starts``: T + 1 ascending starts, starts[T] = the vector length;
    an element belongs to the last tensor whose start is not behind it, so padding takes the
    preceding tensor's q (``lars_update``, csrc/kernels/lars.hip)."""
    D = int(starts[-1])
    spans = torch.as_tensor([starts[t + 1] - starts[t] for t in range(len(starts) - 1)])
    spans[0] += starts[0]
    qe = torch.repeat_interleave(q.detach().float().cpu(), spans)
    p = p[:D].float()
    gv = g[:D].float() * torch.tensor(scale, dtype=torch.float32)
    if weight_decay:
        gv = gv + weight_decay * p
    gv = torch.where(qe == 0, torch.zeros_like(gv), qe * gv)
    return sgd_update(p, gv, buf[:D] if buf is not None else None, lr, momentum, 0.0, nesterov,
                      first)


__all__ = [n for n in dir() if not n.startswith("_") and n not in ("math", "torch", "Optional",
                                                                     "Tuple", "annotations")]
