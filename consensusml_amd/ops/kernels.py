"""Device-dispatching wrappers of the aggregation / optimizer / gossip kernels.

GPU tensors -> HIP kernels of ``csrc/kernels`` (via ``_C``); CPU tensors -> the oracles of
``ops.reference`` (used by the gloo plumbing config and the CPU tests). Worker matrices are
``[n, D]`` worker-major with unit column stride (row stride free, so views into all-gather /
all-to-all receive buffers need no copy).
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from ..config import COORD_RULES
from . import reference as ref
from .native import lib

RULE_IDS = {"mean": 0, "krum": 1, "multi_krum": 2, "geomed": 3, "centered_clip": 4,
            "bulyan_select": 5, "nnm_only": 6}
PRE_IDS = {"none": 0, "nnm": 1}
WEIGHT_RULES = ("krum", "multi_krum", "geomed", "centered_clip")   # weights: robust_weights
GOSSIP_MAX_NBRS = 8   # neighbour buffers one gossip_mix_k launch reads (kMaxNbrs, gossip_fault.hip)


def sorted_range(rule: str, n: int, trim: int = 0) -> Tuple[int, int]:
    """Sorted-rank window [lo, lo+cnt) averaged by a coordinate rule over n values."""
    if rule == "median":
        return ((n - 1) // 2, 1) if n % 2 else (n // 2 - 1, 2)
    if rule == "trimmed_mean":
        if 2 * trim >= n:
            raise ValueError(f"trimmed_mean needs n > 2*trim (n={n}, trim={trim})")
        return trim, n - 2 * trim
    if rule == "mean":
        return 0, n
    raise ValueError(rule)


def near_range(rule: str, n: int, f: int, trim: Optional[int] = None) -> Tuple[int, int, int]:
    """(lo, cnt, keep) of a coordinate rule: the centre is the mean of sorted ranks [lo, lo+cnt)
    and the rule averages the ``keep`` values nearest to it (``reference.mean_around``).
    keep == 0: the plain window rules (median, trimmed_mean), whose result is the centre."""
    if rule in ("meamed", "phocas"):
        if 2 * f >= n:
            raise ValueError(f"{rule} needs n > 2f (n={n}, f={f})")
        if rule == "meamed":
            return (*sorted_range("median", n), n - f)
        b = f if trim is None else trim
        if 2 * b >= n:
            raise ValueError(f"phocas needs n > 2*trim (n={n}, trim={b})")
        return b, n - 2 * b, n - f
    return (*sorted_range(rule, n, f if trim is None else trim), 0)


@dataclass(frozen=True)
class Combine:
    """The keyword arguments of ``agg_update`` / ``agg_update_multi`` that a rule fixes."""
    combine: str
    n: int
    lo: int = 0
    cnt: int = 1
    keep: Optional[int] = None
    w: Optional[torch.Tensor] = None
    rows: Optional[torch.Tensor] = None
    mix: Optional[torch.Tensor] = None

    def kwargs(self) -> dict:
        return dict(vars(self))


def rule_combine(rule: str, n: int, f: int, trim: Optional[int] = None, *,
                 w: Optional[torch.Tensor] = None, sel: Optional[torch.Tensor] = None,
                 mix: Optional[torch.Tensor] = None, rows_total: Optional[int] = None) -> Combine:
    """How ``rule`` over n workers combines the rows -- the whole table:

    coordinate rules  sorted, ``near_range(rule, n, f, trim)``, pre-mixed by ``mix`` if given
    bulyan            sorted: the f-trimmed mean of the n - 2f rows ``sel`` holds (Bulyan's
                      selection, ``robust_weights`` rule ``'bulyan_select'``)
    everything else   (mean, Gram-space rules) weighted by ``w`` over ``rows_total`` or n rows
    """
    if rule in COORD_RULES:
        lo, cnt, keep = near_range(rule, n, f, trim)
        return Combine("sorted", n, lo, cnt, keep, mix=mix)
    if rule == "bulyan":
        theta = n - 2 * f
        lo, cnt = sorted_range("trimmed_mean", theta, f)
        return Combine("sorted", theta, lo, cnt, rows=sel[:theta])
    if rule != "mean" and rule not in WEIGHT_RULES:
        raise ValueError(f"unknown rule {rule!r}")
    return Combine("weighted", rows_total or n, w=w)


@dataclass
class OptArgs:
    """Hyper-parameters of one fused optimizer step (SGD or Adam/AdamW), or of the LARS step
    (``lars_update``: SGD's fields; the trust coefficient and the ratio's eps go to ``lars_ratio``,
    so this class keeps the fields the recorded engine traces list)."""
    kind: str = "sgd"            # none | sgd | adam (L2 weight decay) | adamw (decoupled) | lars
    lr: float = 0.1
    momentum: float = 0.0
    weight_decay: float = 0.0
    nesterov: bool = False
    first: bool = False          # first SGD step: momentum buffer <- g
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    step: int = 1                # Adam step (1-based) for bias correction
    gscale: float = 1.0

    def opt_id(self) -> int:
        if self.kind == "lars":
            raise ValueError("OptArgs(kind='lars') is the step of lars_update, not of agg_update")
        return {"none": 0, "sgd": 1, "adamw": 2, "adam": 3 if self.weight_decay else 2}[self.kind]


def _as2d(X: torch.Tensor) -> torch.Tensor:
    if X.dim() == 1:
        X = X[None]
    assert X.dim() == 2 and X.stride(1) == 1, "worker matrix must be [n, D] with unit column stride"
    return X


# --------------------------------------------------------------------------- fused update
def agg_update(X: torch.Tensor, *, combine: str, lo: int = 0, cnt: int = 1,
               w: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None,
               n: Optional[int] = None, D: Optional[int] = None, opt: Optional[OptArgs] = None,
               master: Optional[torch.Tensor] = None, s1: Optional[torch.Tensor] = None,
               s2: Optional[torch.Tensor] = None, param_out: Optional[torch.Tensor] = None,
               gout: Optional[torch.Tensor] = None,
               mix: Optional[torch.Tensor] = None, keep: Optional[int] = None) -> None:
    """Aggregate worker rows and apply the optimizer in one pass (in place on the state).

    combine='sorted'   mean of sorted ranks [lo, lo+cnt) per coordinate
    combine='weighted' sum_i w_i x_i (w None -> all ones)
    mix                sorted combine only: fp32 [n, n] on X's device, a linear pre-mix of the
                       rows per coordinate, y_i = sum_j mix[i, j] x_j in fp32, before the sort
                       (n <= 32). A zero entry contributes nothing even where x_j is NaN / inf.
    keep               sorted combine only: [lo, lo+cnt) is the centre's window and the result is
                       the mean of the ``keep`` sorted values nearest to the centre
                       (``reference.mean_around``; n / 2 <= keep <= n). None / 0: the plain window.
    """
    X = _as2d(X)
    n = n if n is not None else (rows.numel() if rows is not None else X.shape[0])
    D = D if D is not None else X.shape[1]
    opt = opt or OptArgs(kind="none")
    _check_mix(mix, combine, n)
    keep = _check_keep(keep, combine, n)
    if X.is_cuda:
        head, tail = _binding_args(rows, combine, lo, cnt, w, opt, master, s1, s2, gout, mix, keep)
        lib().agg_update(X, n, D, *head, param_out, *tail)
        return
    # ---- CPU reference path
    Xr = X[rows.long()] if rows is not None else X[:n]
    Xr = Xr[:, :D].float()
    if combine == "sorted":
        if mix is not None:
            Xr = ref.mix_rows(mix[:n, :n].float().cpu(), Xr, torch.float32)
        if keep:
            g = ref.mean_around(Xr, lo, cnt, keep)
        else:
            S, _ = torch.sort(ref._sanitize(Xr), dim=0)
            g = S[lo:lo + cnt].mean(0)
    else:
        ww = torch.ones(n) if w is None else w[:n].float().cpu()
        nz = (ww != 0).nonzero().flatten()
        g = (ww[nz, None] * Xr[nz]).sum(0) if nz.numel() else torch.zeros(D)
    g = g * opt.gscale
    if gout is not None:
        gout[:D].copy_(g)
    k = opt.opt_id()
    if k == 0:
        return
    if k == 1:
        p, b = ref.sgd_update(master[:D], g, s1[:D] if s1 is not None else None, opt.lr,
                              opt.momentum, opt.weight_decay, opt.nesterov, opt.first)
        master[:D].copy_(p)
        if opt.momentum:
            s1[:D].copy_(b)
    else:
        p, m, v = ref.adam_update(master[:D], g, s1[:D], s2[:D], opt.step, opt.lr, opt.beta1,
                                  opt.beta2, opt.eps, opt.weight_decay, decoupled=(k == 2))
        master[:D].copy_(p)
        s1[:D].copy_(m)
        s2[:D].copy_(v)
    if param_out is not None:
        param_out[:D].copy_(master[:D].to(param_out.dtype))


def _binding_args(rows, combine, lo, cnt, w, opt, master, s1, s2, gout, mix, keep):
    """What ``lib().agg_update`` and ``lib().agg_update_multi`` both take: the arguments from
    ``rows`` to ``s2`` and, after the single form's ``param_out``, those from ``gout`` on."""
    bc1 = 1.0 - opt.beta1 ** opt.step
    bc2 = 1.0 - opt.beta2 ** opt.step
    head = (rows, 0 if combine == "sorted" else 1, lo, cnt, w, opt.opt_id(), master, s1, s2)
    tail = (gout, opt.lr, opt.momentum, opt.weight_decay, opt.beta1, opt.beta2, opt.eps,
            opt.lr / bc1, 1.0 / math.sqrt(bc2), opt.gscale, opt.nesterov, opt.first, mix, keep)
    return head, tail


def _check_keep(keep: Optional[int], combine: str, n: int) -> int:
    if not keep:
        return 0
    if combine != "sorted":
        raise ValueError("keep is a form of the sorted combine only")
    if keep < 0 or keep > n or 2 * keep < n:
        raise ValueError(f"keep must be 0 or in [n / 2, n] (keep={keep}, n={n})")
    return int(keep)


def _check_mix(mix: Optional[torch.Tensor], combine: str, n: int) -> None:
    if mix is None:
        return
    if combine != "sorted":
        raise ValueError("mix is a pre-mix of the sorted combine only")
    if n > 32:
        raise ValueError(f"the mixed sorted combine supports at most 32 rows (n={n})")
    if mix.dtype != torch.float32 or tuple(mix.shape) != (n, n) or not mix.is_contiguous():
        raise ValueError(f"mix must be a contiguous fp32 [{n}, {n}] tensor, got "
                         f"{mix.dtype} {tuple(mix.shape)}")


# --------------------------------------------------------------------------- Gram + weights
class GramWorkspace:
    """Per-device cache of the split-K partial buffer of the Gram kernel."""
    _cache = {}

    @classmethod
    def get(cls, device: torch.device, n: int, D: int) -> torch.Tensor:
        nbytes = lib().gram_workspace_bytes(n, D)
        key = (device, nbytes)
        buf = cls._cache.get(key)
        if buf is None:
            buf = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
            cls._cache[key] = buf
        return buf


def agg_update_multi(segs, *, combine: str, lo: int = 0, cnt: int = 1,
                     w: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None,
                     n: int, opt: Optional[OptArgs] = None, master: Optional[torch.Tensor] = None,
                     s1: Optional[torch.Tensor] = None, s2: Optional[torch.Tensor] = None,
                     gout: Optional[torch.Tensor] = None,
                     mix: Optional[torch.Tensor] = None, keep: Optional[int] = None) -> None:
    """``agg_update`` over several segments in ONE launch on GPU (the sharded engine's buckets).
    ``segs``: (X [rows, >= D], D, off, param_out) -- worker rows, element count, offset into the
    shared master / s1 / s2 / gout vectors, and the segment's parameters."""
    opt = opt or OptArgs(kind="none")
    _check_mix(mix, combine, n)
    keep = _check_keep(keep, combine, n)
    if segs and segs[0][0].is_cuda and len(segs) <= 16:
        head, tail = _binding_args(rows, combine, lo, cnt, w, opt, master, s1, s2, gout, mix, keep)
        lib().agg_update_multi([_as2d(x) for x, _, _, _ in segs], [int(d) for _, d, _, _ in segs],
                               [int(o) for _, _, o, _ in segs], [p for _, _, _, p in segs], n,
                               *head, *tail)
        return
    sl = lambda t, o, d: None if t is None else t[o:o + d]   # noqa: E731
    for X, D, off, pout in segs:
        agg_update(X, combine=combine, lo=lo, cnt=cnt, w=w, rows=rows, n=n, D=D, opt=opt,
                   master=sl(master, off, D), s1=sl(s1, off, D), s2=sl(s2, off, D),
                   param_out=pout, gout=sl(gout, off, D), mix=mix, keep=keep)


def gram(X: torch.Tensor, rows: Optional[torch.Tensor] = None, n: Optional[int] = None,
         D: Optional[int] = None, out: Optional[torch.Tensor] = None,
         accumulate: bool = False, center: Optional[torch.Tensor] = None,
         grid_cap: int = 0) -> torch.Tensor:
    """G = X X^T in fp64 ([n, n]); MFMA kernel on GPU. ``accumulate``: out += X X^T.
    ``center`` (int32 [1] on X's device): the Gram of the rows relative to row ``center[0]``
    (same distances, no cancellation for near-duplicate rows; see ``gram_center``).
    ``grid_cap`` > 0: at most that many stage-1 workgroups on GPU (tests of the multi-trip loops
    at small sizes; ignored on CPU)."""
    if accumulate and out is None:
        raise ValueError("accumulate needs out")
    X = _as2d(X)
    n = n if n is not None else (rows.numel() if rows is not None else X.shape[0])
    D = D if D is not None else X.shape[1]
    if X.is_cuda:
        if out is None:
            out = torch.empty(n, n, dtype=torch.float64, device=X.device)
        if X.data_ptr() % 16 or (X.stride(0) * X.element_size()) % 16:
            X = X[:n if rows is None else X.shape[0], :D].contiguous()
            X = torch.nn.functional.pad(X, (0, (-D) % 8))
        ws = GramWorkspace.get(X.device, n, D)
        lib().gram(X, n, D, rows, ws, out, accumulate, center, grid_cap)
        return out
    Xr = X[rows.long()] if rows is not None else X[:n]
    Xr = Xr[:, :D]
    if center is not None and int(center[0]) >= 0:   # a negative center: uncentered pass
        c = min(int(center[0]), n - 1)
        xc = Xr[c].double()
        Xr = Xr.double() - torch.where(torch.isfinite(xc), xc, torch.zeros_like(xc))
    G = ref.gram(Xr)
    if out is not None:
        if accumulate:
            out.add_(G)
        else:
            out.copy_(G)
        return out
    return G


def gram_center(G: torch.Tensor, n: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [1]: the medoid of the finite rows of G (least summed squared distance to the
    other finite rows; ties -> lower index), the center of a second, centered Gram pass."""
    if out is None:
        out = torch.zeros(1, dtype=torch.int32, device=G.device)
    if G.is_cuda:
        lib().gram_center(G[:n, :n].contiguous(), n, out)   # the CPU branch's block
        return out
    out.reshape(-1)[0] = ref.gram_center(G[:n, :n])   # (element 1 of an engine center: guard state)
    return out


def gram_sum(Gb: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out = Gb[0] + Gb[1] + ... in bucket order (one launch on GPU; the same fp64 adds as
    accumulating the buckets' Grams one after another)."""
    if Gb.is_cuda:
        lib().gram_sum(Gb, out)
        return out
    out.copy_(Gb[0])
    for k in range(1, Gb.shape[0]):
        out.add_(Gb[k])
    return out


def robust_weights(G: torch.Tensor, rule: str, n: int, f: int = 0, m: Optional[int] = None,
                   iters: int = 8, eps: float = 1e-6, tol: float = 0.0, tau: float = 10.0,
                   w_out: Optional[torch.Tensor] = None, scores: Optional[torch.Tensor] = None,
                   sel: Optional[torch.Tensor] = None, guard: bool = False,
                   center_out: Optional[torch.Tensor] = None,
                   sel_counts: Optional[torch.Tensor] = None, pre: str = "none",
                   mix_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weights over worker rows (fp32 [n] or [n+1] for centered clipping) from the Gram matrix.

    ``pre='nnm'``: nearest-neighbour mixing first. M = ``reference.nnm_matrix(G, n, f)`` (fp32
    [n, n] into ``mix_out``), the rule runs on the Gram of the mixed rows M G M^T, and the
    returned weights are M^T w -- weights over the ORIGINAL rows whose weighted sum is the
    rule's aggregate of the mixed rows. ``scores``, ``sel`` and ``sel_counts`` then refer to the
    mixed rows; the guard, the non-finite row count and ``center_out`` keep reading the unmixed
    G. Rule ``'nnm_only'`` (the coordinate rules' mixing matrix) writes only ``mix_out`` (the
    identity on a tripped guard) and leaves the weights alone.

    In the same launch (weights.hip): ``sel_counts`` += (w > 0); ``center_out`` = the medoid of
    G (the next step's Gram center); ``guard`` (G from a pass centered on the previous step's
    medoid): at least half the worker rows non-finite = a captured center -> weights zeroed
    (centered clipping keeps its previous aggregate) and ``center_out`` = -1. ``center_out``
    holds, on entry, the center this pass used: a negative one (an uncentered pass, e.g. the step
    after a trip) disarms the guard; a 2-element ``center_out`` also carries the previous pass's
    count of non-finite rows, and only an increase trips -- so workers that are genuinely
    non-finite (even half of them) are aggregated around instead of freezing the weights."""
    dim = n + 1 if rule == "centered_clip" else n
    if pre not in PRE_IDS:
        raise ValueError(f"unknown pre-aggregation {pre!r}; choose from {tuple(PRE_IDS)}")
    only = rule == "nnm_only"
    if (pre == "nnm" and rule in ("mean", "bulyan_select")) or (only and pre != "nnm"):
        raise ValueError(f"pre={pre!r} is not defined for rule {rule!r}")
    if only and mix_out is None:
        raise ValueError("rule 'nnm_only' needs mix_out")
    if G.is_cuda:
        if w_out is None:
            w_out = torch.empty(dim, dtype=torch.float32, device=G.device)
        lib().robust_weights(G.contiguous(), RULE_IDS[rule], n, f, m or 0, iters, eps, tol, tau,
                             w_out, scores, sel, guard, center_out, sel_counts, PRE_IDS[pre],
                             mix_out)
        return w_out
    if guard and center_out is not None and int(center_out.reshape(-1)[0]) < 0:
        guard = False
    Me = None
    if pre == "nnm":
        M = ref.nnm_matrix(G, n, f)
        if mix_out is not None:
            mix_out.copy_(M.float())
        Me = ref.nnm_extend(M, dim)
    if only:
        w = torch.zeros(n) if w_out is None else w_out.clone()
    else:
        Gr = G if Me is None else ref.nnm_gram(G[:dim, :dim], Me)
        w = _robust_weights_ref(Gr, rule, n, f, m, iters, eps, tol, tau, scores, sel)
    picked = w[:n] > 0                      # selections: over the (mixed) rows the rule saw
    if Me is not None and not only:
        w = (Me.t() @ w.double()).float()   # weights over the original rows
    nbad = int((~torch.isfinite(torch.diagonal(G)[:n])).sum())
    trip = guard and nbad > 0 and 2 * nbad >= n
    if center_out is not None and center_out.numel() >= 2:
        # element 1: the previous pass's non-finite row count (only an INCREASE trips)
        trip = trip and nbad > int(center_out.reshape(-1)[1])
        center_out.reshape(-1)[1] = nbad
    if trip:
        w = torch.zeros_like(w)
        if rule == "centered_clip":
            w[n] = 1.0
        picked = torch.zeros_like(picked)
        if sel is not None and rule != "bulyan_select":
            sel[:n].zero_()
        if only:
            mix_out.copy_(torch.eye(n))
    if only:
        if center_out is not None:
            center_out.reshape(-1)[0] = -1 if trip else ref.gram_center(G[:n, :n])
        return w if w_out is None else w_out
    if sel_counts is not None:
        sel_counts += picked.double()
    if center_out is not None:
        center_out.reshape(-1)[0] = -1 if trip else ref.gram_center(G[:n, :n])
    if w_out is not None:
        w_out.copy_(w)
        return w_out
    return w


def _robust_weights_ref(G, rule, n, f, m, iters, eps, tol, tau, scores, sel) -> torch.Tensor:
    if rule == "mean":
        bad = ~torch.isfinite(torch.diagonal(G))
        good = (~bad).double()
        w = good / good.sum().clamp_min(1)
    elif rule == "krum":
        w = ref.krum_weights(G, f, 1)
        if scores is not None:
            scores.copy_(ref.krum_scores(G, f))
    elif rule == "multi_krum":
        w = ref.krum_weights(G, f, m if m else n - f)
        if scores is not None:
            scores.copy_(ref.krum_scores(G, f))
    elif rule == "geomed":
        w = ref.weiszfeld_weights(G, iters, eps, tol)
    elif rule == "centered_clip":
        w = ref.centered_clip_weights(G, tau, iters)
    elif rule == "bulyan_select":
        idx = ref.bulyan_select(G, f)
        w = torch.zeros(n, dtype=torch.float64)
        w[idx] = 1.0 / idx.numel()
        if sel is not None:
            sel[: idx.numel()] = idx.to(sel.dtype)
            sel[n] = idx.numel()
    else:
        raise ValueError(rule)
    if sel is not None and rule != "bulyan_select":
        sel[:n].copy_((w[:n] > 0).to(sel.dtype))
    return w.float()


# --------------------------------------------------------------------------- high level
def aggregate(X: torch.Tensor, rule: str, f: int = 0, trim: Optional[int] = None,
              m: Optional[int] = None, iters: int = 8, eps: float = 1e-6, tau: float = 10.0,
              clip_iters: int = 3, v0: Optional[torch.Tensor] = None,
              pre: str = "none") -> torch.Tensor:
    """Full robust aggregate of a local [n, D] worker matrix -> fp32 [D] (native on GPU).
    ``pre='nnm'``: the rule on the nearest-neighbour-mixed rows (``robust_weights``)."""
    X = _as2d(X)
    n, D = X.shape
    out = torch.empty(D, dtype=torch.float32, device=X.device)
    if pre != "none" and rule in ("mean", "bulyan"):
        raise ValueError(f"pre={pre!r} is not defined for rule {rule!r}")
    plan = functools.partial(rule_combine, rule, n, f, trim)
    if rule in ("mean",):
        c = plan(w=torch.full((n,), 1.0 / n, device=X.device))
    elif rule in COORD_RULES:
        mix = None if pre == "none" else torch.empty(n, n, dtype=torch.float32, device=X.device)
        c = plan(mix=mix)
        if mix is not None:
            robust_weights(gram(X), "nnm_only", n, f, pre=pre, mix_out=mix)
    elif rule in ("krum", "multi_krum", "geomed"):
        c = plan(w=robust_weights(gram(X), rule, n, f, m, iters, eps, pre=pre))
    elif rule == "centered_clip":
        v0 = torch.zeros(D, dtype=X.dtype, device=X.device) if v0 is None else v0.to(X.dtype)
        X = torch.cat([X, v0[None]], 0)
        # non-finite workers carry weight 0 and are skipped by the weighted kernel
        c = plan(w=robust_weights(gram(X), "centered_clip", n, f, tau=tau, iters=clip_iters,
                                  pre=pre), rows_total=n + 1)
    elif rule == "bulyan":
        sel = torch.zeros(n + 1, dtype=torch.int32, device=X.device)
        robust_weights(gram(X), "bulyan_select", n, f, sel=sel)
        c = plan(sel=sel)
    else:
        raise ValueError(f"unknown rule {rule!r}")
    agg_update(X, gout=out, **c.kwargs())
    return out


def gossip_mix(master: torch.Tensor, left: torch.Tensor, right: torch.Tensor, w0: float,
               w1: float, w2: float, clip: float = 0.0,
               param_out: Optional[torch.Tensor] = None,
               work: Optional[torch.Tensor] = None) -> None:
    """In-place ring mixing of the fp32 master with the neighbours' bf16 parameters (the k = 2
    form of ``gossip_mix_k``, including its rule for non-finite neighbours under clipping)."""
    if master.is_cuda:
        if work is None:
            work = torch.empty(lib().gossip_workspace_bytes(master.numel()) // 4,
                               dtype=torch.float32, device=master.device)
        lib().gossip_mix(master, param_out, left, right, w0, w1, w2, clip, work)
        return
    x = ref.gossip_mix(master, left, right, w0, w1, w2, clip)
    master.copy_(x)
    if param_out is not None:
        param_out.copy_(x.to(param_out.dtype))


def gossip_mix_k(master: torch.Tensor, nbrs: List[torch.Tensor], w: List[float], w0: float,
                 clip: float = 0.0, param_out: Optional[torch.Tensor] = None,
                 work: Optional[torch.Tensor] = None,
                 param_out2: Optional[torch.Tensor] = None, grid_cap: int = 0) -> None:
    """In-place k-neighbour mixing (1 <= k <= 8) of the fp32 master with the neighbours' bf16
    parameters: x <- (w0 + sum w_k) x + sum_k w_k clip_k(nb_k - x). ``param_out2``: a second
    copy of the rounded parameters (the delayed-gossip send buffer) written in the same pass.

    With ``clip`` > 0 a neighbour whose squared distance to x (summed in fp32) is not finite --
    it holds a NaN or an Inf, or the sum overflows -- is dropped: its term is exactly zero at
    every coordinate and its weight stays with x; a non-finite x drops every neighbour.
    ``clip`` == 0 gives no protection: a NaN propagates.

    ``grid_cap`` > 0 caps the launch at that many workgroups, which then stride over the vector
    (for tests of the multi-trip loops at small sizes); 0 is the default launch."""
    if master.is_cuda:
        if work is None:
            work = torch.empty(lib().gossip_workspace_bytes(master.numel()) // 4,
                               dtype=torch.float32, device=master.device)
        lib().gossip_mix_k(master, param_out, list(nbrs), [float(v) for v in w], w0, clip, work,
                           param_out2, grid_cap=grid_cap)
        return
    x = ref.gossip_mix_k(master, nbrs, w, w0, clip)
    master.copy_(x)
    if param_out is not None:
        param_out.copy_(x.to(param_out.dtype))
    if param_out2 is not None:
        param_out2.copy_(x.to(param_out2.dtype))


FAULT_IDS = {"none": 0, "sign_flip": 1, "gaussian": 2, "scaled": 3, "zero": 4, "nan": 5}


def inject_fault(g: torch.Tensor, kind: str, scale: float = 10.0, sigma: float = 1.0,
                 seed: int = 0) -> None:
    """Corrupt a local flat gradient in place (Byzantine simulation)."""
    if kind == "none":
        return
    if g.is_cuda and kind in FAULT_IDS:
        lib().fault(g, FAULT_IDS[kind], scale, sigma, seed)
        return
    if kind == "sign_flip":
        g.mul_(-scale)
    elif kind == "gaussian":
        gen = torch.Generator(device=g.device).manual_seed(seed)
        g.copy_(torch.randn(g.shape, generator=gen, device=g.device) * sigma)
    elif kind == "scaled":
        g.mul_(scale)
    elif kind == "zero":
        g.zero_()
    elif kind == "nan":
        g.fill_(float("nan"))
    else:
        raise ValueError(f"fault {kind!r} needs cross-worker statistics (see parallel.faults)")


WORKER_MOMENTUM_PASS = 256 * 4 * 8   # elements of a row one workgroup covers per pass
                                     # (kMB * kMU * 8, worker_momentum.hip)


def worker_momentum(rows: torch.Tensor, mom: torch.Tensor, beta: float) -> None:
    """Worker-side momentum over an [R, L] window, in place: ``mom`` (fp32) <- beta * mom + rows,
    ``rows`` (bf16 / fp32) <- mom rounded to the rows' dtype. Unit column stride, any row stride
    (a bucket's column range of the flat gradient buffer and of the momentum state)."""
    if rows.is_cuda:
        lib().worker_momentum(rows, mom, float(beta))
        return
    if rows.shape != mom.shape or mom.dtype != torch.float32:
        raise ValueError(f"worker_momentum: rows {tuple(rows.shape)} {rows.dtype} against mom "
                         f"{tuple(mom.shape)} {mom.dtype}")
    ref.worker_momentum(rows, mom, beta)


# --------------------------------------------------------------------------- global-norm clipping
CLIP_STATS = ref.CLIP_STATS   # fp64 elements of a clipping stats tensor: [norm, coef, non-finite
                              # norms seen so far, squared norm]


def sq_norm_workspace(segments, device=None) -> torch.Tensor:
    """An fp64 workspace large enough for ``sq_norm`` over these segments (one partial per
    workgroup; allocate once and reuse while the segment lengths stay the same)."""
    segments = list(segments)
    if segments and segments[0].is_cuda:
        n = lib().sq_norm_workspace(segments[0].dtype == torch.bfloat16,
                                    [int(s.numel()) for s in segments])
        return torch.empty(max(int(n), 1), dtype=torch.float64, device=segments[0].device)
    return torch.empty(1, dtype=torch.float64, device=device or "cpu")


def sq_norm(segments, scale: float, work: Optional[torch.Tensor], out: torch.Tensor,
            grid_cap: int = 0) -> torch.Tensor:
    """out[0] (fp64) = sum over every element x of the segments of (float(x) * scale)^2
    (``reference.sq_norm``). ``segments``: contiguous 1-D tensors of one dtype (bf16 / fp32) on
    one device. GPU: fp64 per-workgroup partials into ``work`` (``sq_norm_workspace``; None
    allocates one) summed in index order, no atomics: the same data gives the same bits."""
    segments = [s.reshape(-1) for s in segments]
    if not segments:
        raise ValueError("sq_norm: no segments")
    if segments[0].is_cuda:
        if work is None:
            work = sq_norm_workspace(segments)
        lib().sq_norm(segments, float(scale), work, out, grid_cap)
        return out
    out.reshape(-1)[0] = ref.sq_norm(segments, scale)
    return out


def clip_coef(norm2: torch.Tensor, max_norm: float, base: float, w_out: torch.Tensor,
              stats: torch.Tensor, reduced: Optional[torch.Tensor] = None) -> torch.Tensor:
    """w_out[0] (fp32) = base * min(1, max_norm / (sqrt(s) + 1e-6)) with s = ``reduced[0]`` when
    given (the squared norm all-reduced over ranks), else ``norm2[0]``; ``stats`` (fp64
    [CLIP_STATS]) = [norm, coef, += 1 when s is not finite (then coef = 0), s]
    (``reference.clip_coef``). Nothing is read back to the host on the GPU path."""
    if max_norm < 0:
        raise ValueError(f"clip_coef: max_norm must not be negative (got {max_norm})")
    if norm2.is_cuda:
        lib().clip_coef(norm2, float(max_norm), float(base), w_out, stats, reduced)
        return w_out
    s = reduced if reduced is not None else norm2
    w, norm, coef, bad = ref.clip_coef(s, max_norm, base)
    w_out.reshape(-1)[0] = w
    st = stats.reshape(-1)
    st[0], st[1], st[3] = norm, coef, s.reshape(-1)[0]
    st[2] += bad
    return w_out


# --------------------------------------------------------------------------- LARS
LARS_STATS = ref.LARS_STATS   # fp64 per tensor: [wn, gn, q, steps with a non-finite norm]
# Elements of one work item of the segmented norm pass. Measured over the project's two standard
# sizes, as one tensor and cut like ResNet-50's tensor list, for C = 4096 .. 262144: 65536 is the
# fastest or within the spread of the fastest in all four (profiles/lars/README.md)
LARS_CHUNK = 65536


class LarsPlan:
    """Tables of one state vector for the LARS kernels (``lars_plan``). Tensor t (the caller's
    order, ascending in the vector) holds elements [starts[t], starts[t] + numels[t]);
    ``starts[T]`` is the vector length. ``items`` (int64 [I, 3] of (tensor, start, len)) cuts every
    tensor into chunks of at most ``chunk`` elements, ``item_off`` (int64 [T + 1]) indexes them per
    tensor. The device copies are made once per device."""

    def __init__(self, starts: List[int], numels: List[int], chunk: int, items: torch.Tensor,
                 item_off: torch.Tensor):
        self.starts, self.numels, self.chunk = starts, numels, chunk
        self.items, self.item_off = items, item_off
        self.T = len(numels)
        self.total = starts[-1]
        self._dev = {}

    def on(self, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(items, item_off, starts, work) on ``device``; work: fp64 [2 I] partials."""
        key = torch.device(device)
        hit = self._dev.get(key)
        if hit is None:
            hit = (self.items.to(key), self.item_off.to(key),
                   torch.tensor(self.starts, dtype=torch.int64, device=key),
                   torch.empty(max(2 * self.items.shape[0], 1), dtype=torch.float64, device=key))
            self._dev[key] = hit
        return hit


def lars_plan(starts, numels, chunk: int = 0, total: Optional[int] = None) -> LarsPlan:
    """The work tables of the LARS kernels over a state vector whose tensor t occupies
    [starts[t], starts[t] + numels[t]) (``numels[t]`` may be 0: a tensor with no element on this
    rank). Starts ascend from 0, are multiples of 8 elements (so both rows load 16 B per lane and
    a vector never straddles two tensors) and tensors do not overlap. ``chunk``: most elements of
    a work item, a positive multiple of 8 (0: ``LARS_CHUNK``). ``total``: the vector length
    (default: the end of the last tensor rounded up to 8)."""
    starts = [int(s) for s in starts]
    numels = [int(n) for n in numels]
    chunk = int(chunk) or LARS_CHUNK
    if len(starts) != len(numels) or not starts:
        raise ValueError("lars_plan: starts and numels must be non-empty and of equal length")
    if chunk <= 0 or chunk % 8:
        raise ValueError(f"lars_plan: chunk must be a positive multiple of 8 (got {chunk})")
    if starts[0] != 0:
        raise ValueError(f"lars_plan: the first tensor must start at 0 (got {starts[0]})")
    end = 0
    for t, (s, n) in enumerate(zip(starts, numels)):
        if s % 8:
            raise ValueError(f"lars_plan: start {s} of tensor {t} is not a multiple of 8 elements")
        if n < 0 or s < end:
            raise ValueError(f"lars_plan: tensor {t} [{s}, +{n}) overlaps its predecessor or is "
                             "negative")
        end = max(end, s + n)
    end8 = -(-end // 8) * 8
    total = end8 if total is None else int(total)
    if total < end:
        raise ValueError(f"lars_plan: total {total} is shorter than the tensors ({end})")
    if total % 8:
        raise ValueError(f"lars_plan: total {total} is not a multiple of 8 elements")
    items, item_off = [], [0]
    for t, (s, n) in enumerate(zip(starts, numels)):
        for a in range(0, n, chunk):
            items.append((t, s + a, min(chunk, n - a)))
        item_off.append(len(items))
    it = torch.tensor(items, dtype=torch.int64).reshape(-1, 3)
    return LarsPlan(starts + [total], numels, chunk, it, torch.tensor(item_off, dtype=torch.int64))


def seg_sq_norm(master: torch.Tensor, g: torch.Tensor, scale: float, plan: LarsPlan,
                out: Optional[torch.Tensor] = None, grid_cap: int = 0) -> torch.Tensor:
    """out (fp64 [T, 2]) = per tensor (sum p^2, sum (float(x) * scale)^2) over exactly the tensor's
    elements of the fp32 master and the co-indexed gradient row ``g`` (bf16 / fp32)
    (``reference.seg_sq_norm``). GPU: one read-only pass, fp64 partials per work item summed in a
    fixed order, no atomics: the same data gives the same bits."""
    if out is None:
        out = torch.zeros(plan.T, 2, dtype=torch.float64, device=master.device)
    if master.is_cuda:
        items, item_off, _, work = plan.on(master.device)
        lib().seg_sq_norm(master, g, float(scale), items, item_off, plan.total, work, out,
                          grid_cap)
        return out
    out.copy_(ref.seg_sq_norm(master, g, scale, plan.starts[:-1], plan.numels))
    return out


def lars_ratio(pairs: torch.Tensor, adapt: torch.Tensor, trust: float, weight_decay: float,
               eps: float, q: torch.Tensor, stats: torch.Tensor,
               reduced: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q (fp32 [T]) = the trust ratios from ``pairs`` (fp64 [T, 2], ``seg_sq_norm``), or from
    ``reduced`` when given (the pairs all-reduced over ranks); ``adapt`` (uint8 [T]): the tensors
    LARS adapts. ``stats`` (fp64 [T, LARS_STATS]) = [wn, gn, q, += 1 when a norm is not finite
    (then q = 0)] (``reference.lars_ratio``). Nothing is read back to the host on the GPU path."""
    if not (trust > 0 and math.isfinite(trust)):
        raise ValueError(f"lars_ratio: trust must be a finite number > 0 (got {trust})")
    if pairs.is_cuda:
        lib().lars_ratio(pairs, adapt, float(trust), float(weight_decay), float(eps), q, stats,
                         reduced)
        return q
    qq, st, bad = ref.lars_ratio(reduced if reduced is not None else pairs, adapt, trust,
                                 weight_decay, eps)
    q.copy_(qq)
    stats = stats.reshape(-1, LARS_STATS)
    stats[:, :3] = st
    stats[:, 3] += bad.double()
    return q


def lars_update(g: torch.Tensor, scale: float, plan: LarsPlan, q: torch.Tensor, opt: OptArgs,
                master: torch.Tensor, s1: Optional[torch.Tensor] = None, segs=None,
                grid_cap: int = 0) -> None:
    """The LARS step in place over the state vector: ``reference.lars_update`` with the factors
    ``q`` (``lars_ratio``) on the gradient row ``g`` times ``scale``, ``opt`` = OptArgs(kind=
    "lars") for lr / momentum / weight_decay / nesterov / first. ``segs``: output segments
    (param_out or None, state offset, length) -- the parameters rewritten from the master (bf16 /
    fp32); None = no parameter output over the whole vector. GPU: 16 segments per launch."""
    if opt.kind != "lars":
        raise ValueError(f"lars_update takes OptArgs(kind='lars'), got {opt.kind!r}")
    if segs is None:
        segs = [(None, 0, plan.total)]
    segs = [(p, int(o), int(n)) for p, o, n in segs]
    if master.is_cuda:
        _, _, starts, _ = plan.on(master.device)
        lib().lars_update(g, float(scale), master, s1, q, starts, plan.starts,
                          [p for p, _, _ in segs], [o for _, o, _ in segs],
                          [n for _, _, n in segs], opt.lr, opt.momentum, opt.weight_decay,
                          opt.nesterov, opt.first, grid_cap)
        return
    for _, o, n in segs:
        if o % 8 or o < 0 or o + n > plan.total:
            raise ValueError(f"lars_update: segment [{o}, +{n}) must start at a multiple of 8 "
                             f"inside the state vector of {plan.total}")
    p, b = ref.lars_update(master, g, s1, q, plan.starts, scale, opt.lr, opt.momentum,
                           opt.weight_decay, opt.nesterov, opt.first)
    for pout, o, n in segs:     # (the reference computes the whole vector; segments select)
        master[o:o + n].copy_(p[o:o + n])
        if opt.momentum:
            s1[o:o + n].copy_(b[o:o + n])
        if pout is not None:
            pout[:n].copy_(p[o:o + n].to(pout.dtype))
