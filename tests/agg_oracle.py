"""Float64 oracle, case table and checker for the fused aggregate-and-update kernel (not
collected: no ``test_`` prefix). Shared by ``test_agg_update_oracle_cpu.py`` (CPU branch of
``K.agg_update``) and ``test_agg_update_oracle_gpu.py`` (``csrc/kernels/agg_update.hip``).

The oracle is plain torch in float64 and uses nothing of ``consensusml_amd``:

``combine64``  the sorted-rank window mean or the weighted sum of the worker rows, the same
               combine over absolute values (the magnitude a rounding bound scales with) and the
               number of terms.
``step64``     one SGD / Adam / AdamW step with ``torch.optim`` semantics.

``run_case`` / ``run_multi_case`` build the inputs of one table entry, call the kernel and assert

(a) ``|gout - g64| <= (k + 2) * 2**-23 * A`` elementwise (forward bound of k fp32 fmas or adds
    plus the 1/cnt and gscale multiplies at unit roundoff 2**-24, doubled; the smallest fp32
    subnormal where A == 0), and bit equality with the selected element for a one-rank window of
    bf16 rows at gscale 1,
(b) master / s1 / s2 against ``step64`` fed with the kernel's own ``gout``, at the tolerances of
    ``test_kernels_gpu.py::test_fused_update``,
(c) ``param_out`` equal to the kernel's own master (rounded to nearest even for bf16),
(d) untouched sentinels in 64-element guard bands around every output, and finite results
    although every element of X the call must not read (columns [D, ld), unused rows,
    zero-weight rows) is NaN,
(e) with ``first`` the momentum buffer, pre-filled with NaN, comes back as the effective gradient.
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

GUARD = 64
SENT = 77.0                      # exact in bf16 and fp32
TINY = 2.0 ** -149               # smallest fp32 subnormal
# tolerances of test_fused_update: (rtol, atol)
TOL_MASTER = (1e-5, 1e-5)
TOL_SGD_BUF = (1e-5, 1e-5)
TOL_ADAM_M = (1e-4, 1e-6)
TOL_ADAM_V = (1e-4, 1e-7)


# --------------------------------------------------------------------------- oracle
def combine64(X, rows, n, D, combine, lo, cnt, w, gscale):
    """(g, A, k): combined gradient, the same combine over absolute values, number of terms."""
    R = X[rows.long()] if rows is not None else X[:n]
    R = R[:, :D].double()
    if combine == "sorted":
        R = torch.where(torch.isnan(R), torch.full_like(R, math.inf), R)
        S = R.sort(dim=0).values[lo:lo + cnt]
        g, A, k = S.sum(0) / cnt, S.abs().sum(0) / cnt, cnt
    else:
        ww = torch.ones(n, dtype=torch.float64, device=X.device) if w is None else w[:n].double()
        keep = (ww != 0).nonzero().flatten()
        T = ww[keep, None] * R[keep]
        g, A, k = T.sum(0), T.abs().sum(0), int(keep.numel())
    return g * gscale, A * abs(gscale), k


def step64(kind, p, g, s1, s2, *, lr, momentum=0.0, weight_decay=0.0, nesterov=False,
           first=False, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    """One optimizer step in the dtype of its inputs (float64 here): new (p, s1, s2)."""
    if kind == "sgd":
        if weight_decay:
            g = g + weight_decay * p
        if momentum:
            s1 = g.clone() if first else momentum * s1 + g
            g = g + momentum * s1 if nesterov else s1
        return p - lr * g, s1, s2
    assert kind in ("adam", "adamw"), kind
    if kind == "adam" and weight_decay:
        g = g + weight_decay * p
    if kind == "adamw":
        p = p * (1.0 - lr * weight_decay)
    m = beta1 * s1 + (1.0 - beta1) * g
    v = beta2 * s2 + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * m / denom, m, v


# --------------------------------------------------------------------------- case table
OPTS = {
    "none": dict(kind="none"),
    "sgd_m0": dict(kind="sgd", lr=0.05, momentum=0.0, weight_decay=0.01),          # s1=None
    "sgd_first": dict(kind="sgd", lr=0.05, momentum=0.9, weight_decay=0.01, first=True),
    "sgd_plain": dict(kind="sgd", lr=0.05, momentum=0.9, weight_decay=0.01),
    "sgd_nesterov": dict(kind="sgd", lr=0.05, momentum=0.9, weight_decay=0.01, nesterov=True),
    "sgd_wd0": dict(kind="sgd", lr=0.05, momentum=0.9, weight_decay=0.0),
    "adam": dict(kind="adam", lr=0.01, weight_decay=0.01, step=3),
    "adamw": dict(kind="adamw", lr=0.01, weight_decay=0.01, step=3),
    "adam_step1": dict(kind="adam", lr=0.01, weight_decay=0.01, step=1),
}
CORE_NS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)     # both edges of every NP bucket
CORE_CYCLE = ("sgd_nesterov", "adam", "sgd_plain", "adamw", "sgd_first", "adam_step1", "sgd_m0")


def np_bucket(n):
    return next(b for b in (2, 4, 8, 16, 32, 64) if n <= b)


def window(combine, n):
    """Rank window of the table's sorted combines: the median, or a trimmed window with lo >= 1
    (n == 2 leaves only rank 1)."""
    if combine == "median":
        return ((n - 1) // 2, 1) if n % 2 else (n // 2 - 1, 2)
    assert combine == "trimmed" and n >= 2
    lo = max(1, n // 4)
    return lo, max(1, n - 2 * lo)


@dataclass(frozen=True)
class Case:
    id: str
    dtype: str                    # worker rows: bf16 | f32
    n: int
    D: int
    combine: str                  # median | trimmed | weighted
    opt: str                      # key of OPTS
    pout: str = "bf16"            # param_out: bf16 | f32
    gscale: float = 1.0
    wzero: Optional[Tuple[int, ...]] = None   # zero weights (default: every i % 3 == 1)
    wnone: bool = False           # w=None (all ones)
    rows: Optional[Tuple[int, ...]] = None    # row indirection into xrows rows
    xrows: int = 0
    mis: str = ""                 # xbase | xstride | state | pout: legal misalignment
    special: bool = False         # +-inf, +-NaN, +-0, subnormals in the rows
    seed: int = 0


@dataclass(frozen=True)
class MultiCase:
    id: str
    dtype: str
    n: int
    Ds: Tuple[int, ...]
    combine: str
    opt: str
    pout: str = "bf16"
    gscale: float = 1.0
    rows: Optional[Tuple[int, ...]] = None
    xrows: int = 0
    misoff: int = -1              # segment whose state offset is moved off the vector grid
    seed: int = 0


def _single_cases():
    cs = []
    i = 0
    # core cross (n = 1 has no window with lo >= 1)
    for dt in ("bf16", "f32"):
        for comb in ("median", "trimmed", "weighted"):
            for n in CORE_NS:
                if comb == "trimmed" and n < 2:
                    continue
                D = 2059 if n <= 32 else 2051
                opt = CORE_CYCLE[i % len(CORE_CYCLE)]
                cs.append(Case(f"core-{dt}-{comb}-n{n}-{opt}", dt, n, D, comb, opt,
                               pout=("bf16", "f32")[i % 2], seed=i))
                i += 1
    # optimizer cross
    combs = ("median", "trimmed", "weighted")
    for n in (5, 33):
        for dt in ("bf16", "f32"):
            for opt in OPTS:
                for po in ("bf16", "f32"):
                    for gs in (1.0, 0.125):
                        cs.append(Case(f"opt-{dt}-n{n}-{opt}-p{po}-gs{gs}", dt, n,
                                       2059 if n <= 32 else 2051, combs[i % 3], opt, pout=po,
                                       gscale=gs, seed=i))
                        i += 1
    # weighted remainder loop
    perm = (4, 0, 7, 2, 8, 5, 1, 6, 3)
    for dt in ("bf16", "f32"):
        for j, nz in enumerate((0, 1, 2, 3, 4, 5, 7, 8, 9)):
            opt = ("sgd_plain", "adam")[j % 2]
            cs.append(Case(f"wrem-{dt}-nz{nz}-{opt}", dt, 9, 2059, "weighted", opt,
                           wzero=perm[:9 - nz], seed=i))
            i += 1
        cs.append(Case(f"wrem-{dt}-nz0-adamw", dt, 9, 2059, "weighted", "adamw", wzero=perm,
                       seed=i))
        for n in (1, 6):
            cs.append(Case(f"wrem-{dt}-wnone-n{n}", dt, n, 2059, "weighted", "sgd_nesterov",
                           wnone=True, seed=i + n))
        i += 8
    # rows indirection
    pick = (9, 2, 11, 0, 5, 7, 4)
    for dt in ("bf16", "f32"):
        cs.append(Case(f"rows-{dt}-trimmed-adamw", dt, 7, 2059, "trimmed", "adamw", rows=pick,
                       xrows=12, seed=i))
        cs.append(Case(f"rows-{dt}-weighted-sgd", dt, 7, 2059, "weighted", "sgd_nesterov",
                       rows=pick, xrows=12, pout="f32", gscale=0.125, seed=i + 1))
        i += 2
    # tiny and exact sizes
    for dt in ("bf16", "f32"):
        for D in (1, 7, 8, 2048):
            cs.append(Case(f"size-{dt}-D{D}-median", dt, 5, D, "median", "sgd_nesterov", seed=i))
            cs.append(Case(f"size-{dt}-D{D}-weighted", dt, 5, D, "weighted", "adam", pout="f32",
                           seed=i + 1))
            i += 2
    # misaligned but legal inputs: the launcher takes the scalar path
    for mis in ("xbase", "xstride", "state", "pout"):
        for dt in ("bf16", "f32"):
            cs.append(Case(f"mis-{mis}-{dt}-trimmed", dt, 8, 2059, "trimmed", "sgd_plain",
                           mis=mis, seed=i))
            cs.append(Case(f"mis-{mis}-{dt}-weighted", dt, 9, 2059, "weighted", "adamw",
                           mis=mis, pout="f32", seed=i + 1))
            cs.append(Case(f"mis-{mis}-{dt}-n33", dt, 33, 2051, "median", "adam", mis=mis,
                           seed=i + 2))
            i += 3
    # special values through an optimizer
    for opt in ("sgd_nesterov", "adamw"):
        cs.append(Case(f"special-{opt}", "bf16", 8, 2059, "trimmed", opt, special=True, seed=i))
        i += 1
    return cs


def _gs_segs(big, vec):
    """16 segment sizes for the one-launch path: ``big`` plus 15 of 8 .. 4096 elements, all
    multiples of 8 except one segment of exactly one vector."""
    small = [max(vec, 8), 16, 4096, 264, 1024, 2048, 520, 40, 3072, 128, 776, 1536, 96, 4000, 808]
    if vec < 8:
        small[3] = vec
    return tuple(small[:5] + [big] + small[5:])


def _multi_cases():
    cs = []
    i = 1000
    # grid-stride: with 16 segments the grid is capped at 2048 / 16 = 128 workgroups of 256
    # threads, 32768 vectors per trip; the big segment is three full trips plus a ragged rest.
    # (Weighted bf16 rows always use 8-element vectors, so the n = 33 size, a multiple of 2
    # only, reaches the one-launch path with the sorted combine alone.)
    shapes = (("bf16", 8, 3 * 262144 + 8 * 37, 8), ("f32", 8, 3 * 131072 + 4 * 9, 4),
              ("bf16", 33, 3 * 65536 + 2 * 11, 2))
    for dt, n, big, vec in shapes:
        for comb in ("trimmed", "weighted"):
            if comb == "weighted" and n > 32:
                continue
            for opt in ("sgd_nesterov", "adamw"):
                cs.append(MultiCase(f"stride-{dt}-n{n}-{comb}-{opt}", dt, n, _gs_segs(big, vec),
                                    comb, opt, seed=i))
                i += 1
    # Bulyan shape: theta = 6 of n = 8 rows, trimmed window, 4 segments
    pick = (6, 1, 7, 3, 0, 4)
    for dt in ("bf16", "f32"):
        for opt in ("sgd_nesterov", "adamw"):
            cs.append(MultiCase(f"bulyan-{dt}-{opt}", dt, 6, (4096, 12288, 800, 20000), "trimmed",
                                opt, rows=pick, xrows=8, seed=i))
            i += 1
        # the weighted combine through the same rows: w[i] pairs with rows[i]
        cs.append(MultiCase(f"rows-weighted-{dt}", dt, 6, (4096, 12288, 800, 20000), "weighted",
                            "sgd_plain", rows=pick, xrows=8, seed=i))
        i += 1
    # fallbacks: per-segment launches (offset or size off the vector grid), Python loop (> 16)
    for dt in ("bf16", "f32"):
        cs.append(MultiCase(f"fallback-off-{dt}", dt, 8, (4096, 2048, 808, 520), "trimmed",
                            "sgd_plain", misoff=2, seed=i))
        cs.append(MultiCase(f"fallback-ragged-{dt}", dt, 8, (4096, 2051, 808, 520), "weighted",
                            "adamw", seed=i + 1))
        cs.append(MultiCase(f"fallback-17seg-{dt}", dt, 5, tuple(8 * (j + 1) for j in range(17)),
                            ("median", "weighted")[dt == "f32"], "adam", seed=i + 2))
        i += 3
    # fp32 parameters from fp32 rows (gout + optimizer is part of every case)
    for comb in ("median", "weighted"):
        cs.append(MultiCase(f"pf32-{comb}", "f32", 9, (1024, 4096, 264), comb, "sgd_first",
                            pout="f32", gscale=0.125, seed=i))
        i += 1
    return cs


CASES = _single_cases()
MULTI_CASES = _multi_cases()


# --------------------------------------------------------------------------- input builders
def _tdt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def _worker_rows(gen, dtype, n, D, used, R, mis="", special=False, nan_rows=()):
    """[R, ld] worker matrix (CPU) with ld > D: random values in rows ``used``, columns [0, D);
    NaN everywhere else and in ``nan_rows``."""
    ld = (D + 7) // 8 * 8 + 8 + (1 if mis == "xstride" else 0)
    o = 1 if mis == "xbase" else 0
    flat = torch.full((R * ld + o + 7,), math.nan).to(dtype)
    X = flat[o:o + R * ld].view(R, ld)
    vals = torch.randn(n, D, generator=gen).to(dtype)
    if special:   # as test_sorted_bf16_extremes: +inf -inf +nan -nan +0 -0 sub -sub
        pat = torch.tensor([0x7F80, -128, 0x7FC0, -64, 0, -32768, 1, -32767], dtype=torch.int16)
        idx = torch.randint(0, n * D, (n * D // 8,), generator=gen)
        vals.view(torch.int16).view(-1)[idx] = pat[torch.arange(idx.numel()) % 8]
    for i, r in enumerate(used):
        X[r, :D] = math.nan if i in nan_rows else vals[i]
    return flat, X, o, ld


def _on(dev, flat, o, R, ld):
    """The view ``flat[o:].view(R, ld)`` rebuilt on ``dev`` (keeps the element offset)."""
    return flat.to(dev)[o:o + R * ld].view(R, ld)


def _weights(gen, c_n, wzero, wnone, size):
    if wnone:
        return None, ()
    zero = tuple(i for i in range(c_n) if i % 3 == 1) if wzero is None else tuple(wzero)
    w = torch.rand(size, generator=gen) + 0.1      # entries past n are never used
    for i in zero:
        w[i] = 0.0
    return w, zero


def _state(gen, kind, first, numel):
    """Random master / s1 / s2 values of an optimizer family (CPU fp32)."""
    m = torch.randn(numel, generator=gen)
    if kind == "sgd":
        s1 = torch.full((numel,), math.nan) if first else torch.randn(numel, generator=gen)
        return m, s1, None
    s1 = 0.1 * torch.randn(numel, generator=gen)
    s2 = 0.05 + torch.rand(numel, generator=gen)   # Adam's second moment is positive
    return m, s1, s2


def _guarded(vals, numel, off, dtype, dev):
    """Buffer of numel + 2 GUARD + 1 sentinels with ``vals`` (or NaN) at [off, off + numel)."""
    buf = torch.full((numel + 2 * GUARD + 1,), SENT)
    buf[off:off + numel] = math.nan if vals is None else vals
    return buf.to(dtype).to(dev)


def _guards_intact(buf, off, numel):
    return bool((buf[:off] == SENT).all()) and bool((buf[off + numel:] == SENT).all())


# --------------------------------------------------------------------------- checker
def _close(got, want, tol, what):
    torch.testing.assert_close(got.double(), want, rtol=tol[0], atol=tol[1], msg=lambda m: f"{what}: {m}")


def check_segment(what, X, rows, n, D, sorted_, lo, cnt, w, hyper, gscale, before, after,
                  bf16_rows, special=False):
    """Assertions (a), (b), (c) and (e) for one segment. ``before`` = (master, s1, s2) as the
    call got them, ``after`` = (master, s1, s2, gout, param_out) as it left them."""
    m0, s10, s20 = before
    m1, s11, s21, gout, pout = after
    kind = hyper["kind"]
    # (a) aggregated gradient
    g64, A, k = combine64(X, rows, n, D, "sorted" if sorted_ else "weighted", lo, cnt, w, gscale)
    go = gout.double()
    fin = torch.isfinite(g64)
    if not special:
        assert bool(fin.all()), f"{what}: oracle gradient not finite"
        assert bool(torch.isfinite(gout).all()), f"{what}: gout not finite"
    same = (go == g64) | (torch.isnan(go) & torch.isnan(g64))
    assert bool(same[~fin].all()), f"{what}: gout differs where the oracle is inf / NaN"
    bound = torch.where(A == 0, torch.full_like(A, TINY), (k + 2) * 2.0 ** -23 * A)
    err = (go - g64).abs()[fin]
    ratio = (err / bound[fin]).max().item() if err.numel() else 0.0
    print(f"{what}: k={k} max |gout - g64| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: gout error {ratio:.3f} of the bound (k={k})"
    if sorted_ and bf16_rows and cnt == 1 and gscale == 1.0 and not special:
        assert torch.equal(gout.view(torch.int32), g64.float().view(torch.int32)), \
            f"{what}: one-rank window of bf16 rows is not the selected element bit for bit"
    # (b) optimizer state against step64 fed with the kernel's own gradient
    if kind == "none":
        return
    ok = torch.isfinite(gout)
    d = lambda t: None if t is None else t.double()   # noqa: E731
    pe, s1e, s2e = step64(kind, d(m0), go, d(s10), d(s20),
                          **{k_: v for k_, v in hyper.items() if k_ != "kind"})
    if not special:
        assert bool(torch.isfinite(m1).all()), f"{what}: master not finite"
    _close(m1[ok], pe[ok], TOL_MASTER, f"{what} master")
    if kind == "sgd":
        if hyper.get("momentum"):
            _close(s11[ok], s1e[ok], TOL_SGD_BUF, f"{what} momentum buffer")
            if hyper.get("first") and not special:   # (e)
                assert bool(torch.isfinite(s11).all()), f"{what}: first step read s1"
    else:
        _close(s11[ok], s1e[ok], TOL_ADAM_M, f"{what} Adam m")
        _close(s21[ok], s2e[ok], TOL_ADAM_V, f"{what} Adam v")
    # (c) parameters are the kernel's own master in the parameter dtype
    want = m1.to(pout.dtype)
    num = ~torch.isnan(m1)
    assert torch.equal(pout[num], want[num]), f"{what}: param_out != master as {pout.dtype}"
    assert bool(torch.isnan(pout[~num]).all()), f"{what}: param_out where master is NaN"


def _hyper(c):
    return dict(OPTS[c.opt])


def run_case(c: Case, dev, K):
    """Build the inputs of ``c`` on ``dev``, call ``K.agg_update`` and check (a)-(e)."""
    gen = torch.Generator().manual_seed(c.seed)
    dtype = _tdt(c.dtype)
    n, D = c.n, c.D
    used = list(c.rows) if c.rows else list(range(n))
    R = c.xrows if c.rows else n + 1
    sorted_ = c.combine != "weighted"
    lo, cnt = window(c.combine, n) if sorted_ else (0, 1)
    w, zero = (None, ()) if sorted_ else _weights(gen, n, c.wzero, c.wnone, R)
    flat, _, o, ld = _worker_rows(gen, dtype, n, D, used, R, c.mis, c.special, nan_rows=zero)
    X = _on(dev, flat, o, R, ld)
    rows = torch.tensor(c.rows, dtype=torch.int32, device=dev) if c.rows else None
    wd = None if w is None else w.to(dev)
    hyper = _hyper(c)
    kind = hyper["kind"]
    so = GUARD + (1 if c.mis == "state" else 0)
    po = GUARD + (1 if c.mis == "pout" else 0)
    m0 = s10 = s20 = None
    mb = s1b = s2b = None
    if kind != "none":
        m0, s10, s20 = _state(gen, kind, hyper.get("first", False), D)
        mb = _guarded(m0, D, so, torch.float32, dev)
        if kind != "sgd" or hyper["momentum"]:
            s1b = _guarded(s10, D, so, torch.float32, dev)
        else:
            s10 = None
        if s20 is not None:
            s2b = _guarded(s20, D, so, torch.float32, dev)
    gb = _guarded(None, D, so, torch.float32, dev)
    pb = _guarded(None, D, po, _tdt(c.pout), dev)
    sl = lambda b, off: None if b is None else b[off:off + D]   # noqa: E731
    before = tuple(None if t is None else t.to(dev) for t in (m0, s10, s20))
    K.agg_update(X, combine="sorted" if sorted_ else "weighted", lo=lo, cnt=cnt, w=wd, rows=rows,
                 n=n, D=D, opt=K.OptArgs(gscale=c.gscale, **hyper), master=sl(mb, so),
                 s1=sl(s1b, so), s2=sl(s2b, so), param_out=sl(pb, po), gout=sl(gb, so))
    # (d) guard bands
    for name, b, off in (("master", mb, so), ("s1", s1b, so), ("s2", s2b, so), ("gout", gb, so),
                         ("param_out", pb, po)):
        if b is not None:
            assert _guards_intact(b, off, D), f"{c.id}: wrote outside {name}"
    if kind == "none":
        assert bool(torch.isnan(pb[po:po + D]).all()), f"{c.id}: OPT_NONE wrote param_out"
    check_segment(c.id, X, rows, n, D, sorted_, lo, cnt, wd, hyper, c.gscale, before,
                  (sl(mb, so), sl(s1b, so), sl(s2b, so), sl(gb, so), sl(pb, po)),
                  c.dtype == "bf16", c.special)


def run_multi_case(c: MultiCase, dev, K):
    """Build the segments of ``c`` on ``dev``, call ``K.agg_update_multi`` and check every
    segment against the oracle (never against ``K.agg_update``)."""
    gen = torch.Generator().manual_seed(c.seed)
    dtype = _tdt(c.dtype)
    n = c.n
    used = list(c.rows) if c.rows else list(range(n))
    R = c.xrows if c.rows else n + 1
    sorted_ = c.combine != "weighted"
    lo, cnt = window(c.combine, n) if sorted_ else (0, 1)
    w, zero = (None, ()) if sorted_ else _weights(gen, n, None, False, R)
    rows = torch.tensor(c.rows, dtype=torch.int32, device=dev) if c.rows else None
    wd = None if w is None else w.to(dev)
    hyper = _hyper(c)
    kind = hyper["kind"]
    # state offsets: segments on an 8-element grid with sentinel gaps between them
    offs, end = [], 0
    for i, D in enumerate(c.Ds):
        off = (end + 7) // 8 * 8 + (8 if i else 0) + (1 if i == c.misoff else 0)
        offs.append(off)
        end = off + D
    total = end
    covered = torch.zeros(total, dtype=torch.bool)
    for D, off in zip(c.Ds, offs):
        covered[off:off + D] = True
    m0, s10, s20 = _state(gen, kind, hyper.get("first", False), total)
    gap = ~covered

    def state_buf(vals):
        v = torch.full((total,), math.nan) if vals is None else vals.clone()
        v[gap] = SENT
        return _guarded(v, total, GUARD, torch.float32, dev)

    mb, s1b, gb = state_buf(m0), state_buf(s10), state_buf(None)
    s2b = state_buf(s20) if s20 is not None else None
    Xs, pbs = [], []
    for D in c.Ds:
        flat, _, o, ld = _worker_rows(gen, dtype, n, D, used, R, nan_rows=zero)
        Xs.append(_on(dev, flat, o, R, ld))
        pbs.append(_guarded(None, D, GUARD, _tdt(c.pout), dev))
    sl = lambda b: None if b is None else b[GUARD:GUARD + total]   # noqa: E731
    K.agg_update_multi([(X, D, off, pb[GUARD:GUARD + D])
                        for X, D, off, pb in zip(Xs, c.Ds, offs, pbs)],
                       combine="sorted" if sorted_ else "weighted", lo=lo, cnt=cnt, w=wd,
                       rows=rows, n=n, opt=K.OptArgs(gscale=c.gscale, **hyper), master=sl(mb),
                       s1=sl(s1b), s2=sl(s2b), gout=sl(gb))
    # (d) guard bands and the gaps between segments
    gapd = gap.to(dev)
    for name, b in (("master", mb), ("s1", s1b), ("s2", s2b), ("gout", gb)):
        if b is not None:
            assert _guards_intact(b, GUARD, total), f"{c.id}: wrote outside {name}"
            assert bool((sl(b)[gapd] == SENT).all()), f"{c.id}: wrote between segments of {name}"
    for i, (pb, D) in enumerate(zip(pbs, c.Ds)):
        assert _guards_intact(pb, GUARD, D), f"{c.id}: wrote outside param_out {i}"
    for i, (X, D, off, pb) in enumerate(zip(Xs, c.Ds, offs, pbs)):
        cut = lambda t: None if t is None else t[off:off + D]   # noqa: E731
        before = tuple(None if t is None else cut(t).to(dev) for t in (m0, s10, s20))
        check_segment(f"{c.id} seg {i} (D={D}, off={off})", X, rows, n, D, sorted_, lo, cnt, wd,
                      hyper, c.gscale, before,
                      (cut(sl(mb)), cut(sl(s1b)), cut(sl(s2b)), cut(sl(gb)), pb[GUARD:GUARD + D]),
                      c.dtype == "bf16")
