"""Exact and float64 oracles of the Gram kernels, the error bound of their fp32 accumulation, and
the case tables of ``test_gram_oracle_gpu.py`` / ``test_gram_oracle_cpu.py`` (not collected: no
``test_`` prefix). The kernels are in ``csrc/kernels/gram.hip``.

Exact oracle. ``int_rows`` draws non-zero integers in [-amax, amax]: exact in bf16 and fp32, and
so is every product. An fp32 sum of integers is exact while it stays below 2^24, whatever the
order of the adds, so for amax^2 D < 2^24 (centred: (2 amax)^2 D < 2^24, the differences reach
2 amax) every MFMA partial, every LDS fold and every fp64 reduce of the kernel is an exact integer
and G must EQUAL the int64 Gram: one dropped, doubled or misrouted column changes a diagonal entry
by at least 1. These cases are compared with ``torch.equal``.

``centered_oracle`` models the centred pass: the centre index is clamped to n - 1 and counts
positions of the *selected* rows; non-finite centre elements count as 0; x_i - x_c is formed in
fp32 and rounded once to the input dtype (bf16: round to nearest even) before it is widened to
float64; a negative centre is an uncentred pass.

Float bound. One wave of stage 1 keeps one fp32 accumulator per Gram element (per column group
when n <= 8 packs G groups into the 16 MFMA rows). A main-loop trip feeds it Q MFMAs (bf16:
16x16x32; fp32: four 16x16x4) of STEP columns each, a tail trip one STEP-column chunk, so the
accumulator of the busiest wave (wave 0 of workgroup 0) sums

    (trips_main Q + trips_tail) STEP   terms,
    trips_main = ceil((Dmain / COLS) / W),  trips_tail = ceil(ceil((D - Dmain) / STEP) / W),
    W = kGWaves * workgroups,  Dmain = floor(D / COLS) COLS,

and the workgroup then folds kGWaves * G accumulators in fp32. A term therefore passes through at
most L = (trips_main Q + trips_tail) STEP + kGWaves G fp32 adds (``chain_len``; + 1 for fp32
inputs, whose products are rounded, bf16 products being exact in fp32), and in any order of the
adds

    |G_ij - G64_ij| <= L 2^-23 sum_k |y_ik y_jk|

with the unit roundoff 2^-24 doubled as ``agg_oracle`` does (the MFMA's internal adds need not
be IEEE roundings, and L u stands for (1 + u)^L - 1). Stage 2 adds the workgroups' partials in
fp64; its 2^-53 per add disappears in that factor of two. The bound is derived, not fitted.
"""
import functools
import math

import numpy as np
import torch

# ----------------------------------------------------------------------------- kernel constants
WAVE = 64                     # kWave
G_BLOCK = 256                 # kGBlock: threads per stage-1 workgroup
G_WAVES = G_BLOCK // WAVE     # kGWaves
MAX_GRAM_BLOCKS = 1024        # kMaxGramBlocks
MAX_RED_BUCKETS = 32          # kMaxRedBuckets
RED_BLOCK = 256               # threads of gram_reduce(_multi)_kernel: the stride of its loops
SUM_BLOCKS = 64               # most workgroups of gram_sum_kernel (256 threads each)
VEC = {"bf16": 8, "f32": 4}           # GramVec<T>::vec: elements of one 16-byte lane load
STEP = {"bf16": 32, "f32": 16}        # GramVec<T>::step: columns of one load of the wave
Q_OF_TT = {1: 8, 2: 8, 3: 4, 4: 4}    # GramQ<TT>: loads in flight per lane and iteration
# launch_gram_dispatch: (largest n, TT, G), first match
LADDER = ((1, 1, 16), (2, 1, 8), (4, 1, 4), (8, 1, 2), (16, 1, 1), (32, 2, 1), (48, 3, 1),
          (64, 4, 1))
MAX_N = 64

DTYPES = ("bf16", "f32")
U2 = 2.0 ** -23               # the unit roundoff of fp32, doubled
EXACT = 2 ** 24               # integers below it are exact in fp32


def tdt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def geometry(dt, n):
    """dict(TT, G, Q, STEP, VEC, COLS, P) of the stage-1 variant that n rows of dtype dt take."""
    assert 1 <= n <= MAX_N
    TT, G = next((tt, g) for top, tt, g in LADDER if n <= top)
    q, step = Q_OF_TT[TT], STEP[dt]
    return dict(TT=TT, G=G, Q=q, STEP=step, VEC=VEC[dt], COLS=G * q * step, P=16 * TT)


def blocks(dt, n, D, grid_cap=0):
    """Stage-1 workgroups (gram_blocks, then grid_cap)."""
    per = geometry(dt, n)["COLS"] * G_WAVES
    nb = max(1, min(MAX_GRAM_BLOCKS, -(-D // per)))
    return min(nb, grid_cap) if grid_cap > 0 else nb


def trips(dt, n, D, nblocks):
    """(main-loop trips, tail trips) of wave 0 of workgroup 0, the busiest wave."""
    g = geometry(dt, n)
    W = G_WAVES * nblocks
    main = D // g["COLS"]
    chunks = -(-(D - main * g["COLS"]) // g["STEP"])
    return -(-main // W), -(-chunks // W)


def chain_len(dt, n, D, nblocks):
    """Most fp32 adds a term of one Gram element passes through (see the module docstring)."""
    g = geometry(dt, n)
    tm, tt = trips(dt, n, D, nblocks)
    return (tm * g["Q"] + tt) * g["STEP"] + G_WAVES * g["G"] + (1 if dt == "f32" else 0)


def amax_for(D, centered, cap=100):
    """Largest amax <= cap for which the integer Gram of D columns is exact in fp32."""
    a = math.isqrt((EXACT - 1) // D)
    a = a // 2 if centered else a
    assert a >= 1, f"no exact integer data at D={D}"
    return min(a, cap)


def assert_exact(amax, D, centered):
    m = 2 * amax if centered else amax
    assert m * m * D < EXACT and m <= 256, f"amax={amax} D={D} centered={centered} is not exact"


# ----------------------------------------------------------------------------- data and oracles
@functools.lru_cache(maxsize=64)
def int_rows(n, D, dt, seed, amax):
    """[n, D] non-zero integers in [-amax, amax] in dtype dt (CPU). Shared: treat as read-only."""
    assert 1 <= amax <= 256
    gen = torch.Generator().manual_seed(7919 * seed + 31 * n + D % 1009)
    v = torch.randint(1, amax + 1, (n, D), generator=gen)
    s = torch.randint(0, 2, (n, D), generator=gen) * 2 - 1
    return (v * s).to(tdt(dt))


def int_case(dt, n, D, centered, seed=0):
    """``int_rows`` at the largest amax that keeps the case exact (asserted)."""
    amax = amax_for(D, centered)
    assert_exact(amax, D, centered)
    return int_rows(n, D, dt, seed, amax)


def _center_row(X, c):
    """Row c of X with its non-finite elements counted as 0 (fp32)."""
    xc = X[c].float()
    return torch.where(torch.isfinite(xc), xc, torch.zeros_like(xc))


def centered_rows(X, c=None, rows=None):
    """float64 [n, D]: the rows the kernel multiplies (see the module docstring). X is bf16 or
    fp32 on the CPU; ``rows`` selects (and may repeat) rows first; c: int or None."""
    Xs = X if rows is None else X[torch.as_tensor(rows, dtype=torch.long)]
    if c is None or c < 0:
        return Xs.double()
    c = min(int(c), Xs.shape[0] - 1)
    return (Xs.float() - _center_row(Xs, c)).to(X.dtype).double()


def centered_oracle(X, c=None, rows=None):
    """float64 Gram of ``centered_rows``."""
    Y = centered_rows(X, c, rows)
    return Y @ Y.t()


def exact_gram(X, c=None, rows=None):
    """The exact Gram of integer rows (float64 [n, n]). The float64 product is the int64 one:
    every partial sum is an integer below 2^24 < 2^53."""
    Y = centered_rows(X, c, rows)
    assert torch.equal(Y.long().double(), Y), "exact_gram is for integer data"
    G = Y @ Y.t()
    assert float(G.diagonal().max()) < EXACT
    return G


def bound(X, dt, n, D, nblocks, c=None, rows=None):
    """(G64, elementwise bound) of float data."""
    Y = centered_rows(X, c, rows)
    return Y @ Y.t(), chain_len(dt, n, D, nblocks) * U2 * (Y.abs() @ Y.abs().t())


def poisoned(Xw, extra_rows=3, dev=None, rows=None):
    """Xw [n, D] inside a NaN buffer that is wider and taller, as the engine's bucket windows are:
    [n + extra_rows, D_alloc], D_alloc the next multiple of 8 above D + 24. ``rows``: the buffer
    rows that take Xw's rows (default 0 .. n - 1)."""
    n, D = Xw.shape
    tall = n + extra_rows if rows is None else max(rows) + 1 + extra_rows
    big = torch.full((tall, (D + 24) // 8 * 8 + 8), math.nan, dtype=Xw.dtype)
    big[list(range(n)) if rows is None else list(rows), :D] = Xw
    return big if dev is None else big.to(dev)


def center_arg(c, dev):
    return None if c is None else torch.tensor([c], dtype=torch.int32, device=dev)


# ----------------------------------------------------------------------------- case tables
ALL_NS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64)
CROSS = [(dt, n, cen) for dt in DTYPES for n in ALL_NS for cen in (False, True)]


def cross_ds(dt, n):
    """[(D, grid_cap)] of the dispatch x size cross. The last D runs twice: as launched (two
    workgroups, W = 8: the six tail chunks take one trip) and under grid_cap = 1 (W = 4: the tail's
    second trip, ending ragged; where COLS = 4 STEP, TT >= 3, a tail has at most 4 chunks and no
    second trip exists: there wave 0 takes a second main-loop trip instead)."""
    g = geometry(dt, n)
    v, s, c = g["VEC"], g["STEP"], g["COLS"]
    last = 4 * c + 5 * s + 3
    ds = [1, v - 1, v, v + 1, s - 1, s, s + 1, c - 1, c, c + 1, 4 * c, last]
    return [(D, 0) for D in ds] + [(last, 1)]


def rotate_center(n, k):
    """Centre of the k-th centred launch of a case: 0, n - 1, a middle row, ..."""
    return (0, n - 1, n // 2)[k % 3]


TRIP_NS = (1, 3, 8, 16, 32, 48, 64)
TRIP_CAPS = (1, 2)
TRIPS = [(dt, n, cen) for dt in DTYPES for n in TRIP_NS for cen in (False, True)]


def trip_ds(dt, n, cap):
    """Three full main-loop trips and a ragged tail (TT >= 3, COLS = 4 STEP: its five chunks hold
    one more COLS, a fourth trip of wave 0); two and a third that only wave 0 of workgroup 0 takes."""
    g = geometry(dt, n)
    W = G_WAVES * cap
    return (3 * W * g["COLS"] + 5 * g["STEP"] + 3, 2 * W * g["COLS"] + g["COLS"] + 1)


CAP_N, CAP_AMAX = 64, 2


def natural_cap_d(dt):
    """Two trips of every wave of the real launch at its 1024-workgroup cap, a third of wave 0
    alone and a ragged rest."""
    c = geometry(dt, CAP_N)["COLS"]
    return 2 * MAX_GRAM_BLOCKS * G_WAVES * c + c + 5


ROWS_NS = (3, 8, 17, 33, 64)
ACC_NS = (8, 17, 33, 64)
NONFINITE_NS = (3, 8, 17, 64)
FLOAT_NS = (3, 8, 16, 33, 64)
MULTI_NS = (16, 17, 33, 48, 49, 64)
MULTI_BUCKETS = (1, 2, MAX_RED_BUCKETS)
SUM_R = 129                   # E = 16641 > 64 * 256: gram_sum_kernel's loop takes a second trip
SUM_NB = (1, 5)
CENTER_NS = (1, 2, 17, 64)


def acc_widths(dt, n):
    """Three unequal slice widths, none a multiple of STEP."""
    g = geometry(dt, n)
    return (g["COLS"] + g["STEP"] + 5, 3, 2 * g["COLS"] + g["VEC"] + 1)


def nonfinite_d(dt, n):
    g = geometry(dt, n)
    return g["COLS"] + g["STEP"] + 3


def nonfinite_cols(dt, n):
    """Columns of the main loop (last column group), of the tail, and D - 1 in a partial vector."""
    g = geometry(dt, n)
    return {"main": g["COLS"] - 3, "tail": g["COLS"] + 2, "last": nonfinite_d(dt, n) - 1}


def nonfinite_kinds(dt):
    return ("nan", "inf", "neg_inf") + (("neg_nan_bits",) if dt == "bf16" else ())


def put_bad(X, i, col, kind):
    """Set X[i, col] (in place) to the non-finite value ``kind``."""
    if kind == "neg_nan_bits":
        assert X.dtype == torch.bfloat16
        X.view(torch.int16)[i, col] = -64          # 0xFFC0
    else:
        X[i, col] = {"nan": math.nan, "inf": math.inf, "neg_inf": -math.inf}[kind]


def float_d(dt, n):
    g = geometry(dt, n)
    return 4 * g["COLS"] + g["STEP"] + 3


@functools.lru_cache(maxsize=32)
def float_rows(kind, n, D, dt, seed=0):
    """(X, centre) of float data in dtype dt. "scaled": N(0, 1) rows scaled 1 .. n, centre
    rotating with n. "cluster": base + 0.01 noise around a common base with the centre row (n // 2)
    of a very different magnitude, so that the single rounding of x_i - x_c matters."""
    gen = torch.Generator().manual_seed(104729 * seed + 17 * n + D % 1013)
    if kind == "scaled":
        X = torch.randn(n, D, generator=gen) * torch.arange(1, n + 1)[:, None]
        c = rotate_center(n, n)
    else:
        assert kind == "cluster", kind
        X = torch.randn(D, generator=gen)[None] + 0.01 * torch.randn(n, D, generator=gen)
        c = n // 2
        X[c] = 300.0 * torch.randn(D, generator=gen)
    return X.to(tdt(dt)), c


def multi_ds(dt, n, nb):
    """Column counts of nb buckets; with two buckets the first has more than RED_BLOCK partial
    workgroups (the reduce's stride loop takes a second trip)."""
    g = geometry(dt, n)
    small = [g["COLS"] + (3 + 5 * b) % g["STEP"] + g["STEP"] * (b % 3) for b in range(nb)]
    if nb == 2:
        small[0] = (RED_BLOCK + 1) * G_WAVES * g["COLS"] + g["STEP"] + 3
    return small


def rows_case(n):
    """(buffer rows that hold X's rows, the ``rows`` argument, the same selection as indices of
    X): X's rows scattered over a taller buffer in reverse order with gaps, and a ``rows`` that is
    a permutation of them with one index repeated."""
    phys = [2 * (n - 1 - i) + 1 for i in range(n)]
    sel = [(3 * k + 1) % n for k in range(n)] if n % 3 else [(k + 1) % n for k in range(n)]
    assert sorted(sel) == list(range(n))
    sel[1] = sel[0]
    return phys, [phys[i] for i in sel], sel


def center_cases(n):
    """[(name, G fp64 [n, n], expected medoid or None for "what the reference says")]: Grams of
    integer rows, so every score is exact and ties are exact ties."""
    from consensusml_amd.ops import reference as R
    X = int_rows(n, 40, "f32", 5, 9).clone()
    cases = [("random", exact_gram(X), None)]
    if n >= 4:
        Xt = X.clone()
        Xt[1::2] = Xt[0:n - 1:2]                         # rows 2k + 1 = rows 2k: pairwise ties
        if n % 2:
            Xt[n - 1] *= 9                               # the row without a twin: far away
        G = exact_gram(Xt)
        w = R.gram_center(G)
        assert w % 2 == 0 and w + 1 < n and torch.equal(Xt[w], Xt[w + 1])
        cases.append(("ties", G, w))                     # the lower row of the tied pair
        Gn = G.clone()
        Gn[w, w] = math.nan
        cases.append(("nonfinite_winner", Gn, None))
        Gi = G.clone()
        Gi[w, w], Gi[w + 1, w + 1] = math.inf, -math.inf
        cases.append(("nonfinite_pair", Gi, None))
    else:
        cases.append(("ties", exact_gram(X[:1].expand(n, -1).contiguous()), 0))
    Gall = exact_gram(X)
    Gall.diagonal().fill_(math.nan)
    cases.append(("all_nonfinite", Gall, 0))
    return cases


def check_center(K, dev, n):
    """``K.gram_center`` on ``dev`` against ``reference.gram_center`` over ``center_cases`` and
    on the (n + 1)^2 Gram of centred clipping."""
    from consensusml_amd.ops import reference as R
    for name, G, want in center_cases(n):
        ref = R.gram_center(G)
        assert want is None or ref == want, name
        out = K.gram_center(G.to(dev), n)
        assert out.dtype == torch.int32 and int(out[0]) == ref, (name, int(out[0]), ref)
        if name.startswith("nonfinite"):
            assert math.isfinite(float(G[ref, ref])), name
    # the (n + 1)^2 Gram: the medoid of its n x n block, whatever row n holds
    for seed in (6, 7, 8, 9):
        X = int_rows(n, 40, "f32", seed, 9)
        X1 = torch.cat([X, 50.0 * torch.ones(1, 40)])
        if n >= 3 and seed % 2:
            X1[n] = X[R.gram_center(exact_gram(X)) - 1]  # row n: a copy of a non-medoid row
        G1 = exact_gram(X1)
        got = int(K.gram_center(G1.to(dev), n)[0])
        assert got == R.gram_center(G1[:n, :n]), (seed, got)


# ----------------------------------------------------------------------------- fp32 emulation
def emulate(Y, dt, n, nblocks, drop=None):
    """The kernel's arithmetic on the float64 rows Y (already centred and rounded): every wave's
    (and column group's) accumulator summed sequentially in float32 over its own columns, the
    workgroup's fold in float32, the workgroups in float64. ``drop``: index of one STEP-wide
    chunk of wave 0's first main-loop trip to leave out. Returns float64 [n, n]."""
    g = geometry(dt, n)
    D = Y.shape[1]
    y = Y.numpy().astype(np.float32)
    assert np.array_equal(y.astype(np.float64), Y.numpy())
    cols, step, gspan = g["COLS"], g["STEP"], g["Q"] * g["STEP"]
    W = G_WAVES * nblocks
    dmain = D // cols * cols
    total = np.zeros((n, n), dtype=np.float64)
    for b in range(nblocks):
        fold = np.zeros((n, n), dtype=np.float32)
        for w in range(G_WAVES):
            gw = b * G_WAVES + w
            for grp in range(g["G"]):
                ks = []
                for k0 in range(gw * cols, dmain, W * cols):
                    for q in range(g["Q"]):
                        lo = k0 + grp * gspan + q * step
                        if drop is not None and gw == 0 and k0 == 0 and grp * g["Q"] + q == drop:
                            continue
                        ks.extend(range(lo, lo + step))
                if grp == 0:
                    for k0 in range(dmain + gw * step, D, W * step):
                        ks.extend(range(k0, min(k0 + step, D)))
                acc = np.zeros((n, n), dtype=np.float32)
                for k in ks:
                    acc = acc + np.outer(y[:, k], y[:, k])      # float32 product and add
                fold = fold + acc
        total += fold.astype(np.float64)
    return torch.from_numpy(total)
