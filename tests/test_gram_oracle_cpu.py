"""The Gram oracle's tables against the launch constants of ``csrc/kernels/gram.hip``, the CPU
branch of ``K.gram`` / ``K.gram_center`` / ``K.gram_sum`` over the case tables of
``test_gram_oracle_gpu.py``, the float bound against a float32 emulation of the kernel's
summation, and the two wrapper fixes."""
import math
import os
import re

import pytest
import torch

import gram_oracle as GR
from consensusml_amd.ops import kernels as K

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    with open(os.path.join(ROOT, "csrc", "kernels", name)) as fh:
        return fh.read()


def test_constants_table():
    """The constants and the n -> (TT, G) ladder of gram.hip are the ones gram_oracle.py states,
    and the case tables stand for what they say."""
    src = _src("gram.hip")
    const = lambda name, text=src: int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))  # noqa: E731
    assert const("kWave", _src("common.h")) == GR.WAVE
    assert const("kGBlock") == GR.G_BLOCK
    assert re.search(r"constexpr int kGWaves = kGBlock / kWave;", src)
    assert const("kMaxGramBlocks") == GR.MAX_GRAM_BLOCKS
    assert const("kMaxRedBuckets") == GR.MAX_RED_BUCKETS
    for ctype, dt in (("bf16", "bf16"), ("float", "f32")):
        m = re.search(rf"struct GramVec<{ctype}> {{ static constexpr int vec = (\d+), step = (\d+); }};", src)
        assert (int(m.group(1)), int(m.group(2))) == (GR.VEC[dt], GR.STEP[dt])
        assert GR.STEP[dt] == 4 * GR.VEC[dt] and GR.VEC[dt] * (2 if dt == "bf16" else 4) == 16
    m = re.search(r"struct GramQ { static constexpr int value = TT <= (\d+) \? (\d+) : (\d+); };", src)
    top, lo, hi = (int(v) for v in m.groups())
    assert {tt: lo if tt <= top else hi for tt in (1, 2, 3, 4)} == GR.Q_OF_TT
    assert re.search(r"return G \* GramQ<TT>::value \* GramVec<T>::step;", src)
    ladder = re.findall(r"if \(n (==|<=) (\d+)\) return launch_gram_t<T, (\d+), (\d+)>", src)
    last = re.search(r"\n  return launch_gram_t<T, (\d+), (\d+)>", src)
    got = [(int(n), int(tt), int(g)) for _, n, tt, g in ladder]
    got.append((GR.MAX_N, int(last.group(1)), int(last.group(2))))
    assert tuple(got) == GR.LADDER
    assert re.search(rf"n < 1 \|\| n > {GR.MAX_N} ", src)
    # the reduce kernels stride their partials by their 256 threads; gram_sum by 64 x 256
    assert len(re.findall(r"<<<P \* P, 256, 0, st", src)) == 2 and GR.RED_BLOCK == 256
    assert re.search(rf"if \(blocks > {GR.SUM_BLOCKS}\) blocks = {GR.SUM_BLOCKS};", src)
    assert GR.SUM_R ** 2 > GR.SUM_BLOCKS * 256

    # what the tables stand for
    seen = set()
    for dt in GR.DTYPES:
        for n in GR.ALL_NS:
            g = GR.geometry(dt, n)
            seen.add((g["TT"], g["G"]))
            assert 16 * g["TT"] >= n and (g["G"] == 1 or 16 // g["G"] >= n)
            ds = GR.cross_ds(dt, n)
            assert all(GR.blocks(dt, n, D) == 1 for D, _ in ds[:-2])
            (D, cap0), (D1, cap1) = ds[-2:]
            assert D == D1 and (cap0, cap1) == (0, 1)
            assert GR.blocks(dt, n, D) == 2 and GR.trips(dt, n, D, 2) == (1, 1)
            # (TT >= 3: COLS = 4 STEP, the tail never holds more chunks than one workgroup has
            # waves and has no second trip to take; the five chunks then make a fifth COLS)
            assert GR.trips(dt, n, D, GR.blocks(dt, n, D, 1)) == ((1, 2) if g["TT"] <= 2 else (2, 1))
            assert D % g["VEC"] != 0
        for n in GR.TRIP_NS:
            for cap in GR.TRIP_CAPS:
                full, one = GR.trip_ds(dt, n, cap)
                assert GR.blocks(dt, n, full, cap) == cap == GR.blocks(dt, n, one, cap)
                tt = GR.geometry(dt, n)["TT"]    # (TT >= 3: the five chunks make one more COLS)
                assert GR.trips(dt, n, full, cap)[0] == (3 if tt <= 2 else 4)
                assert GR.trips(dt, n, one, cap)[0] == 3
                assert (one // GR.geometry(dt, n)["COLS"]) % (GR.G_WAVES * cap) == 1
        D = GR.natural_cap_d(dt)
        assert GR.blocks(dt, GR.CAP_N, D) == GR.MAX_GRAM_BLOCKS > GR.RED_BLOCK
        # two trips of every wave, a third of wave 0 alone, five columns of tail
        assert GR.trips(dt, GR.CAP_N, D, GR.MAX_GRAM_BLOCKS) == (3, 1)
        GR.assert_exact(GR.CAP_AMAX, D, False)
        for n in GR.MULTI_NS:
            assert GR.blocks(dt, n, GR.multi_ds(dt, n, 2)[0]) > GR.RED_BLOCK
        for n in GR.ACC_NS:
            assert all(w % GR.STEP[dt] for w in GR.acc_widths(dt, n))
        for n in GR.NONFINITE_NS:
            g, cols, D = GR.geometry(dt, n), GR.nonfinite_cols(dt, n), GR.nonfinite_d(dt, n)
            assert cols["main"] < g["COLS"] <= cols["tail"] < D - 1 == cols["last"]
            assert cols["main"] // (g["Q"] * g["STEP"]) == g["G"] - 1 and D % g["VEC"] != 0
    assert seen == {(tt, g) for _, tt, g in GR.LADDER}
    # both sides of every switch of the ladder
    assert {m for n, _, _ in GR.LADDER for m in (n, n + 1) if m <= GR.MAX_N} <= set(GR.ALL_NS)


# ----------------------------------------------------------------------------- CPU branch
@pytest.mark.parametrize("dt,n,cen", GR.CROSS, ids=[f"{dt}-n{n}-{'c' if c else 'u'}" for dt, n, c in GR.CROSS])
def test_cpu_branch_cross(dt, n, cen):
    for k, (D, cap) in enumerate(GR.cross_ds(dt, n)):
        X = GR.int_case(dt, n, D, cen)
        c = GR.rotate_center(n, k) if cen else None
        G = K.gram(GR.poisoned(X), n=n, D=D, center=GR.center_arg(c, CPU), grid_cap=cap)
        assert G.dtype == torch.float64 and tuple(G.shape) == (n, n)
        assert torch.equal(G, GR.exact_gram(X, c)), (D, c)


@pytest.mark.parametrize("dt,n,cen", GR.TRIPS, ids=[f"{dt}-n{n}-{'c' if c else 'u'}" for dt, n, c in GR.TRIPS])
def test_cpu_branch_trips(dt, n, cen):
    for cap in GR.TRIP_CAPS:
        for k, D in enumerate(GR.trip_ds(dt, n, cap)):
            X = GR.int_case(dt, n, D, cen)
            c = GR.rotate_center(n, k + cap) if cen else None
            G = K.gram(GR.poisoned(X), n=n, D=D, center=GR.center_arg(c, CPU), grid_cap=cap)
            assert torch.equal(G, GR.exact_gram(X, c)), (cap, D, c)


@pytest.mark.parametrize("dt", GR.DTYPES)
def test_cpu_branch_natural_cap(dt):
    D = GR.natural_cap_d(dt)
    X = GR.int_rows(GR.CAP_N, D, dt, 1, GR.CAP_AMAX)
    Xd = X.double()
    assert torch.equal(K.gram(X), Xd @ Xd.t())


@pytest.mark.parametrize("dt", GR.DTYPES)
@pytest.mark.parametrize("n", GR.ROWS_NS)
def test_cpu_branch_rows_and_center(dt, n):
    D = GR.geometry(dt, n)["COLS"] + GR.STEP[dt] + 3
    X = GR.int_case(dt, n, D, True)
    phys, rows, sel = GR.rows_case(n)
    big = GR.poisoned(X, rows=phys)
    r = torch.tensor(rows, dtype=torch.int32)
    plain = K.gram(big, rows=r, D=D)
    assert torch.equal(plain, GR.exact_gram(X, None, sel))
    assert torch.equal(K.gram(big, rows=r, D=D, center=GR.center_arg(-1, CPU)), plain)
    for c in (0, n - 1, n // 2, n, n + 7):
        G = K.gram(big, rows=r, D=D, center=GR.center_arg(c, CPU))
        assert torch.equal(G, GR.exact_gram(X, c, sel)), c


@pytest.mark.parametrize("dt", GR.DTYPES)
@pytest.mark.parametrize("n", GR.ACC_NS)
def test_cpu_branch_accumulate(dt, n):
    widths = GR.acc_widths(dt, n)
    X = GR.int_case(dt, n, sum(widths), False)
    out = torch.zeros(n, n, dtype=torch.float64)
    s = 0
    for w in widths:
        assert K.gram(X[:, s:s + w], out=out, accumulate=True) is out
        s += w
    assert torch.equal(out, GR.exact_gram(X))
    assert K.gram(X, out=out) is out and torch.equal(out, GR.exact_gram(X))


@pytest.mark.parametrize("dt", GR.DTYPES)
@pytest.mark.parametrize("n", GR.NONFINITE_NS)
def test_cpu_branch_nonfinite(dt, n):
    """A non-finite element in row i leaves every G_jl, j, l != i, exact; a non-finite element of
    the centre row counts as 0."""
    D = GR.nonfinite_d(dt, n)
    X = GR.int_case(dt, n, D, True)
    for i in (0, n - 1):
        keep = torch.ones(n, dtype=torch.bool)
        keep[i] = False
        for kind in GR.nonfinite_kinds(dt):
            for col in GR.nonfinite_cols(dt, n).values():
                Xb = X.clone()
                GR.put_bad(Xb, i, col, kind)
                for c in (None, 1):
                    G = K.gram(Xb, center=GR.center_arg(c, CPU))
                    assert torch.equal(G[keep][:, keep], GR.exact_gram(X, c)[keep][:, keep])
                    assert not math.isfinite(float(G[i, i]))
    c = n // 2
    Xb = X.clone()
    Xb[c, 1], Xb[c, D - 1] = math.nan, math.inf
    keep = torch.ones(n, dtype=torch.bool)
    keep[c] = False
    G = K.gram(Xb, center=GR.center_arg(c, CPU))
    assert torch.equal(G[keep][:, keep], GR.centered_oracle(Xb, c)[keep][:, keep])
    assert not math.isfinite(float(G[c, c]))


@pytest.mark.parametrize("dt", GR.DTYPES)
@pytest.mark.parametrize("kind", ["scaled", "cluster"])
def test_cpu_branch_float(dt, kind):
    """Float data: the CPU branch is the float64 Gram; centred, it differs from the kernel's model
    by the rounding of x_i - x_c alone (it subtracts in float64)."""
    for n in GR.FLOAT_NS:
        X, c = GR.float_rows(kind, n, GR.float_d(dt, n), dt)
        torch.testing.assert_close(K.gram(X), GR.centered_oracle(X), rtol=1e-13, atol=0)
        Y = X.double() - X[c].double()
        torch.testing.assert_close(K.gram(X, center=GR.center_arg(c, CPU)), Y @ Y.t(),
                                   rtol=1e-13, atol=0)


@pytest.mark.parametrize("nb", GR.SUM_NB)
def test_cpu_branch_gram_sum(nb):
    gen = torch.Generator().manual_seed(nb)
    Gb = torch.randn(nb, GR.SUM_R, GR.SUM_R, generator=gen, dtype=torch.float64)
    out = torch.full((GR.SUM_R, GR.SUM_R), math.nan, dtype=torch.float64)
    want = Gb[0].clone()
    for b in range(1, nb):
        want = want + Gb[b]
    assert K.gram_sum(Gb, out) is out and torch.equal(out, want)


@pytest.mark.parametrize("n", GR.CENTER_NS)
def test_cpu_branch_gram_center(n):
    GR.check_center(K, CPU, n)


# ----------------------------------------------------------------------------- the bound
@pytest.mark.parametrize("dt", GR.DTYPES)
@pytest.mark.parametrize("n", [3, 33])
def test_bound_holds_for_an_fp32_emulation_and_sees_a_dropped_chunk(dt, n):
    D = GR.float_d(dt, n)
    nblk = GR.blocks(dt, n, D)
    assert nblk == 2 and GR.trips(dt, n, D, nblk) == (1, 1)
    g = GR.geometry(dt, n)
    assert GR.chain_len(dt, n, D, nblk) == (g["Q"] + 1) * g["STEP"] + 4 * g["G"] + (dt == "f32")
    for kind in ("scaled", "cluster"):
        X, c = GR.float_rows(kind, n, D, dt)
        for cc in (None, c):
            G64, bnd = GR.bound(X, dt, n, D, nblk, cc)
            Y = GR.centered_rows(X, cc)
            err = (GR.emulate(Y, dt, n, nblk) - G64).abs()
            assert bool((err <= bnd).all()), float((err / bnd.clamp_min(1e-300)).max())
            assert float(err.max()) > 0, "the emulation rounds: the bound is not vacuous"
            for drop in (0, g["G"] * g["Q"] - 1):
                bad = (GR.emulate(Y, dt, n, nblk, drop=drop) - G64).abs()
                assert bool((bad > bnd).any()), (kind, cc, drop)


# ----------------------------------------------------------------------------- wrapper fixes
def test_accumulate_needs_out():
    X = torch.ones(3, 16)
    with pytest.raises(ValueError, match="accumulate needs out"):
        K.gram(X, accumulate=True)


def test_gram_center_of_a_larger_gram_takes_the_block():
    GR.check_center(K, CPU, 17)
