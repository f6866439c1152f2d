"""The Gram kernels of ``csrc/kernels/gram.hip`` over their dispatch space against the oracles of
``gram_oracle.py``: integer data must give the int64 Gram bit for bit (``torch.equal``), float
data must stay inside the derived elementwise bound. Not covered: D beyond 2^31 columns (tens of
GB; it would not run in seconds)."""
import math

import pytest
import torch

import gram_oracle as GR
from consensusml_amd.ops import kernels as K

pytestmark = pytest.mark.gpu


def _cid(dt, n, cen):
    return f"{dt}-n{n}-{'c' if cen else 'u'}"


def _windowed(cuda, X, c=None, grid_cap=0):
    """K.gram on the [:n, :D] window of a NaN buffer (the engine's call)."""
    n, D = X.shape
    return K.gram(GR.poisoned(X, dev=cuda), n=n, D=D, center=GR.center_arg(c, cuda),
                  grid_cap=grid_cap).cpu()


# ----------------------------------------------------------------------------- a. dispatch x size
@pytest.mark.parametrize("dt,n,cen", GR.CROSS, ids=[_cid(*c) for c in GR.CROSS])
def test_dispatch_size_cross(cuda, dt, n, cen):
    for k, (D, cap) in enumerate(GR.cross_ds(dt, n)):
        X = GR.int_case(dt, n, D, cen)
        c = GR.rotate_center(n, k) if cen else None
        G = _windowed(cuda, X, c, cap)
        assert G.dtype == torch.float64 and tuple(G.shape) == (n, n)
        assert torch.equal(G, GR.exact_gram(X, c)), f"D={D} grid_cap={cap} center={c}"


# ----------------------------------------------------------------------------- b. multi-trip loop
@pytest.mark.parametrize("dt,n,cen", GR.TRIPS, ids=[_cid(*c) for c in GR.TRIPS])
def test_main_loop_trips(cuda, dt, n, cen):
    for cap in GR.TRIP_CAPS:
        for k, D in enumerate(GR.trip_ds(dt, n, cap)):
            X = GR.int_case(dt, n, D, cen)
            c = GR.rotate_center(n, k + cap) if cen else None
            G = _windowed(cuda, X, c, cap)
            assert torch.equal(G, GR.exact_gram(X, c)), f"D={D} grid_cap={cap} center={c}"


def _partials(cuda, Xs, n, c=None, grid_cap=0):
    """gram_partial of every bucket into a workspace of its own, then one gram_reduce_multi."""
    from consensusml_amd.ops.native import lib
    per = max(lib().gram_workspace_bytes(n, X.shape[1]) for X in Xs) // 4
    pool = torch.full((len(Xs), per), math.nan, dtype=torch.float32, device=cuda)
    works, nblks = [], []
    for b, X in enumerate(Xs):
        D = X.shape[1]
        works.append(pool[b])
        nblks.append(lib().gram_partial(GR.poisoned(X, dev=cuda), n, D, pool[b],
                                        GR.center_arg(c, cuda), grid_cap))
    G = torch.full((n, n), math.nan, dtype=torch.float64, device=cuda)
    lib().gram_reduce_multi(works, nblks, n, G)
    return G.cpu(), nblks


@pytest.mark.parametrize("dt", GR.DTYPES)
def test_partial_trips_under_grid_cap(cuda, dt):
    n, cap = 17, 1
    Xs = [GR.int_case(dt, n, D, True, seed=3 + b) for b, D in enumerate(GR.trip_ds(dt, n, cap))]
    for c in (None, 5):
        G, nblks = _partials(cuda, Xs, n, c, grid_cap=cap)
        assert nblks == [cap, cap]
        assert torch.equal(G, sum(GR.exact_gram(X, c) for X in Xs))


# ----------------------------------------------------------------------------- c. the natural cap
@pytest.mark.parametrize("dt", GR.DTYPES)
def test_natural_block_cap(cuda, dt):
    """The real launch at 1024 workgroups: every wave's second trip, wave 0's third, and the
    second trip (nblk > 256) of gram_reduce_kernel. The reference is the device's float64 matmul,
    exact for these integers."""
    n, D = GR.CAP_N, GR.natural_cap_d(dt)
    GR.assert_exact(GR.CAP_AMAX, D, False)
    gen = torch.Generator(device=cuda).manual_seed(12)
    X = torch.full((n, (D + 24) // 8 * 8 + 8), math.nan, dtype=GR.tdt(dt), device=cuda)
    v = torch.randint(1, GR.CAP_AMAX + 1, (n, D), generator=gen, device=cuda)
    s = torch.randint(0, 2, (n, D), generator=gen, device=cuda) * 2 - 1
    X[:, :D] = (v * s).to(X.dtype)
    del v, s
    G = K.gram(X, D=D)
    Xd = X[:, :D].double()
    want = Xd @ Xd.t()
    assert float(want.diagonal().min()) >= D and float(want.max()) < GR.EXACT
    assert torch.equal(G, want)


# ----------------------------------------------------------------------------- d. alignment
@pytest.mark.parametrize("dt", GR.DTYPES)
@pytest.mark.parametrize("n", [3, 17])
def test_alignment_and_stride(cuda, dt, n):
    D = GR.geometry(dt, n)["COLS"] + GR.STEP[dt] + 3
    X = GR.int_case(dt, n, D, False)
    want = GR.exact_gram(X)
    pad = lambda w: torch.full((n, w), math.nan, dtype=X.dtype)  # noqa: E731
    # an aligned base inside a wider buffer: ld > D, no copy
    big = torch.cat([pad(8), X, pad(13)], 1).to(cuda)
    assert big[:, 8:].data_ptr() % 16 == 0 and (big.stride(0) * big.element_size()) % 16 == 0
    assert torch.equal(K.gram(big[:, 8:], D=D).cpu(), want)
    # a misaligned base: the wrapper's copy + pad
    big = torch.cat([pad(1), X, pad(15)], 1).to(cuda)
    assert big[:, 1:].data_ptr() % 16 != 0
    assert torch.equal(K.gram(big[:, 1:], D=D).cpu(), want)
    assert torch.equal(K.gram(big[:, 1:D + 1]).cpu(), want)
    # a row stride that is no multiple of 16 bytes
    big = torch.cat([X, pad(1 if D % 2 == 0 else 2)], 1).to(cuda)
    assert (big.stride(0) * big.element_size()) % 16 != 0
    assert torch.equal(K.gram(big, D=D).cpu(), want)
    c = GR.center_arg(n - 1, cuda)
    assert torch.equal(K.gram(big, D=D, center=c).cpu(), GR.exact_gram(X, n - 1))
    # a 1-D X is one row
    g1 = K.gram(X[n - 1].to(cuda))
    assert tuple(g1.shape) == (1, 1) and torch.equal(g1.cpu(), want[n - 1:, n - 1:])


# ----------------------------------------------------------------------------- e. rows
@pytest.mark.parametrize("dt", GR.DTYPES)
@pytest.mark.parametrize("n", GR.ROWS_NS)
def test_rows_and_center(cuda, dt, n):
    D = GR.geometry(dt, n)["COLS"] + GR.STEP[dt] + 3
    X = GR.int_case(dt, n, D, True)
    phys, rows, sel = GR.rows_case(n)
    big = GR.poisoned(X, rows=phys, dev=cuda)
    r = torch.tensor(rows, dtype=torch.int32, device=cuda)
    plain = K.gram(big, rows=r, D=D).cpu()
    assert tuple(plain.shape) == (n, n) and torch.equal(plain, GR.exact_gram(X, None, sel))
    neg = K.gram(big, rows=r, D=D, center=GR.center_arg(-1, cuda)).cpu()
    assert torch.equal(neg.view(torch.int64), plain.view(torch.int64)), "a negative centre"
    for c in (0, n - 1, n // 2, n, n + 7):           # positions in rows; >= n clamps to n - 1
        G = K.gram(big, rows=r, D=D, center=GR.center_arg(c, cuda)).cpu()
        assert torch.equal(G, GR.exact_gram(X, c, sel)), c


# ----------------------------------------------------------------------------- f. accumulate
@pytest.mark.parametrize("dt", GR.DTYPES)
@pytest.mark.parametrize("n", GR.ACC_NS)
def test_accumulate_slices(cuda, dt, n):
    widths = GR.acc_widths(dt, n)
    X = GR.int_case(dt, n, sum(widths), False)
    # the slices at 16-byte aligned offsets of one NaN buffer, gaps between them
    offs, end = [], 0
    for w in widths:
        offs.append(end)
        end = (end + w + 15) // 8 * 8
    big = torch.full((n + 2, end + 8), math.nan, dtype=X.dtype)
    s = 0
    for o, w in zip(offs, widths):
        big[:n, o:o + w] = X[:, s:s + w]
        s += w
    big = big.to(cuda)
    out = torch.zeros(n, n, dtype=torch.float64, device=cuda)
    for o, w in zip(offs, widths):
        assert K.gram(big[:, o:], n=n, D=w, out=out, accumulate=True) is out
    assert torch.equal(out.cpu(), GR.exact_gram(X))
    # and without accumulate the same buffer is overwritten, mirror included
    assert K.gram(big[:, offs[1]:], n=n, D=widths[1], out=out) is out
    s = widths[0]
    assert torch.equal(out.cpu(), GR.exact_gram(X[:, s:s + widths[1]]))


# ----------------------------------------------------------------------------- g. non-finite
@pytest.mark.parametrize("cen", [False, True], ids=["u", "c"])
@pytest.mark.parametrize("dt", GR.DTYPES)
@pytest.mark.parametrize("n", GR.NONFINITE_NS)
def test_nonfinite_isolation(cuda, dt, n, cen):
    """A non-finite element of row i makes G_ii non-finite and leaves every G_jl, j, l != i, the
    exact value (nothing is said about the rest of row and column i)."""
    D = GR.nonfinite_d(dt, n)
    X = GR.int_case(dt, n, D, True)
    c = 1 if cen else None
    want = GR.exact_gram(X, c)
    for i in (0, n - 1):
        keep = torch.ones(n, dtype=torch.bool)
        keep[i] = False
        for kind in GR.nonfinite_kinds(dt):
            for where, col in GR.nonfinite_cols(dt, n).items():
                Xb = X.clone()
                GR.put_bad(Xb, i, col, kind)
                G = _windowed(cuda, Xb, c)
                assert torch.equal(G[keep][:, keep], want[keep][:, keep]), (i, kind, where)
                assert not math.isfinite(float(G[i, i])), (i, kind, where)


@pytest.mark.parametrize("dt", GR.DTYPES)
@pytest.mark.parametrize("n", GR.NONFINITE_NS)
def test_nonfinite_center_row(cuda, dt, n):
    """NaN and +inf in the centre row count as 0 in the centring: every other row stays exact."""
    D = GR.nonfinite_d(dt, n)
    X = GR.int_case(dt, n, D, True)
    cols = GR.nonfinite_cols(dt, n)
    for c in (0, n // 2, n - 1):
        for a, b in (("main", "last"), ("tail", "main")):
            Xb = X.clone()
            Xb[c, cols[a]], Xb[c, cols[b]] = math.nan, math.inf
            keep = torch.ones(n, dtype=torch.bool)
            keep[c] = False
            G = _windowed(cuda, Xb, c)
            assert torch.equal(G[keep][:, keep], GR.centered_oracle(Xb, c)[keep][:, keep]), (c, a, b)
            assert not math.isfinite(float(G[c, c])), (c, a, b)


# ----------------------------------------------------------------------------- h. float data
@pytest.mark.parametrize("kind", ["scaled", "cluster"])
@pytest.mark.parametrize("dt", GR.DTYPES)
@pytest.mark.parametrize("n", GR.FLOAT_NS)
def test_float_data_within_the_bound(cuda, dt, n, kind):
    """|G - G64| <= chain_len 2^-23 sum_k |y_ik y_jk| elementwise, y the rows the kernel
    multiplies (centred: x_i - x_c rounded once to the input dtype)."""
    D = GR.float_d(dt, n)
    nblk = GR.blocks(dt, n, D)
    X, c = GR.float_rows(kind, n, D, dt)
    for cc in (None, c):
        G64, bnd = GR.bound(X, dt, n, D, nblk, cc)
        G = _windowed(cuda, X, cc)
        err = (G - G64).abs()
        ratio = float((err / bnd.clamp_min(1e-300)).max())
        print(f"gram float {dt} n={n} {kind} center={cc}: max err / bound = {ratio:.4f} "
              f"(chain {GR.chain_len(dt, n, D, nblk)})")
        assert bool(torch.isfinite(G).all()) and bool((err <= bnd).all()), ratio


# ----------------------------------------------------------------------------- i. reduce and sum
@pytest.mark.parametrize("nb", GR.MULTI_BUCKETS)
@pytest.mark.parametrize("dt", GR.DTYPES)
@pytest.mark.parametrize("n", GR.MULTI_NS)
def test_partial_reduce_multi(cuda, dt, n, nb):
    Ds = GR.multi_ds(dt, n, nb)
    cen = nb == 1
    Xs = [GR.int_case(dt, n, D, cen, seed=20 + b) for b, D in enumerate(Ds)]
    c = n - 1 if cen else None
    G, nblks = _partials(cuda, Xs, n, c)
    assert nblks == [GR.blocks(dt, n, D) for D in Ds]
    assert nb != 2 or nblks[0] > GR.RED_BLOCK
    assert torch.equal(G, sum(GR.exact_gram(X, c) for X in Xs))


@pytest.mark.parametrize("nb", GR.SUM_NB)
def test_gram_sum(cuda, nb):
    gen = torch.Generator().manual_seed(nb)
    Gb = torch.randn(nb, GR.SUM_R, GR.SUM_R, generator=gen, dtype=torch.float64)
    out = torch.full((GR.SUM_R, GR.SUM_R), math.nan, dtype=torch.float64, device=cuda)
    want = Gb[0].clone()
    for b in range(1, nb):
        want = want + Gb[b]
    assert K.gram_sum(Gb.to(cuda), out) is out
    assert torch.equal(out.cpu(), want)


# ----------------------------------------------------------------------------- j. centre
@pytest.mark.parametrize("n", GR.CENTER_NS)
def test_gram_center(cuda, n):
    GR.check_center(K, cuda, n)


# ----------------------------------------------------------------------------- k. wrapper
def test_accumulate_needs_out(cuda):
    X = torch.ones(3, 16, device=cuda)
    with pytest.raises(ValueError, match="accumulate needs out"):
        K.gram(X, accumulate=True)
