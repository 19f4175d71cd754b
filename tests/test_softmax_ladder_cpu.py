"""The ladder problem of the GPU softmax accuracy tests (tests/softmax_ladder.py), checked without a GPU: its logits are exact,
its longdouble reference agrees with 50-digit values (tests/golden/softmax_ladder_hp.npz, make_softmax_ladder_golden.py), and its
bounds leave plain float64 arithmetic a factor of four of room."""
from fractions import Fraction

import numpy as np
import pytest

from conftest import load_golden
import softmax_ladder as SL

LD = np.longdouble
# every problem a GPU test builds: the family shapes at both tops, the clamp problem, the batched problems' tops and row counts
PROBLEMS = ([(D, K, N, top, None) for _, D, K, N in SL.SHAPES for top in SL.TOPS]
            + [(D, K, N, 640, SL.CLAMP_TAIL) for D, K, N in SL.CLAMP_SHAPES]
            + [(D, K, N, top, None) for D, K in SL.BATCHED_SHAPES for N, top in zip(SL.BATCHED_ROWS, SL.BATCHED_TOPS)])


def test_longdouble_is_extended_precision():
    """The reference is only a reference if longdouble carries at least 64 significant bits (x87 extended or wider)."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_shapes_cover_every_family_at_ragged_row_counts():
    assert {f for f, _, _, _ in SL.SHAPES} == {"small", "narrow", "mid", "rowwave-vi", "fused", "two-stage"}
    assert all(N in SL.NS and N % 32 for _, _, _, N in SL.SHAPES) and {N for _, _, _, N in SL.SHAPES} == set(SL.NS)
    assert all(any((d, k, n) == (D, K, N) for _, d, k, n in SL.SHAPES) for D, K, N in SL.CLAMP_SHAPES)


@pytest.mark.parametrize("D,K,N,top,tail", PROBLEMS)
def test_logits_are_exact(D, K, N, top, tail):
    """L from float64 NumPy equals rational arithmetic on a sample of entries (every component at 9 rows, first and last among
    them), component 0 is every row's maximum and x_kn = -a_k - s_k Z[n, 0]."""
    Z, c, b, W, L, ref = SL.case(D, K, N, top, 0, tail)
    a, s = SL.ladder(K, top, tail)
    rows = sorted(set(np.linspace(0, N - 1, 9).astype(int).tolist()))
    for n in rows:
        z = [Fraction(float(v)) for v in Z[n]]
        quad = sum(z[d] * Fraction(float(W[0, d, e])) * z[e] for d in range(D) for e in range(D)) / 2       # W_k = I for every k
        for k in range(K):
            exact = Fraction(float(c[k])) + sum(Fraction(float(b[k, d])) * z[d] for d in range(D)) - quad
            assert Fraction(float(L[k, n])) == exact, (k, n)
    assert np.array_equal(W, np.broadcast_to(np.eye(D), W.shape))
    assert np.array_equal(L.argmax(axis=0), np.zeros(N, dtype=int)) and np.array_equal(L.max(axis=0), L[0])
    assert np.array_equal(L - L[0], -a[:, None] - s[:, None] * Z[None, :, 0])
    assert np.array_equal(ref.x.astype(np.float64), L - L[0]) and Z.min() >= 0.0


@pytest.mark.parametrize("top", SL.TOPS)
def test_longdouble_reference_against_50_digits(top):
    """R, n, sx, sxx relatively to 2^-60; lse to 2^-60 (|lse| + 1): its bound is absolute, and a row at the origin has
    lse = log(1 + 1e-40...), which no max + log(sum) in any finite precision returns relatively."""
    g = load_golden("softmax_ladder_hp")
    D, K, N, seed = (int(v) for v in g["shape"])
    Z, c, b, W, L, ref = SL.case(D, K, N, top, seed)
    scale = LD(2.0) ** int(g["scale_log2"])
    hp = lambda name: g[f"t{top}_{name}_hi"].astype(LD) + g[f"t{top}_{name}_lo"].astype(LD)
    tol = LD(2.0) ** -60
    for name, got in (("R", ref.R), ("n", ref.n), ("sx", ref.sx), ("sxx", ref.sxx)):
        want = hp(name) / scale
        assert want.shape == got.shape and np.all(want > 0)
        worst = float((np.abs(got - want) / want).max())
        print(f"top {top} {name}: worst relative difference 2^{np.log2(max(worst, 1e-30)):.1f}")
        assert worst <= tol, name
    want = hp("lse")
    assert float((np.abs(ref.lse - want) / (np.abs(want) + 1)).max()) <= tol


@pytest.mark.parametrize("D,K,N,top,tail", PROBLEMS)
def test_float64_numpy_has_room_under_every_bound(D, K, N, top, tail):
    """Plain float64 NumPy (exp, divide, sums in NumPy's own order) stays under a quarter of every bound.  (The two rungs of the
    clamp problem lie below float64's normal range, exp(-720) = 2e-313: they are left out, as on the GPU.)"""
    Z, c, b, W, L, ref = SL.case(D, K, N, top, 0, tail)
    R, lse, n, sx, sxx = SL.float64_softmax_stats(Z, L)
    ks = slice(None) if tail is None else slice(0, K - 2)
    ratios = {"table": ref.table_ratio(R, ks), "lse": ref.lse_ratio(lse), "sc0": ref.sc0_ratio(lse.sum()),
              "n": ref.stat_ratio(n, ref.n, ks), "sx": ref.stat_ratio(sx, ref.sx, ks), "sxx": ref.stat_ratio(sxx, ref.sxx, ks)}
    print(D, K, N, top, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) < 0.25, ratios
