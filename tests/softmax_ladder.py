"""The ladder problem: a softmax whose logits are exact in float64 and whose terms cover the whole exponent range of the device
exponentials (mimo_device.h: exp_nonpos, exp_nonpos_t2048, exp_nonpos_t2048c, exp_c_issue / exp_c_finish), with a longdouble
reference and PER-ENTRY error bounds.  Imported by tests/test_softmax_ladder_cpu.py (no GPU) and tests/test_gpu_softmax_accuracy.py.

problem(D, K, N, top, seed) -> (Z, c, b, W):
    Z[n, 0]   = ((37 n) mod 1024) / 1024              Z[n, d > 0] = integers(0, 9) / 4         (all >= 0)
    a_k       = round(16 k top / (K - 1)) / 16        s_k = k mod 4  (s_0 = 0)
    c = -a,   b[:, 0] = -s, the rest of b zero,       W_k = I
Every input is dyadic, so  L = c + b'z - z'Wz / 2  is exact in float64 under any summation or FMA order (at most 31 significant
bits between 2^9 and 2^-21).  Component 0 is each row's maximum, so x_kn = L_kn - max = -a_k - s_k Z[n, 0] exactly: component k
lives in the band [-a_k - 3, -a_k], and its n_k, sx_k, sxx_k carry the exponential's error at |x| ~ a_k.  All features are
nonnegative: every statistic is a sum of positive terms and a relative bound means something.

Bounds (u = 2^-53; r the exact responsibilities):
    term(k, n)  = u (2 |x_kn| + 8)                                  one exponential: the documented reduction error u |x|, doubled,
                                                                     plus polynomial (< 0.3 u), table entry, FMA chain and final
                                                                     product (~3 u), doubled
    relb(k, n)  = term(k, n) + sum_j r_jn term(j, n) + u (K + 4)    a table entry r_kn, relatively (the sum's error is the
                                                                     r-weighted mean of its terms' errors, plus a K-term chain)
    statb(k)    = max_n relb(k, n) + u (N + 8)                      every entry of n_k, sx_k, sxx_k, relatively (u N: the worst
                                                                     case of a length-N chain)
    lse_n       : u (|lse_n| + 2) + sum_j r_jn term(j, n) + u (K + 4),   absolutely
    sc[0]       : the sum over the rows of the lse_n bounds + u N max|lse|,  absolutely
They come from the contract and the number format, never from a kernel's output."""
import functools

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
NS = (257, 515, 1029)            # ragged, a few tiles

# (family, Dz, K, N): the shapes of the GPU tests; the families are those engine.plan(K) reports AT THESE N for a plain pass
SHAPES = [
    ("small", 2, 8, 257), ("small", 4, 8, 515),
    ("narrow", 2, 64, 1029), ("narrow", 3, 32, 515), ("narrow", 5, 16, 257), ("narrow", 8, 16, 1029), ("narrow", 16, 8, 515),
    ("mid", 12, 16, 257), ("mid", 16, 80, 1029),
    ("rowwave-vi", 8, 32, 515), ("rowwave-vi", 8, 64, 257), ("rowwave-vi", 9, 20, 1029),
    ("fused", 8, 40, 515), ("fused", 3, 256, 1029), ("fused", 16, 64, 1029), ("fused", 14, 64, 515),
    ("two-stage", 12, 200, 515), ("two-stage", 32, 64, 257),
]
TOPS = (640, 700)
CLAMP_TAIL = (720.0, 800.0)      # a_{K-2}, a_{K-1} of the clamp problem: both below the exponentials' argument clamp at -707
CLAMP_SHAPES = [(2, 8, 257), (3, 32, 515), (12, 16, 257), (8, 32, 515), (8, 40, 515), (12, 200, 515)]      # one per family
BATCHED_SHAPES = [(2, 8), (8, 40), (16, 64)]
BATCHED_ROWS, BATCHED_TOPS = (257, 3, 515), (640, 640, 320)


def ladder(K, top, tail=None):
    """-> (a (K,), s (K,)); tail = (a_{K-2}, a_{K-1}) replaces the last two rungs."""
    k = np.arange(K)
    a = np.round(16.0 * k * top / (K - 1)) / 16.0
    if tail is not None:
        a[K - 2], a[K - 1] = tail
    return a, (k % 4).astype(np.float64)


def problem(D, K, N, top, seed, tail=None):
    rng = np.random.default_rng(seed)
    Z = np.empty((N, D))
    Z[:, 0] = ((37 * np.arange(N)) % 1024) / 1024.0
    Z[:, 1:] = rng.integers(0, 9, size=(N, D - 1)) / 4.0
    a, s = ladder(K, top, tail)
    b = np.zeros((K, D))
    b[:, 0] = -s
    return Z, -a, b, np.broadcast_to(np.eye(D), (K, D, D)).copy()


def logits(Z, c, b, W):
    """L (K, N) in float64: exact for a ladder problem, whatever the order of the operations."""
    return c[:, None] + b @ Z.T - 0.5 * np.einsum('na,kab,nb->kn', Z, W, Z)


class Reference:
    """longdouble softmax and statistics of exact logits L over the rows Z, and the bounds of the module docstring."""

    def __init__(self, Z, L):
        self.Z, self.L = Z, L
        K, N = L.shape
        Ll = L.astype(LD)
        self.max = L.max(axis=0)
        self.x = Ll - self.max.astype(LD)                      # exact
        e = np.exp(self.x)
        tot = e.sum(axis=0)
        self.R = e / tot
        self.lse = self.max.astype(LD) + np.log(tot)
        self.n = self.R.sum(axis=1)
        # bounds
        self.term = U * (2.0 * np.abs(self.x).astype(np.float64) + 8.0)
        mean_term = (self.R.astype(np.float64) * self.term).sum(axis=0)
        self.relb = self.term + mean_term + U * (K + 4)
        self.statb = self.relb.max(axis=1) + U * (N + 8)
        self.lse_b = U * (np.abs(self.lse).astype(np.float64) + 2.0) + mean_term + U * (K + 4)
        self.sc0 = self.lse.sum()
        self.sc0_b = float(self.lse_b.sum() + U * N * np.abs(self.lse).max())

    @functools.cached_property
    def sx(self):
        Zt = np.ascontiguousarray(self.Z.T).astype(LD)                                     # (D, N)
        return (self.R[:, None, :] * Zt[None, :, :]).sum(axis=2)                         # pairwise sums along the rows

    @functools.cached_property
    def phi2(self):
        """z z' per row as (D D, N), float64 (exact: dyadic features)."""
        N, D = self.Z.shape
        return np.ascontiguousarray((self.Z[:, :, None] * self.Z[:, None, :]).reshape(N, D * D).T)

    @functools.cached_property
    def sxx(self):
        K, (N, D) = self.L.shape[0], self.Z.shape
        P = self.phi2.astype(LD)
        out = np.empty((K, D * D), dtype=LD)
        for k in range(K):
            out[k] = (P * self.R[k][None, :]).sum(axis=1)
        return out.reshape(K, D, D)

    # -- ratios: |got - ref| / bound, per entry ------------------------------------------------------------
    def table_ratio(self, Rg, comps=None):
        """worst |r - r_ref| / (relb r_ref) over the table (over the components `comps`)."""
        k = slice(None) if comps is None else comps
        return float((np.abs(Rg.astype(LD)[k] - self.R[k]) / (self.relb[k] * self.R[k])).max())

    def lse_ratio(self, lse):
        return float((np.abs(lse.astype(LD) - self.lse) / self.lse_b).max())

    def sc0_ratio(self, sc0):
        return float(abs(LD(sc0) - self.sc0) / self.sc0_b)

    def stat_ratio(self, got, ref, comps=None, floor=None):
        """worst |S - S_ref| / (statb(k) S_ref [+ floor]) over the entries of one statistic (leading axis: the component).
        An entry whose reference is exactly 0 must be 0."""
        K = ref.shape[0]
        sb = self.statb.reshape((K,) + (1,) * (ref.ndim - 1))
        den = sb * ref + (0 if floor is None else floor)
        err = np.abs(np.asarray(got).astype(LD) - ref)
        ratio = np.where(den > 0, err / np.where(den > 0, den, 1), np.where(err > 0, np.inf, 0.0))
        k = slice(None) if comps is None else comps
        return float(ratio[k].max())

    def abs_feature_sums(self):
        """sum_n |phi_nf| for f = 1, z_d, z_d z_e: (), (D,), (D, D) — the scale of the skipped weights' share (rule c)."""
        N, D = self.Z.shape
        return float(N), self.Z.sum(axis=0), self.phi2.sum(axis=1).reshape(D, D)


@functools.lru_cache(maxsize=None)
def case(D, K, N, top, seed=0, tail=None):
    """-> (Z, c, b, W, L, Reference), computed once per session and shared; treat every array as read-only."""
    Z, c, b, W = problem(D, K, N, top, seed, tail)
    L = logits(Z, c, b, W)
    for arr in (Z, c, b, W, L):
        arr.setflags(write=False)
    return Z, c, b, W, L, Reference(Z, L)


def float64_softmax_stats(Z, L):
    """Plain NumPy float64 arithmetic of the same operation (the honest-arithmetic yardstick of the CPU tests)."""
    m = L.max(axis=0)
    e = np.exp(L - m)
    tot = e.sum(axis=0)
    R = e / tot
    lse = m + np.log(tot)
    return R, lse, R.sum(axis=1), R @ Z, np.einsum('kn,na,nb->kab', R, Z, Z)
