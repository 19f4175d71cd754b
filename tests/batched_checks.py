"""Shared by the batched GPU modules (test_gpu_batched*.py) and tests/test_batched_cells_cpu.py: the random batch, the
naive per-problem oracle, the per-component error measure — and a plain Python restatement of the rules of
mimo_batched.hip that decide which kernel instantiation and which tile split a problem gets (batched_covers,
batched_tiles_per_wg, the (NCB, RBW) choice).  No GPU and no library are needed to import this module."""
import numpy as np

from oracle import mimo_oracle as O

TOL = 1e-11

# ---- the kernel's rules, restated (test_batched_cells_cpu.py checks the constants against the headers) -----------------
TILE = 32            # kTile: rows per tile
MAX_D = 16           # kBatchedMaxD
MAX_K = 128          # kBatchedMaxK
MAX_PAIRS = 40       # kBatchedMaxPairs: K16 * NCB statistics blocks of one workgroup
MAX_WG = 128         # workgroups per problem at most (batched_tiles_per_wg)
MIN_TPW = 4          # tiles per workgroup at least
PHILOX_BATCH = 8     # tiles one PhiloxBatch covers


def feat_count(D):
    return (D + 1) * (D + 2) // 2


def ncb_of(D):
    """16-wide feature column blocks."""
    return -(-feat_count(D) // 16)


def covers(K, D):
    if D < 1 or D > MAX_D or K < 1 or K > MAX_K:
        return False
    return -(-K // 16) * ncb_of(D) <= MAX_PAIRS


def kmax(D):
    """The largest K the batched pass takes at Dz = D."""
    return max(K for K in range(1, MAX_K + 1) if covers(K, D))


def pair_of(D, K):
    """(NCB, RBW) of the kernel instantiation that serves (Dz, K)."""
    assert covers(K, D)
    return ncb_of(D), 1 if -(-K // 16) <= 4 else 2


def pair_kmax(ncb, rbw):
    """The largest K of an (NCB, RBW) pair, or 0 when the pair is unreachable."""
    k16 = min(4 * rbw, MAX_PAIRS // ncb)
    return 16 * k16 if k16 > 4 * (rbw - 1) else 0


def tiles_per_wg(nrows):
    tiles = -(-nrows // TILE)
    return max(-(-tiles // MAX_WG), MIN_TPW)


def split(nrows):
    """The (tile0, ntiles) runs of a problem's workgroups."""
    tiles, tpw = -(-nrows // TILE), tiles_per_wg(nrows)
    return [(t, min(tpw, tiles - t)) for t in range(0, tiles, tpw)]


# ---- random batches and the oracle --------------------------------------------------------------------------------------
def problems(rng, rows, D, K, off=0):
    """Data and (c, b, W) of len(rows) problems; component `off` of every problem switched off (c = -inf) when K has more
    than off + 1 components (off=None: none)."""
    B = len(rows)
    Zs = [rng.standard_normal((n, D)) * 1.5 + rng.standard_normal(D) for n in rows]
    A = rng.standard_normal((B, K, D, D))
    W = A @ A.transpose(0, 1, 3, 2) / D + 0.3 * np.eye(D)
    b = rng.standard_normal((B, K, D))
    c = rng.standard_normal((B, K))
    if off is not None and K > off + 1:
        c[:, off] = -np.inf
    return Zs, c, b, W


def oracle(Z, c, b, W, chunk=8192):
    """(n, sx, sxx, scalars[3], lse) of one problem, naively (long problems in row chunks, to bound the memory of the
    (K, N, Dz) intermediates)."""
    K, D = b.shape
    n, sx, sxx, srl, lse = np.zeros(K), np.zeros((K, D)), np.zeros((K, D, D)), 0.0, []
    for i in range(0, len(Z), chunk):
        Zc = Z[i:i + chunk]
        L = O.canonical_eval(Zc, c, b, W)
        l = O.logsumexp(L, axis=0)
        r = np.exp(L - l)
        dn, dsx, dsxx = O.packed_stats(Zc, r)
        n += dn; sx += dsx; sxx += dsxx
        srl += np.sum(np.where(r > 0, r * np.where(np.isfinite(L), L, 0.), 0.))
        lse.append(l)
    lse = np.concatenate(lse) if lse else np.zeros(0)
    return n, sx, sxx, np.array([lse.sum(), srl, lse.sum() - srl]), lse


def oracle_labels(Z, c, b, W, u, chunk=8192):
    """The inverse-CDF labels of one problem's rows for the uniforms u (N,)."""
    out = [O.sample_discrete_from_log(O.canonical_eval(Z[i:i + chunk], c, b, W), u[i:i + chunk])
           for i in range(0, len(Z), chunk)]
    return np.concatenate(out) if out else np.zeros(0, np.int32)


def label_oracle(Z, labels, K, chunk=8192):
    """(n, sx, sxx) of hard labels, naively."""
    D = Z.shape[1]
    labels = np.asarray(labels, dtype=np.int64)
    n, sx, sxx = np.zeros(K), np.zeros((K, D)), np.zeros((K, D, D))
    for i in range(0, len(Z), chunk):
        dn, dsx, dsxx = O.packed_stats(Z[i:i + chunk], O.one_hot(labels[i:i + chunk], K))
        n += dn; sx += dsx; sxx += dsxx
    return n, sx, sxx


def qerr(a, ref, floor=1.0):
    """Relative error of one quantity at its own scale (per component for the statistics), with an absolute floor."""
    a, ref = np.asarray(a, dtype=float), np.asarray(ref, dtype=float)
    if ref.size == 0:
        return 0.0
    if ref.ndim >= 2:          # per component k
        ax = tuple(range(1, ref.ndim))
        scale = np.maximum(np.abs(ref).max(axis=ax), floor)
        return float((np.abs(a - ref).max(axis=ax) / scale).max())
    return float((np.abs(a - ref) / np.maximum(np.abs(ref), floor)).max())


def check_against(S, sc, lse, ref):
    """Statistics, scalars and lse rows of a softmax pass against (n, sx, sxx, scalars, lse)."""
    n, sx, sxx, scal, l = ref
    errs = {"n": qerr(S.n[:, None], n[:, None]), "sx": qerr(S.sx, sx), "sxx": qerr(S.sxx, sxx),
            "scalars": qerr(sc, scal), "lse": qerr(lse, l)}
    assert max(errs.values()) <= TOL, errs


def check_stats(S, Z, labels, K):
    """Statistics of hard labels: exact integer counts, sums within TOL."""
    labels = np.asarray(labels, dtype=np.int64)
    n, sx, sxx = label_oracle(Z, labels, K)
    assert np.array_equal(S.n, np.bincount(labels, minlength=K).astype(float))
    assert np.array_equal(S.n, n)
    errs = {"sx": qerr(S.sx, sx), "sxx": qerr(S.sxx, sxx)}
    assert max(errs.values()) <= TOL, errs
