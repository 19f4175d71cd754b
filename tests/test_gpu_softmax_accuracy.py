"""Every softmax of the library, per entry, over the whole exponent range of its exponentials.

The other GPU tests compare with the float64 oracle through whole-array measures (max|a - b| / max|b|): absolute in effect, so a
responsibility of 1e-40 or a component whose n_k is 1e-100 may be wrong by 100 % unseen.  Here every table entry, every normaliser
and every entry of n_k, sx_k, sxx_k is held RELATIVELY against a longdouble reference of the ladder problem (tests/softmax_ladder.py:
exact dyadic logits, component k in the band [-a_k - 3, -a_k], a_k up to 640 / 700), under bounds that come from the exponentials'
contract in mimo_device.h (relative error ~ 2^-53 |x|) and the float64 format, not from any kernel's output.  Every test prints its worst
device / bound ratio per output before it asserts.

Measured on an MI355X, against the longdouble reference (worst device / bound ratio over the family's shapes and both tops;
"before": the library with the reduction constant ln2/2048 of the 2048-entry exponentials off by 1.41e-14 relative — 38 of the
82 cases failed, exactly those on the 2048-entry table —, "after": the nearest double, all pass):

    test                       family / route                  before                            after
    tables        table, lse   small; narrow Dz=16 K=8 (*)     62.4,  0.00                       0.149, 0.00
                               fused Dz >= 14 (E2K)            60.0,  0.17                       0.145, 0.17
                               narrow, mid, rowwave-vi, fused  0.149, 0.21                       unchanged
                               (Dz < 14), two-stage (*)
    statistics    n, sx, sxx,  small                           52.5,  51.7,  51.7,  0.00         0.126, 0.122, 0.123, 0.00
                  sc0          narrow                          52.2,  51.4,  51.5,  0.03         0.123, 0.122, 0.123, 0.03
                               rowwave-vi                      50.8,  49.9,  50.0,  0.10         0.121, 0.119, 0.119, 0.10
                               mid                             0.127, 0.123, 0.125, 0.09         unchanged (64-entry table)
                               fused (Dz < 14)                 0.106, 0.104, 0.105, 0.03         unchanged
                               two-stage                       0.121, 0.119, 0.120, 0.06         unchanged
    fused Dz >= 14             dense (resp_skip_log2 = 0)      44.3,  43.1,  43.1,  0.13         0.105, 0.103, 0.103, 0.13
                               skip 60, a_k <= 30              4.45,  4.18,  4.22,  0.13         0.011, 0.011, 0.012, 0.13
                               skip 60, a_k > 30 (**)          0.000                             0.000
    clamp         statistics   small, narrow, rowwave-vi       48.2,  43.0,  43.0                0.115, 0.103, 0.102
                               mid, fused, two-stage           0.127, 0.103, 0.096               unchanged
                  tables       small / the others              61.7 / 0.147                      0.148 / 0.147
    batched       n, sx, sxx,  Dz, K = (2, 8), (8, 40),        0.146, 0.146, 0.146, 0.09         unchanged (64-entry table)
                  sc0          (16, 64)
    predict       weights      dx = 2, K = 8, dy = 8           62.3                              0.149

(*) a request for the per-datum tables runs on the small-shape kernel in its range (Dz <= 4 here) and on the tile kernels (fused /
two-stage; 64-entry table below Dz = 14, the 2048-entry one at Dz = 14 .. 16, K <= 64: the narrow shape Dz = 16, K = 8) everywhere
else, whatever family serves the plain pass: the tables of the narrow, mid and row-owner shapes are the tile kernels'.  Every route
returned the logits bit for bit.
(**) by construction of the rule: 2^-60 sum_n |phi_nf| exceeds statb(k) S_ref by orders of magnitude on every rung above 30, so this
half only says that nothing larger than the skipped weights is lost; the exponentials of those rungs are held by the dense run.
The lse and sc0 ratios are float64's own rounding of max + log(sum) and of the row sum (NumPy float64 gives the same figures).
"""
import numpy as np
import pytest

import softmax_ladder as SL

pytestmark = pytest.mark.gpu

E2K_MIN_D = 14                    # the fused kernel's 2048-entry exponential and its skipped statistics start at Dz = 14
SKIP_DENSE_A = 30.0               # rungs a_k <= 30: every weight is above 2^-60 (e^-33 = 2^-47.6), the skip leaves them alone
IDS = [f"{fam}-d{D}-k{K}-n{N}" for fam, D, K, N in SL.SHAPES]
PLAIN = [(s, i) for s, i in zip(SL.SHAPES, IDS) if not (s[0] == "fused" and s[1] >= E2K_MIN_D)]
SKIPPED = [(s, i) for s, i in zip(SL.SHAPES, IDS) if s[0] == "fused" and s[1] >= E2K_MIN_D]


def report(tag, ratios):
    print(f"\n[softmax-ladder] {tag}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()), flush=True)
    return ratios


def bind(engine, fam, Z, K):
    engine.upload(Z)
    assert engine.plan(K)["kind"] == fam, (fam, engine.plan(K))


def stat_ratios(ref, S, sc, top, comps=None, floors=(None, None, None)):
    """n (and, at top 640 and below, where every product r z z is a normal number, sx and sxx) per entry against statb; sc[0]."""
    out = {"n": ref.stat_ratio(S.n, ref.n, comps, floors[0])}
    if top <= 640:
        out["sx"] = ref.stat_ratio(S.sx, ref.sx, comps, floors[1])
        out["sxx"] = ref.stat_ratio(S.sxx, ref.sxx, comps, floors[2])
    out["sc0"] = ref.sc0_ratio(sc[0])
    return out


def table_ratios(engine, ref, K, L, comps=None):
    """The resident tables of a keep_* pass: logits bit for bit (the bounds' premise), then r_kn and lse_n per entry."""
    Lg = engine.get_logp(K)
    assert np.array_equal(Lg, L), f"the route rounds the logits: max |dL| = {np.abs(Lg - L).max():.3e}"
    return {"table": ref.table_ratio(engine.get_resp(K), comps), "lse": ref.lse_ratio(engine.get_lse())}


@pytest.mark.parametrize("top", SL.TOPS)
@pytest.mark.parametrize("fam,D,K,N", SL.SHAPES, ids=IDS)
def test_tables(engine, fam, D, K, N, top):
    """3a: r_kn against relb(k, n), lse_n against its bound, every entry; the logits first, bit for bit."""
    Z, c, b, W, L, ref = SL.case(D, K, N, top)
    bind(engine, fam, Z, K)
    engine.estep(c, b, W, keep_resp=True, keep_logp=True, keep_lse=True)
    r = report(f"tables {fam} Dz={D} K={K} N={N} top={top}", table_ratios(engine, ref, K, L))
    assert max(r.values()) < 1.0, r


@pytest.mark.parametrize("top", SL.TOPS)
@pytest.mark.parametrize("fam,D,K,N", [s for s, _ in PLAIN], ids=[i for _, i in PLAIN])
def test_statistics(engine, fam, D, K, N, top):
    """3b: the plain pass of the family's own kernel: n_k (top 640: also sx_k, sxx_k) per entry against statb(k), sc[0]."""
    Z, c, b, W, L, ref = SL.case(D, K, N, top)
    bind(engine, fam, Z, K)
    S, sc = engine.estep(c, b, W)
    r = report(f"statistics {fam} Dz={D} K={K} N={N} top={top}", stat_ratios(ref, S, sc, top))
    assert max(r.values()) < 1.0, r


@pytest.mark.parametrize("top", SL.TOPS)
@pytest.mark.parametrize("fam,D,K,N", [s for s, _ in SKIPPED], ids=[i for _, i in SKIPPED])
def test_statistics_fused_skip(engine, fam, D, K, N, top):
    """3c: the fused kernel at Dz >= 14 leaves weights below 2^-resp_skip_log2 out of its statistics.  Dense (0): the plain bounds.
    Default (60): rungs a_k <= 30 keep the plain bounds; the rest may miss, per entry, at most 2^-60 sum_n |phi_nf| of skipped
    weights:  |S - S_ref| <= 2^-60 sum_n |phi_nf| + statb(k) S_ref."""
    Z, c, b, W, L, ref = SL.case(D, K, N, top)
    bind(engine, fam, Z, K)
    try:
        engine.tune("resp_skip_log2", 0)
        S, sc = engine.estep(c, b, W)
    finally:
        engine.tune("resp_skip_log2", 60)
    dense = report(f"statistics {fam} Dz={D} K={K} N={N} top={top} dense", stat_ratios(ref, S, sc, top))
    S, sc = engine.estep(c, b, W)
    a, _ = SL.ladder(K, top)
    near, far = np.flatnonzero(a <= SKIP_DENSE_A), np.flatnonzero(a > SKIP_DENSE_A)
    assert near.size and far.size
    f1, fz, fzz = ref.abs_feature_sums()
    tau = 2.0 ** -60
    floors = (np.full(K, tau * f1), np.broadcast_to(tau * fz, (K, D)), np.broadcast_to(tau * fzz, (K, D, D)))
    r_near = report(f"statistics {fam} Dz={D} K={K} N={N} top={top} skip 60, a_k <= 30", stat_ratios(ref, S, sc, top, near))
    r_far = report(f"statistics {fam} Dz={D} K={K} N={N} top={top} skip 60, a_k > 30", stat_ratios(ref, S, sc, top, far, floors))
    assert max(dense.values()) < 1.0, dense
    assert max(r_near.values()) < 1.0 and max(r_far.values()) < 1.0, (r_near, r_far)


@pytest.mark.parametrize("D,K,N", SL.CLAMP_SHAPES, ids=[f"d{D}-k{K}-n{N}" for D, K, N in SL.CLAMP_SHAPES])
def test_clamp(engine, D, K, N):
    """3d: two rungs below the argument clamp at -707 (a = 720, 800): their entries come out as exp(-707) / sum <= 2e-307, their
    n_k <= N 2e-307, everything is finite, and every other component meets the plain bounds (against the true reference: what the
    clamp adds to a row's sum is below 2e-307 of it)."""
    fam = next(f for f, d, k, _ in SL.SHAPES if (d, k) == (D, K))
    Z, c, b, W, L, ref = SL.case(D, K, N, 640, 0, SL.CLAMP_TAIL)
    rest = slice(0, K - 2)
    bind(engine, fam, Z, K)
    S, sc = engine.estep(c, b, W)
    rs = report(f"clamp statistics {fam} Dz={D} K={K} N={N}", stat_ratios(ref, S, sc, 640, rest))
    assert all(np.all(np.isfinite(v)) for v in (S.n, S.sx, S.sxx, sc[:1]))
    assert np.all(S.n[K - 2:] >= 0.0) and np.all(S.n[K - 2:] <= N * 2e-307)
    engine.estep(c, b, W, keep_resp=True, keep_logp=True, keep_lse=True)
    rt = report(f"clamp tables {fam} Dz={D} K={K} N={N}", table_ratios(engine, ref, K, L, rest))
    R, lse = engine.get_resp(K), engine.get_lse()
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(lse))
    assert np.all(R[K - 2:] >= 0.0) and np.all(R[K - 2:] <= 2e-307)
    assert max(rs.values()) < 1.0 and max(rt.values()) < 1.0, (rs, rt)


@pytest.fixture(scope="module")
def batched_engine():
    from mimo_amd.batched import BatchedHipEngine
    eng = BatchedHipEngine(0)
    yield eng
    eng.close()


@pytest.mark.parametrize("D,K", SL.BATCHED_SHAPES, ids=[f"d{D}-k{K}" for D, K in SL.BATCHED_SHAPES])
def test_batched(batched_engine, D, K):
    """3e: three problems (257, 3 and 515 rows; tops 640, 640, 320) in one launch: each problem's statistics and sc[:, 0] under
    the bounds of its own reference.  (The batched kernel has no skipped statistics: plain bounds at Dz = 16 too.)"""
    cases = [SL.case(D, K, N, top) for N, top in zip(SL.BATCHED_ROWS, SL.BATCHED_TOPS)]
    batched_engine.upload([cs[0] for cs in cases])
    S, sc = batched_engine.estep(np.stack([cs[1] for cs in cases]), np.stack([cs[2] for cs in cases]), np.stack([cs[3] for cs in cases]))
    worst = {}
    for i, cs in enumerate(cases):
        r = report(f"batched Dz={D} K={K} problem {i} N={SL.BATCHED_ROWS[i]} top={SL.BATCHED_TOPS[i]}",
                   stat_ratios(cs[5], S[i], sc[i], SL.BATCHED_TOPS[i]))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    assert max(worst.values()) < 1.0, worst


def test_predict_gating_weights(engine):
    """3f: posterior prediction with dx = 2, K = 8, dy = 8, affine: expert k maps every input to the k-th unit vector (M_k zero but
    for a 1 in row k of the offset column, Q = 0, Cc = I), so the predicted mean IS the gating weight vector: every entry against
    relb (top 640, N = 257).  The kernel's 1 / sum and product in place of a division is one rounding more: inside relb's u (K + 4)."""
    D, K, N, top = 2, 8, 257, 640
    Z, c, b, W, L, ref = SL.case(D, K, N, top)
    M = np.zeros((K, K, D + 1))
    M[np.arange(K), np.arange(K), D] = 1.0
    engine.upload(Z)
    mu, _, _ = engine.predict(c, b, W, M, np.zeros((K, D + 1, D + 1)), np.broadcast_to(np.eye(K), (K, K, K)).copy(),
                              affine=True, mode='average')
    r = report(f"predict gating weights dx={D} K={K} N={N} top={top}", {"weights": ref.table_ratio(np.ascontiguousarray(mu.T))})
    assert np.all(np.isfinite(mu)) and max(r.values()) < 1.0, r
