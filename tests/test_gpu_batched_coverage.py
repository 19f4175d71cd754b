"""GPU: every instantiation, tile split and batch layout of the batched passes (mimo_batched.hip through BatchedHipEngine).

The tables below are chosen from the kernel's own rules (tests/batched_checks.py restates batched_covers,
batched_tiles_per_wg and the (NCB, RBW) choice) and tests/test_batched_cells_cpu.py asserts, without a GPU, what they
cover: all 18 (NCB, RBW) pairs at their largest K and at a ragged K, every Dz, workgroups of 4, 5, 9 and 18 tiles, the
128-workgroup cap, one-row last tiles, reduce chains of 0 .. 8 partial blocks.  Reference throughout: the NumPy oracle on
each problem's rows alone, and a solo HipEngine pass over the same rows; TOL and qerr are the batched path's own
(batched_checks).  Labels equal the oracle's exactly and counts are exact integers; all inputs are seeded.

Switched-off components (c = -inf): the label modes never draw them and their statistics are exactly zero.  The softmax
carries them at exp(-707) (the clamp of the kernel's exponential, as in the solo kernels), so there their statistics are
below 1e-290 — the bound tests/test_gpu_parity.py::test_switched_off_component_and_far_clusters sets for the solo engine.
"""
import numpy as np
import pytest

from batched_checks import (TOL, check_against, check_stats, kmax, oracle, oracle_labels, problems, qerr)
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.engine import HipEngine
from oracle import mimo_oracle as O

pytestmark = pytest.mark.gpu

# (Dz, K): per (NCB, RBW) pair the largest K of the pair and one K whose last row block is padded
CELLS = [
    (3, 64), (2, 37), (4, 128), (1, 65),            # NCB 1
    (5, 64), (6, 23), (6, 128), (5, 81),            # NCB 2
    (7, 64), (8, 7), (8, 128), (7, 100),            # NCB 3
    (9, 64), (9, 33), (9, 128), (9, 70),            # NCB 4
    (10, 64), (11, 17), (10, 128), (11, 113),       # NCB 5
    (12, 64), (12, 5), (12, 96), (12, 81),          # NCB 6
    (13, 64), (13, 49), (13, 80), (13, 65),         # NCB 7
    (14, 64), (14, 20), (14, 80), (14, 70),         # NCB 8
    (15, 64), (15, 3),                              # NCB 9 (RBW 1 only)
    (16, 64), (16, 47),                             # NCB 10 (RBW 1 only)
]
CELL_ROWS = [33, 0, 2500, 1, 32, 31]

# rows per problem that leave the four-tiles-per-workgroup split (see test_batched_cells_cpu.py for what each one produces)
LARGE_ROWS = [16384, 16385, 20480, 20449, 32801, 70001]
SMALL_ROWS = [0, 1, 33, 0, 31]                      # interleaved with the large problems
SPLIT_SHAPES = [(2, 100), (8, 64)]                  # one RBW = 2 and one RBW = 1 shape (the Philox batch is RBW = 1's)

# 0 .. 8 workgroups per problem: the lengths of the reduce kernel's chains
CHAIN_ROWS = [0, 100, 200, 300, 400, 520, 650, 780, 900]
CHAIN_SHAPES = [(3, 17), (2, 100)]

SWEEP = 5


def split_rows():
    rows = []
    for i, n in enumerate(LARGE_ROWS):
        rows += [n] + SMALL_ROWS[i:i + 1]
    return rows


@pytest.fixture(scope="module")
def beng():
    return BatchedHipEngine(0)


@pytest.fixture(scope="module")
def solo():
    return HipEngine(0)


def off_components(c):
    return np.flatnonzero(np.isneginf(c))


def packed(S):
    return [s.packed() for s in S]


def same_bits(A, B):
    return len(A) == len(B) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(A, B))


def softmax_pass(beng, solo, Zs, c, b, W, witness=None):
    """The softmax pass with keep_lse + entropy_split against the oracle (and the solo engine for the problems in
    `witness`, all non-empty ones by default), without statistics, and plain.  Returns (packed statistics, scalars, lse)."""
    Sb, scb = beng.estep(c, b, W, keep_lse=True, entropy_split=True)
    lseb = beng.get_lse()
    for i, Z in enumerate(Zs):
        assert lseb[i].shape == (len(Z),)
        check_against(Sb[i], scb[i], lseb[i], oracle(Z, c[i], b[i], W[i]))
        off = off_components(c[i])
        assert np.all(Sb[i].n[off] < 1e-290) and np.all(np.abs(Sb[i].sxx[off]) < 1e-290)
        if len(Z) == 0 or (witness is not None and i not in witness):
            continue
        solo.upload(Z)
        S1, sc1 = solo.estep(c[i], b[i], W[i], keep_lse=True, entropy_split=True)
        check_against(Sb[i], scb[i], lseb[i], (S1.n, S1.sx, S1.sxx, sc1, solo.get_lse()))
    assert all(np.isfinite(p).all() for p in packed(Sb)) and np.isfinite(scb).all()
    S3, sc3 = beng.estep(c, b, W, stats=False, entropy_split=True)
    assert S3 is None and np.array_equal(sc3, scb)
    S2, sc2 = beng.estep(c, b, W)
    assert np.array_equal(sc2[:, 0], scb[:, 0]) and np.isnan(sc2[:, 1:]).all()
    assert same_bits(packed(S2), packed(Sb))
    return packed(Sb), scb, lseb


def draw_pass(beng, solo, Zs, c, b, W, seeds, u, witness=None):
    """The label draw with host uniforms and with Philox seeds: labels equal to the oracle's (and the solo engine's),
    exact counts, statistics, the resident labels.  Returns {mode: (labels, packed statistics)}."""
    K = c.shape[1]
    out = {}
    for mode in ("host", "philox"):
        labs, S = beng.gibbs_labels(c, b, W, seeds=seeds if mode == "philox" else None, sweep=SWEEP,
                                    u=u if mode == "host" else None)
        for i, Z in enumerate(Zs):
            n = len(Z)
            uu = u[i].reshape(-1) if mode == "host" else O.philox_uniforms(seeds[i], np.arange(n), SWEEP)
            ref = oracle_labels(Z, c[i], b[i], W[i], uu)
            assert labs[i].dtype == np.int32 and labs[i].shape == (n,)
            wrong = np.flatnonzero(labs[i] != ref)
            assert wrong.size == 0, (mode, i, n, f"{wrong.size} labels differ, first at local row {wrong[:1]} "
                                                 f"(tile {wrong[:1] // 32})")
            off = off_components(c[i])
            assert not np.isin(labs[i], off).any()                        # c = -inf: never drawn
            check_stats(S[i], Z, labs[i], K)
            assert not S[i].packed()[off].any()                           # ... and exactly zero statistics
            if n == 0 or (witness is not None and i not in witness):
                continue
            solo.upload(Z)
            sl, sS = solo.gibbs_labels(c[i], b[i], W[i], seed=seeds[i], sweep=SWEEP, u=u[i] if mode == "host" else None)
            assert np.array_equal(sl, labs[i]), (mode, i, n)
            assert np.array_equal(sS.n, S[i].n)
            assert qerr(S[i].sx, sS.sx) <= TOL and qerr(S[i].sxx, sS.sxx) <= TOL
        assert same_bits(beng.get_labels(), labs)
        assert same_bits(packed(beng.label_stats(None, K)), packed(S))
        out[mode] = (labs, packed(S))
    labs2, none = beng.gibbs_labels(c, b, W, seeds=seeds, sweep=SWEEP, stats=False)
    assert none is None and same_bits(labs2, out["philox"][0])
    return out


def given_pass(beng, solo, Zs, K, rng, witness=None):
    """Statistics of given labels: random ones, and every row on the last component (highest row block, highest lane).
    Returns the packed statistics of both."""
    rows = [len(Z) for Z in Zs]
    out = []
    for labels in ([rng.integers(0, K, size=n).astype(np.int32) for n in rows], [np.full(n, K - 1, dtype=np.int32) for n in rows]):
        S = beng.label_stats(labels, K)
        for i, Z in enumerate(Zs):
            check_stats(S[i], Z, labels[i], K)
            if len(Z) == 0 or (witness is not None and i not in witness):
                continue
            solo.upload(Z)
            sS = solo.label_stats(labels[i], K)
            assert np.array_equal(sS.n, S[i].n)
            assert qerr(S[i].sx, sS.sx) <= TOL and qerr(S[i].sxx, sS.sxx) <= TOL
        out.append(packed(S))
    return out


def draws_for(rng, rows):
    return [int(s) for s in rng.integers(0, 2**63, size=len(rows))], [rng.random(n) for n in rows]


# ---- a. every instantiation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", CELLS)
def test_every_instantiation(beng, solo, D, K):
    rng = np.random.default_rng(1000 * D + K)
    rows = [int(n) for n in rng.permutation(CELL_ROWS)]
    Zs, c, b, W = problems(rng, rows, D, K)
    seeds, u = draws_for(rng, rows)
    beng.upload(Zs)
    softmax_pass(beng, solo, Zs, c, b, W)
    draw_pass(beng, solo, Zs, c, b, W, seeds, u)
    given_pass(beng, solo, Zs, K, rng)


# ---- b. tile split --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", SPLIT_SHAPES)
def test_tile_split(beng, solo, D, K):
    """Workgroups of 4, 5, 9 and 18 tiles, ragged last workgroups, the 128-workgroup cap and the Philox batch's refills
    (RBW = 1), in one batch with tiny and empty problems; then each large problem alone: the same bits."""
    rng = np.random.default_rng(77 * D + K)
    rows = split_rows()
    Zs, c, b, W = problems(rng, rows, D, K)
    seeds, u = draws_for(rng, rows)
    beng.upload(Zs)
    Ssm, scal, lse = softmax_pass(beng, solo, Zs, c, b, W)
    draws = draw_pass(beng, solo, Zs, c, b, W, seeds, u)
    given = given_pass(beng, solo, Zs, K, np.random.default_rng(5))
    grng = np.random.default_rng(5)                         # the random labels given_pass drew first
    glabels = [grng.integers(0, K, size=n).astype(np.int32) for n in rows]
    for i, n in enumerate(rows):
        if n not in LARGE_ROWS:
            continue
        s = slice(i, i + 1)
        beng.upload([Zs[i]])
        S1, sc1 = beng.estep(c[s], b[s], W[s], keep_lse=True, entropy_split=True)
        assert np.array_equal(S1[0].packed(), Ssm[i]) and np.array_equal(sc1[0], scal[i]), n
        assert np.array_equal(beng.get_lse()[0], lse[i]), n
        L1, G1 = beng.gibbs_labels(c[s], b[s], W[s], seeds=[seeds[i]], sweep=SWEEP)
        assert np.array_equal(L1[0], draws["philox"][0][i]) and np.array_equal(G1[0].packed(), draws["philox"][1][i]), n
        L1, G1 = beng.gibbs_labels(c[s], b[s], W[s], u=[u[i]])
        assert np.array_equal(L1[0], draws["host"][0][i]) and np.array_equal(G1[0].packed(), draws["host"][1][i]), n
        assert np.array_equal(beng.label_stats([glabels[i]], K)[0].packed(), given[0][i]), n


# ---- c. reduce chains ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", CHAIN_SHAPES)
def test_reduce_chain_lengths(beng, D, K):
    """Problems of 0, 1, ..., 8 workgroups in one batch: the fixed-order sum of the reduce kernel (four interleaved
    chains and a remainder) at every length, per problem against the oracle."""
    rng = np.random.default_rng(31 * D + K)
    Zs, c, b, W = problems(rng, CHAIN_ROWS, D, K)
    beng.upload(Zs)
    S, sc = beng.estep(c, b, W, entropy_split=True)
    labels = [rng.integers(0, K, size=len(Z)).astype(np.int32) for Z in Zs]
    Sl = beng.label_stats(labels, K)
    bad = {}
    for length, Z in enumerate(Zs):
        n, sx, sxx, scal, _ = oracle(Z, c[length], b[length], W[length])
        errs = {"n": qerr(S[length].n[:, None], n[:, None]), "sx": qerr(S[length].sx, sx), "sxx": qerr(S[length].sxx, sxx),
                "scalars": qerr(sc[length], scal)}
        print(f"chain length {length}: {errs}")
        if not max(errs.values()) <= TOL:
            bad[length] = errs
        try:
            check_stats(Sl[length], Z, labels[length], K)
        except AssertionError as e:
            bad[(length, "labels")] = str(e)[:200]
    assert not bad, f"chain lengths with wrong sums: {bad}"


# ---- d. coverage boundary -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", range(1, 17))
def test_coverage_boundary(beng, solo, D):
    """At K = Kmax(Dz) all three entry points run and agree with the oracle; at Kmax(Dz) + 1 each one refuses; a legal
    pass afterwards returns the bits it returned before."""
    K = kmax(D)
    rng = np.random.default_rng(900 + D)
    rows = [40, 0, 3]
    Zs, c, b, W = problems(rng, rows, D, K)
    seeds, u = draws_for(rng, rows)
    beng.upload(Zs)
    before = softmax_pass(beng, solo, Zs, c, b, W)
    draw_pass(beng, solo, Zs, c, b, W, seeds, u)
    given_pass(beng, solo, Zs, K, rng)
    _, c1, b1, W1 = problems(rng, rows, D, K + 1)
    with pytest.raises(_lib.MimoHipError):
        beng.estep(c1, b1, W1)
    with pytest.raises(_lib.MimoHipError):
        beng.gibbs_labels(c1, b1, W1, seeds=seeds)
    with pytest.raises(_lib.MimoHipError):
        beng.gibbs_labels(c1, b1, W1, u=u)
    with pytest.raises(_lib.MimoHipError):
        beng.label_stats([np.zeros(n, np.int32) for n in rows], K + 1)
    S, sc = beng.estep(c, b, W, keep_lse=True, entropy_split=True)
    assert same_bits(packed(S), before[0]) and np.array_equal(sc, before[1]) and same_bits(beng.get_lse(), before[2])


# ---- e. batch layout and reuse ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", [(2, 100), (13, 49)])
def test_all_empty_batch(beng, D, K):
    rng = np.random.default_rng(3)
    rows = [0] * 5
    Zs, c, b, W = problems(rng, rows, D, K)
    beng.upload(Zs)
    S, sc = beng.estep(c, b, W, keep_lse=True, entropy_split=True)
    assert all(not p.any() for p in packed(S)) and not sc.any()
    assert all(x.shape == (0,) for x in beng.get_lse())
    S, sc = beng.estep(c, b, W)
    assert all(not p.any() for p in packed(S)) and not sc[:, 0].any() and np.isnan(sc[:, 1:]).all()
    for kw in ({"seeds": [1, 2, 3, 4, 5]}, {"u": [np.zeros(0)] * 5}):
        labs, S = beng.gibbs_labels(c, b, W, **kw)
        assert all(x.shape == (0,) and x.dtype == np.int32 for x in labs) and all(not p.any() for p in packed(S))
        assert all(x.shape == (0,) for x in beng.get_labels())
        assert all(not p.any() for p in packed(beng.label_stats(None, K)))
    S = beng.label_stats([np.zeros(0, np.int32)] * 5, K)
    assert all(not p.any() for p in packed(S))


@pytest.mark.parametrize("D,K", [(3, 17), (9, 70)])
def test_empty_problems_first_last_and_in_runs(beng, solo, D, K):
    rng = np.random.default_rng(41 * D + K)
    rows = [0, 0, 700, 0, 0, 0, 33, 1, 0, 0, 2500, 0]
    Zs, c, b, W = problems(rng, rows, D, K)
    seeds, u = draws_for(rng, rows)
    beng.upload(Zs)
    softmax_pass(beng, solo, Zs, c, b, W)
    draw_pass(beng, solo, Zs, c, b, W, seeds, u)
    given_pass(beng, solo, Zs, K, rng)


def _all_modes(eng, Zs, c, b, W, seeds, u, labels):
    """Every output of every mode of one batch, as a flat list of arrays."""
    K = c.shape[1]
    eng.upload(Zs)
    S, sc = eng.estep(c, b, W, keep_lse=True, entropy_split=True)
    out = packed(S) + [sc] + eng.get_lse()
    L, G = eng.gibbs_labels(c, b, W, seeds=seeds, sweep=SWEEP)
    out += L + packed(G)
    L, G = eng.gibbs_labels(c, b, W, u=u)
    out += L + packed(G)
    out += packed(eng.label_stats(labels, K))
    return out


def test_context_reuse(beng):
    """One context takes a large batch, a small one, a larger K, a smaller K, fewer and more problems: each result is
    bit-identical to a fresh engine's (stale partial blocks, operand images, work tables or label arrays would show)."""
    rng = np.random.default_rng(59)
    steps = [([20449, 33, 0, 5000], 8, 64), ([31, 1], 8, 64), ([40, 0, 3000], 8, 128), ([3000, 40, 0], 8, 5),
             ([1], 2, 100), ([600, 0, 600, 33, 32801], 2, 37), ([0, 0], 2, 37), ([77], 14, 80)]
    runs = []
    for rows, D, K in steps:
        Zs, c, b, W = problems(rng, rows, D, K)
        seeds, u = draws_for(rng, rows)
        labels = [rng.integers(0, K, size=n).astype(np.int32) for n in rows]
        runs.append((Zs, c, b, W, seeds, u, labels))
    used = [_all_modes(beng, *r) for r in runs]
    for r, got in zip(runs, used):
        fresh = BatchedHipEngine(0)
        try:
            want = _all_modes(fresh, *r)
        finally:
            fresh.close()
        assert same_bits(got, want), [len(z) for z in r[0]]
    # and against the oracle, so that "identical" is not "identically wrong"
    Zs, c, b, W, seeds, u, labels = runs[-3]
    beng.upload(Zs)
    S, sc = beng.estep(c, b, W, keep_lse=True, entropy_split=True)
    lse = beng.get_lse()
    for i, Z in enumerate(Zs):
        check_against(S[i], sc[i], lse[i], oracle(Z, c[i], b[i], W[i]))


# ---- f. hard inputs -----------------------------------------------------------------------------------------------------
def _far_clusters(rng, n, D, K, live):
    """Tight clusters, far apart: for most (row, component) pairs l - max < -745, the responsibility is exactly 0 in
    float64.  Components outside `live` are switched off."""
    centres = 12. * np.sqrt(3. / D) * rng.standard_normal((K, D))      # squared distances ~ 864 chi2_D / D at every Dz
    lab = rng.choice(live, size=n)
    Z = centres[lab] + rng.standard_normal((n, D)) / np.sqrt(3.)
    W = np.stack(K * [np.eye(D)]) * rng.uniform(3., 4., K)[:, None, None]
    b = np.einsum('kde,ke->kd', W, centres)
    c = -0.5 * np.einsum('kd,kd->k', centres, b) + rng.standard_normal(K)
    c[np.setdiff1d(np.arange(K), live)] = -np.inf
    return Z, c, b, W


@pytest.mark.parametrize("D,K,dead", [(3, 40, (16, 32)), (3, 128, (64, 128)), (12, 40, (16, 32)), (9, 128, (64, 128))])
def test_hard_inputs(beng, solo, D, K, dead):
    """A whole 16-component row block (K = 40) or a whole softmax chunk of RBW = 2 (K = 128, components 64 .. 127)
    switched off; a single live component; clusters so far apart that most responsibilities are exactly 0; each next to
    an ordinary problem in the same batch."""
    rng = np.random.default_rng(17 * D + K)
    rows = [700, 1500, 333, 3001, 40]
    Zs, c, b, W = problems(rng, rows, D, K, off=None)
    c[1, dead[0]:dead[1]] = -np.inf                         # problem 1: the row block / chunk off
    c[2, :] = -np.inf                                       # problem 2: one live component, in the last row block
    c[2, K - 3] = 0.25
    live = np.setdiff1d(np.arange(K), np.arange(*dead))
    Zs[3], c[3], b[3], W[3] = _far_clusters(rng, rows[3], D, K, live)         # problem 3: far clusters, the block off too
    Zs[4], c[4], b[4], W[4] = _far_clusters(rng, rows[4], D, K, np.arange(K))
    with np.errstate(invalid='ignore'):
        L3 = O.canonical_eval(Zs[3], c[3], b[3], W[3])
    r3 = np.exp(L3 - O.logsumexp(L3, axis=0))
    assert (r3[live] == 0).mean() > 0.5                     # the premise: most responsibilities are exactly 0
    seeds, u = draws_for(rng, rows)
    beng.upload(Zs)
    Ssm, scal, lse = softmax_pass(beng, solo, Zs, c, b, W)
    assert np.isfinite(np.concatenate(lse)).all()
    draws = draw_pass(beng, solo, Zs, c, b, W, seeds, u)
    for mode in ("host", "philox"):
        assert np.all(draws[mode][0][2] == K - 3)           # the single live component takes every row
    given_pass(beng, solo, Zs, K, rng)
