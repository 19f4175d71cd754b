"""GPU: the row-selection mode of the batched softmax pass (mimo_estep_batched_rows, BatchedHipEngine.estep(rows=...)).

Part A, the contract: problem b gets, bit for bit, what a plain batched pass returns for a batch whose problem b holds
Z_b[rows_b] in that order.  Every cell of test_gpu_batched_coverage.CELLS runs (all 18 (NCB, RBW) instantiations of the
mode, both RBW branches, every Dz) on a batch of five problems with 0, 1, 33, 600 and 2100 rows; the selection sizes
0, 1, 31, 32, 33, 600, 2100 and 2500 and the index patterns rotate over the cells.  References: the plain pass on the same
engine (identity selection), a plain pass on a second engine that uploaded the gathered rows, and on three cells the CPU
oracle at the tolerance of tests/test_gpu_batched.py (batched_checks.TOL).

Part B, the rules around the pass: determinism, non-interference with the upload's own tile split, residency, refusals.

Switched-off components (c = -inf): the softmax carries them at exp(-707), so their statistics are below 1e-290 — the bound
tests/test_gpu_batched_coverage.py states for the plain pass."""
import numpy as np
import pytest

from batched_checks import check_against, kmax, problems
from oracle_engine import OracleEngine
from test_gpu_batched_coverage import CELLS
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.engine import HipEngine, _ptr

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 33, 600, 2100]
# selection sizes of the problems with 1, 33, 600 and 2100 rows (the empty problem's selection is empty): a ragged last tile
# (31, 33, 600, 2100, 2500), a one-row last tile (1, 33), whole tiles (32), more than one workgroup (600 and up: more than
# 4 * 32 * 4 rows), more rows than the problem has (33 of 1, 2500 of 33 / 600 / 2100), an empty selection of a non-empty problem
LAYOUTS = [[0, 31, 2500, 32], [33, 0, 1, 2500], [2100, 600, 33, 0], [32, 2500, 31, 600], [1, 1, 2100, 33]]
PATTERNS = ["reversed", "random", "repeat", "first", "last"]


@pytest.fixture(scope="module")
def beng():
    return BatchedHipEngine(0)


@pytest.fixture(scope="module")
def other():
    return BatchedHipEngine(0)


def pattern(name, n, m, rng):
    if m == 0:
        return np.zeros(0, dtype=np.int64)
    if name == "identity":
        return np.arange(n, dtype=np.int64)
    if name == "reversed":
        return (n - 1 - np.arange(m, dtype=np.int64)) % n
    if name == "random":                                     # with duplicates
        return rng.integers(0, n, size=m).astype(np.int64)
    if name == "repeat":
        return np.full(m, int(rng.integers(0, n)), dtype=np.int64)
    return np.full(m, 0 if name == "first" else n - 1, dtype=np.int64)


def selections(idx, rng):
    sizes = [0] + LAYOUTS[idx % len(LAYOUTS)]
    base = idx // len(LAYOUTS)
    return [pattern(PATTERNS[(base + p) % len(PATTERNS)], n, m, rng) for p, (n, m) in enumerate(zip(ROWS, sizes))]


def packed(S):
    return [s.packed() for s in S]


def same_bits(A, B):
    return len(A) == len(B) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(A, B))


def against_gathered(beng, other, Zs, c, b, W, sel):
    """The selection pass equals a plain pass over the gathered rows on a second engine: S and scalars, bit for bit, with and
    without entropy_split and without statistics."""
    other.upload([Z[r] for Z, r in zip(Zs, sel)])
    for kw in (dict(), dict(entropy_split=True), dict(stats=False), dict(stats=False, entropy_split=True)):
        S, sc = beng.estep(c, b, W, rows=sel, **kw)
        S2, sc2 = other.estep(c, b, W, **kw)
        assert np.array_equal(sc, sc2, equal_nan=True), kw
        if kw.get("stats", True):
            assert same_bits(packed(S), packed(S2)), kw
        else:
            assert S is None
    return beng.estep(c, b, W, rows=sel, entropy_split=True)


# ---- A. the contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(CELLS)), ids=[f"D{D}-K{K}" for D, K in CELLS])
def test_every_cell_equals_a_plain_pass_over_the_gathered_rows(beng, other, idx):
    D, K = CELLS[idx]
    rng = np.random.default_rng(1000 + idx)
    Zs, c, b, W = problems(rng, ROWS, D, K)
    beng.upload(Zs)
    # identity: the plain pass of the same engine
    ident = [pattern("identity", n, n, rng) for n in ROWS]
    for kw in (dict(), dict(entropy_split=True), dict(stats=False)):
        S0, sc0 = beng.estep(c, b, W, **kw)
        S1, sc1 = beng.estep(c, b, W, rows=ident, **kw)
        assert np.array_equal(sc0, sc1, equal_nan=True)
        assert S0 is None and S1 is None or same_bits(packed(S0), packed(S1))
    sel = selections(idx, rng)
    S, sc = against_gathered(beng, other, Zs, c, b, W, sel)
    for i, r in enumerate(sel):
        off = np.flatnonzero(np.isneginf(c[i]))
        assert np.all(S[i].n[off] < 1e-290) and np.all(np.abs(S[i].sxx[off]) < 1e-290)      # c = -inf: nothing
        if len(r) == 0:
            assert not S[i].packed().any() and not sc[i].any()                               # empty selection: zeros
        else:
            assert abs(S[i].n.sum() - len(r)) <= 1e-11 * len(r)


@pytest.mark.parametrize("idx", [1, 19, 34])            # (2, 37): RBW 1; (11, 113): RBW 2; (16, 64): NCB 10
def test_against_the_cpu_oracle(beng, idx):
    D, K = CELLS[idx]
    rng = np.random.default_rng(2000 + idx)
    Zs, c, b, W = problems(rng, ROWS, D, K, off=None)
    beng.upload(Zs)
    for lay in range(len(LAYOUTS)):
        sel = selections(lay + len(LAYOUTS) * idx, rng)
        S, sc = beng.estep(c, b, W, rows=sel, entropy_split=True)
        for i, r in enumerate(sel):
            if len(r) == 0:
                continue
            ref = OracleEngine()
            ref.upload(Zs[i][r])
            Sr, scr = ref.estep(c[i], b[i], W[i], entropy_split=True)
            check_against(S[i], sc[i], np.zeros(0), (Sr.n, Sr.sx, Sr.sxx, scr, np.zeros(0)))


# ---- B. the rules around the pass ----------------------------------------------------------------------------------------
def test_a_problems_block_does_not_depend_on_the_other_selections(beng):
    D, K = 6, 23
    rng = np.random.default_rng(7)
    Zs, c, b, W = problems(rng, ROWS, D, K)
    beng.upload(Zs)
    mine = pattern("random", ROWS[3], 333, rng)
    runs = []
    for others in ([0, 1, 33, 0, 2500], [0, 0, 0, 0, 0], [0, 33, 1, 0, 31]):
        sel = [pattern("random", n, m, rng) for n, m in zip(ROWS, others)]
        sel[3] = mine
        S, sc = beng.estep(c, b, W, rows=sel, entropy_split=True)
        runs.append((S[3].packed(), sc[3]))
    for Sp, scp in runs[1:]:
        assert np.array_equal(Sp, runs[0][0]) and np.array_equal(scp, runs[0][1])


def test_a_selection_pass_leaves_the_uploads_tile_split_alone(beng):
    D, K = 8, 64
    rng = np.random.default_rng(8)
    Zs, c, b, W = problems(rng, ROWS, D, K)
    beng.upload(Zs)
    seeds = [3, 4, 5, 6, 7]
    S0, sc0 = beng.estep(c, b, W, entropy_split=True)
    lab0, L0 = beng.gibbs_labels(c, b, W, seeds=seeds, sweep=2)
    beng.estep(c, b, W, rows=selections(3, rng))
    S1, sc1 = beng.estep(c, b, W, entropy_split=True)
    assert same_bits(packed(S0), packed(S1)) and np.array_equal(sc0, sc1)
    beng.estep(c, b, W, rows=selections(1, rng), stats=False)
    lab1, L1 = beng.gibbs_labels(c, b, W, seeds=seeds, sweep=2)
    assert same_bits(lab0, lab1) and same_bits(packed(L0), packed(L1))


def test_one_context_across_two_shapes_matches_fresh_contexts(beng):
    rng = np.random.default_rng(9)
    got, want = [], []
    shapes = [(12, 96), (2, 37)]
    cases = []
    for j, (D, K) in enumerate(shapes):
        Zs, c, b, W = problems(rng, ROWS, D, K)
        cases.append((Zs, c, b, W, selections(j, rng)))
    for Zs, c, b, W, sel in cases:
        beng.upload(Zs)
        S, sc = beng.estep(c, b, W, rows=sel, entropy_split=True)
        got.append((packed(S), sc))
    for Zs, c, b, W, sel in cases:
        fresh = BatchedHipEngine(0)
        try:
            fresh.upload(Zs)
            S, sc = fresh.estep(c, b, W, rows=sel, entropy_split=True)
            want.append((packed(S), sc))
        finally:
            fresh.close()
    for (Sg, scg), (Sw, scw) in zip(got, want):
        assert same_bits(Sg, Sw) and np.array_equal(scg, scw)


def test_a_selection_pass_ends_the_residency_of_a_random_table(beng):
    D, K = 3, 17
    rng = np.random.default_rng(10)
    Zs, c, b, W = problems(rng, ROWS, D, K)
    beng.upload(Zs)
    beng.random_resp_stats(K, [1, 2, 3, 4, 5])
    beng.weighted_stats(None, K)                          # resident
    beng.estep(c, b, W, rows=selections(0, rng))
    with pytest.raises(_lib.MimoHipError, match=f"error {_lib.E_STATE}"):
        beng.weighted_stats(None, K)


def _call(lib, ctx, c, b, W, K, rows, off, flags, S, sc):
    rows, off = np.ascontiguousarray(rows, dtype=np.int64), np.ascontiguousarray(off, dtype=np.int64)
    return lib.mimo_estep_batched_rows(ctx, _ptr(c), _ptr(b), _ptr(W), K, _ptr(rows), _ptr(off), flags, _ptr(S), _ptr(sc))


def test_refusals_leave_the_context_usable(beng, other):
    lib = _lib.load()
    D, K = 4, 20
    rows = [5, 0, 40]
    rng = np.random.default_rng(11)
    Zs, c, b, W = problems(rng, rows, D, K)
    beng.upload(Zs)
    ctx = beng._ctx
    S, sc = np.empty((3, K, 1 + D + D * D)), np.empty((3, 3))
    good = (np.array([4, 0, 4, 39, 0]), np.array([0, 3, 3, 5]))

    def check_usable():
        sel = [np.array([4, 0, 4]), np.zeros(0, dtype=np.int64), np.array([39, 0])]
        against_gathered(beng, other, Zs, c, b, W, sel)

    assert _call(lib, ctx, c, b, W, K, *good, 0, S, sc) == 0
    bad = [(np.array([5, 0, 4, 39, 0]), good[1], b"problem 0"),                  # index N_b
           (np.array([4, 0, 4, 40, 0]), good[1], b"problem 2"),
           (np.array([4, -1, 4, 39, 0]), good[1], b"-1"),                       # index -1
           (good[0], np.array([0, 3, 2, 5]), b"sel_off"),                        # decreasing
           (good[0], np.array([1, 3, 3, 5]), b"sel_off[0]"),                     # sel_off[0] != 0
           (np.array([4, 0, 4, 0, 0]), np.array([0, 3, 4, 5]), b"problem 1")]    # a non-empty selection of an empty problem
    for r, o, text in bad:
        assert _call(lib, ctx, c, b, W, K, r, o, 0, S, sc) == _lib.E_INVALID
        assert text in lib.mimo_last_error(ctx), (text, lib.mimo_last_error(ctx))
        check_usable()
    r, o = (np.ascontiguousarray(x, dtype=np.int64) for x in good)
    args = (_ptr(c), _ptr(b), _ptr(W), K)
    assert lib.mimo_estep_batched_rows(ctx, *args, None, _ptr(o), 0, _ptr(S), _ptr(sc)) == _lib.E_INVALID
    assert lib.mimo_estep_batched_rows(ctx, *args, _ptr(r), None, 0, _ptr(S), _ptr(sc)) == _lib.E_INVALID
    assert lib.mimo_estep_batched_rows(ctx, *args, _ptr(r), _ptr(o), 0, None, _ptr(sc)) == _lib.E_INVALID
    assert lib.mimo_estep_batched_rows(ctx, *args, _ptr(r), _ptr(o), _lib.F_NO_STATS, None, _ptr(sc)) == 0
    for flag in (_lib.F_KEEP_LSE, _lib.F_DEVICE_IN):
        assert _call(lib, ctx, c, b, W, K, *good, flag, S, sc) == _lib.E_INVALID
    cn = c.copy()
    cn[1, 2] = np.nan
    assert _call(lib, ctx, cn, b, W, K, *good, 0, S, sc) == _lib.E_INVALID
    check_usable()
    with pytest.raises(ValueError):
        beng.estep(c, b, W, rows=[np.array([5]), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)])
    # the 'diag' structure
    beng.set_structure('diag')
    try:
        assert _call(lib, ctx, c, b, W, K, *good, 0, S, sc) == _lib.E_UNSUPPORTED
    finally:
        beng.set_structure('full')
    check_usable()
    # a single-problem context
    solo = HipEngine(0)
    solo.upload(np.concatenate(Zs))
    assert _call(lib, solo._ctx, c, b, W, K, *good, 0, S, sc) == _lib.E_INVALID
    assert b"batch" in lib.mimo_last_error(solo._ctx)


@pytest.mark.parametrize("D", [2, 14])
def test_one_component_too_many_is_unsupported(beng, other, D):
    lib = _lib.load()
    K = kmax(D)
    rows = [40, 7]
    rng = np.random.default_rng(12 + D)
    Zs, c, b, W = problems(rng, rows, D, K + 1)
    beng.upload(Zs)
    sel = [np.array([39, 0, 0]), np.array([6])]
    S, sc = np.empty((2, K + 1, 1 + D + D * D)), np.empty((2, 3))
    assert _call(lib, beng._ctx, c, b, W, K + 1, np.concatenate(sel), [0, 3, 4], 0, S, sc) == _lib.E_UNSUPPORTED
    against_gathered(beng, other, Zs, c[:, :K], b[:, :K], W[:, :K], sel)
