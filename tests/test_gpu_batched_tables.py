"""GPU: the batched table passes (mimo_weighted_stats_batched / mimo_random_resp_stats_batched through
BatchedHipEngine.weighted_stats / random_resp_stats / get_resp) and the batched driver's random start.

Reference throughout: the NumPy oracle on each problem's rows alone (long problems in row chunks) and a solo HipEngine
pass over the same rows; TOL and qerr are the batched path's own (batched_checks).  The Philox table is compared bit for
bit with the solo engine's and within 2 ulp with the oracle's construction v / sum(v): the kernels multiply by ONE
reciprocal of the same sum (<= 1 ulp from the reciprocal's rounding, <= 1/2 ulp from the product's), the oracle divides
(<= 1/2 ulp)."""
import numpy as np
import numpy.random as npr
import pytest

from batched_checks import TOL, kmax, problems, qerr
from conftest import rel_err
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.engine import HipEngine, _ptr
from mimo_amd.mixtures.batched import meanfield_coordinate_descent_batched
from oracle import mimo_oracle as O
from test_gpu_batched_coverage import CELLS
from test_gpu_batched_driver import _models, _posterior, _solo

pytestmark = pytest.mark.gpu

CASES = [  # (rows, Dz, K): the table of tests/test_gpu_batched.py
    ([4099], 2, 4),
    ([0, 33, 31], 1, 1),
    ([0, 1, 31, 32, 33, 4099], 1, 4),
    ([4099, 0, 1, 31, 32, 33], 2, 50),
    ([33, 4099, 0, 1, 31, 32], 2, 128),
    ([1, 0, 4099, 32], 2, 100),
    ([31, 32, 4099, 0, 1, 33], 11, 128),
    ([32, 4099, 1], 11, 4),
    ([0, 1, 31, 32, 33, 4099], 11, 50),
    ([4099, 33, 0, 1], 16, 64),
    ([1, 32, 31], 16, 1),
]
CELL_ROWS = [33, 0, 4099]
START_SHAPES = [(2, 4), (2, 100), (11, 128), (16, 64)]
START_ROWS = [4099, 0, 1, 33]


@pytest.fixture(scope="module")
def beng():
    return BatchedHipEngine(0)


@pytest.fixture(scope="module")
def solo():
    return HipEngine(0)


def tables_for(rng, rows, K):
    """Random weights as a caller may hand them in: unnormalised, negative entries, one all-zero column per problem."""
    tables = [rng.standard_normal((K, n)) * 1.5 + 0.25 for n in rows]
    for t in tables:
        if t.shape[1]:
            t[:, t.shape[1] // 2] = 0.0
    return tables


def table_oracle(Z, table, chunk=8192):
    """(n, sx, sxx) of a (K, N) weight table, naively, in row chunks."""
    K, D = table.shape[0], Z.shape[1]
    n, sx, sxx = np.zeros(K), np.zeros((K, D)), np.zeros((K, D, D))
    for i in range(0, len(Z), chunk):
        dn, dsx, dsxx = O.packed_stats(Z[i:i + chunk], table[:, i:i + chunk])
        n += dn; sx += dsx; sxx += dsxx
    return n, sx, sxx


def stat_errs(S, ref):
    n, sx, sxx = ref
    return {"n": qerr(S.n[:, None], np.asarray(n)[:, None]), "sx": qerr(S.sx, sx), "sxx": qerr(S.sxx, sxx)}


def check_table_stats(S, ref, what):
    errs = stat_errs(S, ref)
    print(what, errs)
    assert max(errs.values()) <= TOL, (what, errs)


def packed(S):
    return [s.packed() for s in S]


def same_bits(A, B):
    return len(A) == len(B) and all(np.array_equal(x, y) for x, y in zip(A, B))


# ---- 1. the weights mode against the oracle and a solo pass -------------------------------------------------------------
@pytest.mark.parametrize("rows,D,K", CASES)
def test_weights_equal_solo_and_oracle(beng, solo, rows, D, K):
    rng = np.random.default_rng(100 * D + K + len(rows))
    Zs = problems(rng, rows, D, K)[0]
    tables = tables_for(rng, rows, K)
    beng.upload(Zs)
    S = beng.weighted_stats(tables)
    assert len(S) == len(rows)
    for i, Z in enumerate(Zs):
        check_table_stats(S[i], table_oracle(Z, tables[i]), f"problem {i} ({len(Z)} rows) against the oracle")
        if len(Z) == 0:
            assert not S[i].packed().any()
            continue
        solo.upload(Z)
        S1 = solo.weighted_stats(tables[i])
        check_table_stats(S[i], (S1.n, S1.sx, S1.sxx), f"problem {i} ({len(Z)} rows) against the solo pass")


# ---- 2. every instantiation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", CELLS)
def test_every_instantiation(beng, D, K):
    rng = np.random.default_rng(1000 * D + K)
    Zs = problems(rng, CELL_ROWS, D, K)[0]
    tables = tables_for(rng, CELL_ROWS, K)
    beng.upload(Zs)
    S = beng.weighted_stats(tables)
    for i, Z in enumerate(Zs):
        check_table_stats(S[i], table_oracle(Z, tables[i]), f"Dz = {D}, K = {K}, problem {i}")


@pytest.mark.parametrize("D", [2, 12, 14, 16])
def test_coverage_boundary(beng, D):
    K = kmax(D)
    rng = np.random.default_rng(900 + D)
    rows = [40, 0, 3]
    Zs = problems(rng, rows, D, K)[0]
    tables = tables_for(rng, rows, K)
    beng.upload(Zs)
    before = beng.weighted_stats(tables)
    for i, Z in enumerate(Zs):
        check_table_stats(before[i], table_oracle(Z, tables[i]), f"Dz = {D}, K = Kmax = {K}, problem {i}")
    with pytest.raises(_lib.MimoHipError):
        beng.weighted_stats(tables_for(rng, rows, K + 1))
    with pytest.raises(_lib.MimoHipError):
        beng.random_resp_stats(K + 1, [1, 2, 3])
    assert same_bits(packed(beng.weighted_stats(tables)), packed(before))


# ---- 3. the random start ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", START_SHAPES)
def test_random_start(beng, solo, D, K):
    rng = np.random.default_rng(55 * D + K)
    # the issue's rows, and a copy of the last problem (same rows, same seed) behind them
    rows = START_ROWS + START_ROWS[-1:]
    Zs, c, b, W = problems(rng, rows, D, K)
    Zs[4] = Zs[3].copy()
    seeds = [int(s) for s in rng.integers(0, 2**63, size=3)]
    seeds = seeds + [seeds[0], seeds[0]]                  # problems 0, 3 and 4 share a key
    beng.upload(Zs)
    S = beng.random_resp_stats(K, seeds)
    resp = beng.get_resp()
    assert len(resp) == len(rows)
    for i, Z in enumerate(Zs):
        n = len(Z)
        assert resp[i].shape == (K, n)
        v = np.stack([O.philox_uniforms(seeds[i], np.arange(n), k) for k in range(K)]) + 2.0 ** -53 if n else np.zeros((K, 0))
        tot = np.zeros(n)
        for k in range(K):                                # k ascending, like the kernels (no pairwise summation)
            tot += v[k]
        want = v / tot
        assert np.all(np.abs(resp[i] - want) <= 2 * np.spacing(np.maximum(resp[i], want))), (i, np.abs(resp[i] - want).max())
        check_table_stats(S[i], table_oracle(Z, want), f"problem {i} ({n} rows) against the oracle")
        if n == 0:
            assert not S[i].packed().any()
            continue
        solo.upload(Z)
        S1 = solo.random_resp_stats(K, seeds[i])
        assert np.array_equal(resp[i], solo.get_resp()), (i, n)
        check_table_stats(S[i], (S1.n, S1.sx, S1.sxx), f"problem {i} ({n} rows) against the solo pass")
    # the counter is the LOCAL row: the shorter problem's table is the head of the longer one's under the same key
    assert np.array_equal(resp[3], resp[0][:, :rows[3]])
    # equal seed and equal rows: identical blocks
    assert np.array_equal(resp[4], resp[3]) and np.array_equal(S[4].packed(), S[3].packed())
    # the resident table gives the same statistics, bit for bit; so does the table handed back in
    assert same_bits(packed(beng.weighted_stats(None, K)), packed(S))
    assert same_bits(packed(beng.weighted_stats(resp)), packed(S))
    assert same_bits(beng.get_resp(), resp)               # a host table does not replace the resident one
    # another K than the resident table's, and a softmax pass (which invalidates the table): MIMO_E_STATE
    with pytest.raises(_lib.MimoHipError, match=f"error {_lib.E_STATE}"):
        beng.weighted_stats(None, K + 1 if K < kmax(D) else K - 1)
    beng.estep(c, b, W)
    with pytest.raises(_lib.MimoHipError, match=f"error {_lib.E_STATE}"):
        beng.weighted_stats(None, K)
    with pytest.raises(_lib.MimoHipError):
        beng.get_resp()
    # ... and so does a new upload
    beng.random_resp_stats(K, seeds)
    beng.upload(Zs)
    with pytest.raises(_lib.MimoHipError, match=f"error {_lib.E_STATE}"):
        beng.weighted_stats(None, K)


# ---- 4. independence and determinism ------------------------------------------------------------------------------------
def test_independence_and_determinism(beng):
    rng = np.random.default_rng(11)
    D, K = 8, 32
    rows = [4099, 1000, 33]
    Zs = problems(rng, rows, D, K)[0]
    tables = tables_for(rng, rows, K)
    seeds = [5, 6, 7]
    beng.upload(Zs)
    S0 = packed(beng.weighted_stats(tables))
    assert same_bits(packed(beng.weighted_stats(tables)), S0)            # two runs: bit-identical
    R0 = packed(beng.random_resp_stats(K, seeds))
    T0 = beng.get_resp()
    assert same_bits(packed(beng.random_resp_stats(K, seeds)), R0) and same_bits(beng.get_resp(), T0)
    # problem 0's rows, row count, table and seed change: problems 1 and 2 do not move by a bit
    Zs2 = [rng.standard_normal((777, D))] + Zs[1:]
    tables2 = [rng.standard_normal((K, 777))] + tables[1:]
    beng.upload(Zs2)
    S2 = packed(beng.weighted_stats(tables2))
    R2 = packed(beng.random_resp_stats(K, [99] + seeds[1:]))
    T2 = beng.get_resp()
    for i in (1, 2):
        assert np.array_equal(S2[i], S0[i]) and np.array_equal(R2[i], R0[i]) and np.array_equal(T2[i], T0[i])
    assert not np.array_equal(R2[0][:, 0], R0[0][:, 0])
    # a problem alone and in a batch of five copies: the same bits
    beng.upload([Zs[1]])
    Sa = packed(beng.weighted_stats(tables[1:2]))
    Ra = packed(beng.random_resp_stats(K, seeds[1:2]))
    beng.upload([Zs[1]] * 5)
    Sc = packed(beng.weighted_stats([tables[1]] * 5))
    Rc = packed(beng.random_resp_stats(K, [seeds[1]] * 5))
    for i in range(5):
        assert np.array_equal(Sc[i], Sa[0]) and np.array_equal(Sc[i], S0[1])
        assert np.array_equal(Rc[i], Ra[0]) and np.array_equal(Rc[i], R0[1])


@pytest.mark.parametrize("D,K", [(2, 100), (13, 49)])
def test_all_empty_batch(beng, D, K):
    rng = np.random.default_rng(3)
    Zs = problems(rng, [0] * 5, D, K)[0]
    beng.upload(Zs)
    assert all(not p.any() for p in packed(beng.weighted_stats([np.zeros((K, 0))] * 5)))
    assert all(not p.any() for p in packed(beng.random_resp_stats(K, [1, 2, 3, 4, 5])))
    assert all(t.shape == (K, 0) for t in beng.get_resp())
    assert all(not p.any() for p in packed(beng.weighted_stats(None, K)))


# ---- 5. errors ----------------------------------------------------------------------------------------------------------
def test_errors(beng, solo):
    rng = np.random.default_rng(6)
    D, K, rows = 3, 4, [40, 3]
    Zs = problems(rng, rows, D, K)[0]
    tables = tables_for(rng, rows, K)
    lib = beng._lib
    flat = np.ascontiguousarray(np.concatenate([t.reshape(-1) for t in tables]))
    seeds = np.array([1, 2], dtype=np.uint64)
    S = np.empty((2, K, 1 + D + D * D))
    # contexts without a batch: a fresh batched engine, and a single-problem context
    fresh = BatchedHipEngine(0)
    try:
        with pytest.raises(_lib.MimoHipError):
            fresh.weighted_stats(None, K)
        with pytest.raises(_lib.MimoHipError):
            fresh.random_resp_stats(K, [])
    finally:
        fresh.close()
    solo.upload(np.concatenate(Zs))
    assert lib.mimo_weighted_stats_batched(solo._ctx, _ptr(flat), K, 0, _ptr(S)) == _lib.E_INVALID
    assert b"batch" in lib.mimo_last_error(solo._ctx)
    assert lib.mimo_random_resp_stats_batched(solo._ctx, K, _ptr(seeds), 0, _ptr(S)) == _lib.E_INVALID
    # flags, NULL results, NULL seeds
    beng.upload(Zs)
    ctx = beng._ctx
    assert lib.mimo_weighted_stats_batched(ctx, _ptr(flat), K, _lib.F_NO_STATS, _ptr(S)) == _lib.E_INVALID
    assert lib.mimo_weighted_stats_batched(ctx, _ptr(flat), K, 0, None) == _lib.E_INVALID
    assert lib.mimo_random_resp_stats_batched(ctx, K, _ptr(seeds), _lib.F_NO_STATS, _ptr(S)) == _lib.E_INVALID
    assert lib.mimo_random_resp_stats_batched(ctx, K, _ptr(seeds), 0, None) == _lib.E_INVALID
    assert lib.mimo_random_resp_stats_batched(ctx, K, None, 0, _ptr(S)) == _lib.E_INVALID
    assert lib.mimo_weighted_stats_batched(ctx, None, K, 0, _ptr(S)) == _lib.E_STATE          # no table is resident
    assert lib.mimo_weighted_stats_batched(ctx, _ptr(flat), 0, 0, _ptr(S)) == _lib.E_INVALID   # K < 1
    # malformed arguments never reach the library
    with pytest.raises(ValueError):
        beng.weighted_stats(tables[:1])
    with pytest.raises(ValueError):
        beng.weighted_stats([tables[0], tables[1][:, :2]])
    with pytest.raises(ValueError):
        beng.random_resp_stats(K, [1])
    # another structure: the pass refuses, and works again under the full one
    beng.set_structure('diag')
    try:
        with pytest.raises(_lib.MimoHipError):
            beng.weighted_stats(tables)
        with pytest.raises(_lib.MimoHipError):
            beng.random_resp_stats(K, [1, 2])
    finally:
        beng.set_structure('full')
    # the pass still runs after all of that
    Sw = beng.weighted_stats(tables)
    Sr = beng.random_resp_stats(K, [1, 2])
    for i, Z in enumerate(Zs):
        check_table_stats(Sw[i], table_oracle(Z, tables[i]), f"weights, problem {i}")
        check_table_stats(Sr[i], table_oracle(Z, beng.get_resp()[i]), f"random start, problem {i}")


# ---- 6. the driver ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gmm_c1_d2_k4_dir", "ilr_dx1_dy1_k6_dir"])
def test_driver_start_uses_no_solo_engine(engine, beng, monkeypatch, name):
    kw = dict(randomize=True, tol=0., maxiter=12, sample_likelihood=False)
    B = 4
    seeds = [21, 21, 22, 23]

    def refuse(self, *args, **kwargs):
        raise AssertionError("the batched driver's random start went to a solo engine")

    runs = {}
    with monkeypatch.context() as mp:
        mp.setattr(HipEngine, "weighted_stats", refuse)
        mp.setattr(HipEngine, "random_resp_stats", refuse)
        for init_rng in ("philox", "host"):
            _, models, data = _models(name, engine, B=B)
            npr.seed(1234)
            vlbs = meanfield_coordinate_descent_batched(models, data, seeds=seeds, init_rng=init_rng, engine=beng, **kw)
            assert [len(v) for v in vlbs] == [kw["maxiter"]] * B and np.isfinite(np.array(vlbs)).all()
            runs[init_rng] = (models, data, vlbs)
    assert runs["philox"][2][0] == runs["philox"][2][1]             # identical copies under one key: bit-identical traces
    # the solo runs of the same models from the same states: host draws in model order after the same numpy seed
    for init_rng in ("host", "philox"):
        models, data, vlbs = runs[init_rng]
        _, solos, _ = _models(name, engine, B=B)
        npr.seed(1234)
        for m, s, d, seed, v in zip(models, solos, data, seeds, vlbs):
            vs = _solo(s, d, init_rng=init_rng, seed=seed, **kw)
            err = rel_err(np.array(v), np.array(vs))
            perr = max(rel_err(a, b) for a, b in zip(_posterior(m), _posterior(s)))
            print(f"{name} {init_rng}: trace {err:.2e}, posterior {perr:.2e}")
            assert err < 1e-10 and perr < 1e-8, (init_rng, err, perr)
