"""GPU: one BatchedHipEngine through a sequence of every kind of batched call — what single-call tests cannot see.  The entry
points share the operand image's buffers (theta_h / theta_d), the partial blocks, the result block (S_d / S_h) and the staged
table (win), and each leaves some of the resident tables valid and drops others.  K alternates between 3 and 17 (one and two
row blocks of 16), so the image and the partial blocks grow in the middle of the sequence.  Every returned array equals, bit
for bit, what a fresh engine returns that made only that call and its prerequisites; after every step each getter succeeds or
raises as the residency rules say."""
import numpy as np
import pytest

import batched_checks as bc
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine

pytestmark = pytest.mark.gpu

D = 2
ROWS = (0, 1, 2 * bc.TILE + 1)       # an empty problem, a single row, more than one tile with a ragged tail
B = len(ROWS)
K_LO, K_HI = 3, 17
GETTERS = ("get_lse", "get_labels", "get_resp", "get_row_weights", "vi_run")


def _prior(rng, nb, K):
    m0 = rng.standard_normal((nb, K, D))
    kap = rng.uniform(0.05, 0.5, size=(nb, K))
    G = rng.standard_normal((nb, K, D, D)) / np.sqrt(D)
    P0 = np.eye(D) + G @ np.swapaxes(G, 2, 3)
    P0 = 0.5 * (P0 + np.swapaxes(P0, 2, 3))
    return dict(alpha0=rng.uniform(0.5, 2.0, size=(nb, K)), pa=kap[..., None] * m0, pb=kap,
                pc=P0 + kap[..., None, None] * (m0[..., :, None] * m0[..., None, :]), pd=np.full((nb, K), 2.0),
                prior_logZ=rng.standard_normal((nb, K)))


class _Inputs:
    def __init__(self):
        rng = np.random.default_rng(20)
        self.Z, *self.lo = bc.problems(rng, ROWS, D, K_LO)
        _, *self.hi = bc.problems(rng, ROWS, D, K_HI)
        self.seeds = np.array([11, 12, 13], dtype=np.uint64)
        n2 = ROWS[2]
        # an empty selection, a duplicated index, a selection longer than one tile (any order, with repeats)
        self.sel = [np.zeros(0, dtype=np.int64), np.array([0, 0, 0]), rng.integers(0, n2, size=bc.TILE + 9)]
        self.w = [rng.random(n) + 0.25 for n in ROWS]
        self.prior_hi, self.prior_lo = _prior(rng, B, K_HI), _prior(rng, B, K_LO)
        # prediction: B = 2 models, dx = dy = 1, K = 2, one x block for both
        pb, pk = 2, 2
        a = rng.standard_normal((pb, pk, 2, 2))
        self.pred = dict(x=rng.standard_normal((5, 1)), c=rng.standard_normal((pb, pk)), b=rng.standard_normal((pb, pk, 1)),
                         W=rng.uniform(0.5, 2.0, size=(pb, pk, 1, 1)), M=rng.standard_normal((pb, pk, 1, 2)),
                         Q=a @ np.swapaxes(a, 2, 3) + 0.5 * np.eye(2), Cc=rng.uniform(0.5, 2.0, size=(pb, pk, 1, 1)))
        # the shared batch of the last step
        self.Zs = rng.standard_normal((2 * bc.TILE + 1, D)) * 1.5
        _, *self.shared = bc.problems(rng, (1, 1), D, K_HI)
        self.log_gating = np.log([0.3, 0.7])


def _flat(r):
    """A call's result as a flat list of arrays (SuffStats by their parts, None skipped)."""
    if r is None:
        return []
    if isinstance(r, (list, tuple)):
        return [a for x in r for a in _flat(x)]
    if isinstance(r, dict):
        return [a for k in sorted(r) for a in _flat(r[k])]
    if hasattr(r, "sxx"):
        return [r.n, r.sx, r.sxx]
    return [np.asarray(r)]


def _same_bits(got, want, step):
    got, want = _flat(got), _flat(want)
    assert len(got) == len(want) and got, step
    for i, (x, y) in enumerate(zip(got, want)):
        assert x.shape == y.shape and x.dtype == y.dtype, (step, i, x.shape, y.shape)
        if x.dtype == np.float64:
            nan = np.isnan(x) & np.isnan(y)          # the NaN scalars of a pass without the entropy split
            x, y = np.where(nan, 0.0, x).view(np.uint64), np.where(nan, 0.0, y).view(np.uint64)
        assert np.array_equal(x, y), (step, i)


def _getter(eng, name, K):
    if name == "get_resp":
        return eng.get_resp(K)
    if name == "vi_run":
        return eng.vi_run(K, 1, 0.)
    return getattr(eng, name)()


def _residency(eng, works, K):
    """Each getter in `works` succeeds, every other one raises MIMO_E_STATE.  (vi_run changes what is resident, so it is only
    ever asked where it must raise.)"""
    assert "vi_run" not in works
    for name in GETTERS:
        if name in works:
            _getter(eng, name, K)
        else:
            with pytest.raises(_lib.MimoHipError, match=f"libmimo_hip error {_lib.E_STATE}:"):
                _getter(eng, name, K)


def test_every_call_in_sequence_equals_the_call_alone():
    I = _Inputs()

    def _fresh(shared=False):
        e = BatchedHipEngine(0)
        if shared:
            e.upload_shared(I.Zs, 2)
        else:
            e.upload(I.Z)
        return e

    eng = BatchedHipEngine(0)
    eng.upload(I.Z)
    _residency(eng, (), K_LO)

    def step(name, call, works, K, prereq=None, fresh=None, also=()):
        """call(engine) on the sequence engine and on a fresh one (after prereq(fresh)); `also`: getters whose output is compared too."""
        f = fresh() if fresh else _fresh()
        if prereq:
            prereq(f)
        got, want = call(eng), call(f)
        _same_bits(got, want, name)
        for g in also:
            _same_bits(_getter(eng, g, K), _getter(f, g, K), (name, g))
        f.close()
        _residency(eng, works, K)
        return got

    # 1 .. 4: softmax pass with a kept lse, label draw at two row blocks, statistics of the resident labels, minibatch pass
    step("1 estep keep_lse", lambda e: e.estep(*I.lo, keep_lse=True), ("get_lse",), K_LO, also=("get_lse",))
    step("2 gibbs_labels", lambda e: e.gibbs_labels(*I.hi, seeds=I.seeds, sweep=3), ("get_labels",), K_HI, also=("get_labels",))
    step("3 label_stats resident", lambda e: e.label_stats(None, K_HI), ("get_labels",), K_HI,
         prereq=lambda e: e.gibbs_labels(*I.hi, seeds=I.seeds, sweep=3))
    step("4 estep rows", lambda e: e.estep(*I.hi, rows=I.sel, entropy_split=True), (), K_HI)
    # 5 .. 8: random start and its resident table, weighted pass from host weights and from the resident ones
    step("5 random_resp_stats", lambda e: e.random_resp_stats(K_LO, I.seeds), ("get_resp",), K_LO, also=("get_resp",))
    step("6 weighted_stats resident", lambda e: e.weighted_stats(None, K_LO), ("get_resp",), K_LO,
         prereq=lambda e: e.random_resp_stats(K_LO, I.seeds))
    step("7 estep weighted", lambda e: e.estep(*I.hi, row_weights=I.w), ("get_row_weights",), K_HI, also=("get_row_weights",))
    step("8 estep resident weights", lambda e: e.estep(*I.hi, row_weights='resident'), ("get_row_weights",), K_HI,
         prereq=lambda e: e.estep(*I.hi, row_weights=I.w), also=("get_row_weights",))
    # 9: prediction reads nothing of the batch (its B differs) but takes the result block: with a prior of this K resident the
    # loop would run on step 8's statistics before it, and refuses after it
    eng.vi_set_prior(**I.prior_hi)
    step("9 predict", lambda e: e.predict(**I.pred), ("get_row_weights",), K_HI, fresh=lambda: BatchedHipEngine(0))
    with pytest.raises(_lib.MimoHipError, match=f"libmimo_hip error {_lib.E_STATE}: mimo_vi_run_batched: no statistics are resident"):
        eng.vi_run(K_HI, 1, 0.)
    # 10, 11: back to one row block; the resident loop on the statistics of step 10
    step("10 estep", lambda e: e.estep(*I.lo), ("get_row_weights",), K_LO)

    def vi(e):
        e.vi_set_prior(**I.prior_lo)
        return e.vi_run(K_LO, 2, 0.), e.vi_state(K_LO), e._vi_resident(K_LO)

    f = _fresh()                                 # (step 11 is the one place where vi_run must succeed: the call is the check)
    f.estep(*I.lo)
    got, want = vi(eng), vi(f)
    _same_bits(got, want, "11 vi_run")
    assert list(got[0][1]) == [2] * B            # n_done: tol = 0 stops nobody
    f.close()
    for name in ("get_lse", "get_labels", "get_resp"):
        with pytest.raises(_lib.MimoHipError, match=f"libmimo_hip error {_lib.E_STATE}:"):
            _getter(eng, name, K_LO)
    eng.get_row_weights()
    # 12: a shared batch on the same engine
    eng.upload_shared(I.Zs, 2)
    _residency(eng, (), K_HI)
    f = _fresh(shared=True)
    _same_bits(eng.estep(*I.shared, keep_lse=True), f.estep(*I.shared, keep_lse=True), "12 estep keep_lse")
    _same_bits(eng.get_lse(), f.get_lse(), "12 lse")
    _residency(eng, ("get_lse",), K_HI)
    _same_bits(eng.outer_responsibilities(I.log_gating), f.outer_responsibilities(I.log_gating), "12 outer")
    _same_bits(eng.get_row_weights(), f.get_row_weights(), "12 outer weights")
    _residency(eng, ("get_lse", "get_row_weights"), K_HI)
    _same_bits(eng.estep(*I.shared, row_weights='resident'), f.estep(*I.shared, row_weights='resident'), "12 estep resident")
    _residency(eng, ("get_row_weights",), K_HI)
    f.close()
    eng.close()
