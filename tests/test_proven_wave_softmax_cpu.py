"""The certified E-step's softmax over the live row block on proven waves, on the CPU ("E-step certificates",
the proven wave):

  * the association.  The eight lanes of a row hold eight consecutive slots each and add tree_sum8 of them, then exchange at
    lane ^ 8, ^ 16, ^ 32; a proven wave gives each lane two slots of the row's live block and runs the same three stages.  Both
    are emulated in float64, operation by operation, on rows whose live block holds e in (0, 1] with one entry equal to 1 and
    whose other 48 entries are at most 2^-60 (what the eight-slot lanes see) or absent (what the two-slot lanes see): the sum,
    1 / sum by the kernel's Newton formula and every weight of the live block must be the same bits;
  * how often the path can fire: the share of (tile, wave) pairs of the benchmark model whose eight rows are all proven, per
    lag behind the reference pass, under the passes and the policy of tests/test_estep_certificate_cpu.py."""
import numpy as np

from test_block_order_cpu import blocks_of, partition
from test_estep_certificate_cpu import EPS, LN_TAU, RENEW, T, benchmark_passes, bounds_built, certificates, native


def _newton_inverse(s):
    """1 / s as normalise_tile takes it: a seed and two steps inv = fma(fma(-s, inv, 1), inv, inv).  NumPy has no fma; the seed
    here is the correctly rounded quotient, at which both steps are evaluated in exact rational arithmetic rounded once per fma
    — the two lane maps are given the same function, and equal sums must give equal results."""
    from fractions import Fraction
    out = np.empty_like(s)
    for i, v in enumerate(s):
        inv = 1.0 / v
        for _ in range(2):
            r = float(Fraction(1) - Fraction(v) * Fraction(inv))
            inv = float(Fraction(r) * Fraction(inv) + Fraction(inv))
        out[i] = inv
    return out


def _tree_sum8(v):
    return ((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])) + ((v[:, 4] + v[:, 5]) + (v[:, 6] + v[:, 7]))


def _eight_slot_sum(e):
    """e (rows, 64) -> the sum every lane of the row ends with: lane `part` adds slots 8 part .. 8 part + 7 as a tree, the stages
    ^ 8, ^ 16, ^ 32 add lanes part ^ 1, ^ 2, ^ 4 (each stage the same commutative add on both sides)"""
    p = np.stack([_tree_sum8(e[:, 8 * c:8 * c + 8]) for c in range(8)], axis=1)
    for stage in (1, 2, 4):
        p = p + p[:, np.arange(8) ^ stage]
    assert (p == p[:, :1]).all()
    return p[:, 0]


def _two_slot_sum(e16):
    """e16 (rows, 16), the live block alone -> the same for lanes that hold slots 2 part and 2 part + 1 of it"""
    p = e16[:, 0::2] + e16[:, 1::2]
    for stage in (1, 2, 4):
        p = p + p[:, np.arange(8) ^ stage]
    assert (p == p[:, :1]).all()
    return p[:, 0]


def test_two_slot_lanes_add_in_the_eight_slot_lanes_association():
    rng = np.random.default_rng(18)
    rows = 100_000
    blk = rng.integers(4, size=rows)
    # the live block: a mix of magnitudes (uniform, and 2^-u down to the threshold), so that every level of the tree rounds
    live = np.where(rng.random((rows, 16)) < 0.5, rng.uniform(0.0, 1.0, size=(rows, 16)), np.exp2(-60.0 * rng.random((rows, 16))))
    live = np.maximum(live, np.finfo(float).tiny)
    live[np.arange(rows), rng.integers(16, size=rows)] = 1.0
    live[: rows // 8, :] = np.where(rng.random((rows // 8, 16)) < 0.7, 1.0, live[: rows // 8, :])      # (sums up to 16)
    assert ((live > 0.0) & (live <= 1.0)).all() and (live.max(axis=1) == 1.0).all()
    cols = 16 * blk[:, None] + np.arange(16)[None, :]

    def placed(other):
        e = other.copy()
        np.put_along_axis(e, cols, live, axis=1)
        return e

    # the other 48 entries as the plain pass has them: at most tau = 2^-60 each, in the second half of the rows all 48 AT tau;
    # and as a certified pass has them where it loads the -inf row: 0
    below_tau = np.exp2(-60.0 - 40.0 * rng.random((rows, 64)))
    below_tau[rows // 2:] = 2.0 ** -60
    s2 = _two_slot_sum(live)
    inv2 = _newton_inverse(s2)
    w2 = live * inv2[:, None]
    assert (s2 >= 1.0).all()
    for name, e in (("values up to tau", placed(below_tau)), ("zeros", placed(np.zeros((rows, 64))))):
        s8 = _eight_slot_sum(e)
        assert np.array_equal(s8.view(np.uint64), s2.view(np.uint64)), name
        inv8 = _newton_inverse(s8)
        assert np.array_equal(inv8.view(np.uint64), inv2.view(np.uint64)), name
        w8 = np.take_along_axis(e * inv8[:, None], cols, axis=1)
        assert np.array_equal(w8.view(np.uint64), w2.view(np.uint64)), name


def proven_masks(passes):
    """the library's policy over the passes (run_policy of tests/test_estep_certificate_cpu.py, as built) -> per certified pass
    (lag behind its reference pass, the mask of proven rows)"""
    state, prev_part, out = None, None, []
    for params, order, L in passes:
        blk, part = blocks_of(order), partition(order)
        stood, prev_part = part == prev_part, part
        if state is not None and state["part"] != part:
            state = None
        if state is not None and state["age"] < RENEW:
            U, M = bounds_built(state["cert"], native(state["ref"], params)[2])
            state["age"] += 1
            out.append((state["age"], U - M <= LN_TAU - EPS))
        elif stood:
            state = dict(ref=params, part=part, cert=certificates(L, blk), age=0)
    return out


def proven_wave_share(prov):
    """share of (tile, wave) pairs whose eight rows (8 wave .. 8 wave + 7 of the tile) are all proven"""
    n = len(prov) // T * T
    return float(prov[:n].reshape(-1, 8).all(axis=1).mean())


def test_share_of_proven_waves_on_the_benchmark_model():
    """24 576 rows of the benchmark's recipe and start, 25 iterations: the share of (tile, wave) pairs with all eight rows proven,
    per lag.  The bar of one half (the project's go / no-go bar for certificates) is held on the mean over the first eleven
    certified passes, the benchmark's certified steps; the model gives 0.74."""
    masks = proven_masks(benchmark_passes())
    assert len(masks) >= 11
    shares = []
    for lag, prov in masks:
        shares.append(proven_wave_share(prov))
        n = len(prov) // T * T
        print("lag %2d  rows proven %.4f  waves with eight proven rows %.4f  tiles with 32 proven rows %.4f"
              % (lag, prov.mean(), shares[-1], prov[:n].reshape(-1, T).all(axis=1).mean()))
    mean11 = float(np.mean(shares[:11]))
    print("mean over the first eleven certified passes: %.4f" % mean11)
    assert mean11 >= 0.5
