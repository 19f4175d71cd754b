"""CPU: the batched table passes (mimo_weighted_stats_batched / mimo_random_resp_stats_batched) without a GPU — loud
failures of the new entry points on a null context, and the argument validation of BatchedHipEngine.weighted_stats /
random_resp_stats and of meanfield_coordinate_descent_batched that happens before any library call.  (The table mode and
the fill kernel live in mimo_batched.hip, whose ISA tests/test_batched_cpu.py already checks for barriers.)"""
import numpy as np
import numpy.random as npr
import pytest

from conftest import load_golden
import model_checks as mc
from oracle_engine import OracleEngine
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.mixtures.batched import meanfield_coordinate_descent_batched


def test_batched_table_entry_points_fail_loudly_on_a_null_context():
    lib = _lib.load()
    seeds = np.array([1], dtype=np.uint64)
    resp = np.ones((1, 2))
    S = np.empty((1, 7))
    assert lib.mimo_weighted_stats_batched(None, resp.ctypes.data, 1, 0, S.ctypes.data) == _lib.E_INVALID
    assert lib.mimo_weighted_stats_batched(None, None, 1, 0, None) == _lib.E_INVALID
    assert lib.mimo_random_resp_stats_batched(None, 1, seeds.ctypes.data, 0, S.ctypes.data) == _lib.E_INVALID
    assert lib.mimo_random_resp_stats_batched(None, 1, None, 0, None) == _lib.E_INVALID


def _offline(rows, D):
    """An engine object without a context or a library: only the host-side validation runs."""
    eng = object.__new__(BatchedHipEngine)
    eng._ctx, eng.B, eng.D = None, len(rows), D
    eng.row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return eng


def test_batched_tables_argument_validation():
    eng = _offline([5, 3], 2)
    K = 4
    bad = [[np.zeros((K, 5))],                                          # one table per problem
           [np.zeros((K, 5)), np.zeros((K, 3)), np.zeros((K, 3))],
           [np.zeros((K, 5)), np.zeros(3)],                             # ndim != 2
           [np.zeros((K, 5, 1)), np.zeros((K, 3))],
           [np.zeros((K, 5)), np.zeros((K + 1, 3))],                    # one K for all problems
           [np.zeros((K, 5)), np.zeros((K, 4))],                        # N_b against row_off
           [np.zeros((K, 3)), np.zeros((K, 5))],
           [np.zeros((5, K)), np.zeros((3, K))]]                        # (N_b, K): transposed
    for tables in bad:
        with pytest.raises(ValueError):
            eng.weighted_stats(tables)
    with pytest.raises(ValueError):
        eng.weighted_stats(None)                                        # the resident table's K must be given
    for seeds in ([1], [1, 2, 3], []):
        with pytest.raises(ValueError):
            eng.random_resp_stats(K, seeds)
    # well-formed arguments pass the validation (and then need the library: the offline object has none)
    with pytest.raises(AttributeError):
        eng.weighted_stats([np.zeros((K, 5)), np.zeros((K, 3))])
    with pytest.raises(AttributeError):
        eng.random_resp_stats(K, [1, 2])


def test_batched_driver_argument_validation_unchanged():
    g = load_golden("gibbs_c1_trace")
    engine = OracleEngine()
    models = [mc.build_gmm(g, engine)[1] for _ in range(2)]
    data = [g["X"], g["X"][:100]]
    ilr = mc.build_ilr(load_golden("ilr_svi_dx2_dy1_k8"), engine)[1]
    state = npr.get_state()
    with pytest.raises(ValueError):
        meanfield_coordinate_descent_batched(models, data, seeds=[1])
    with pytest.raises(ValueError):
        meanfield_coordinate_descent_batched(models, data, seeds=[1, 2, 3])
    with pytest.raises(ValueError):
        meanfield_coordinate_descent_batched(models, data[:1])
    with pytest.raises(ValueError):
        meanfield_coordinate_descent_batched([], [])
    with pytest.raises(ValueError):
        meanfield_coordinate_descent_batched([models[0], ilr], [data[0], data[1]])
    after = npr.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]      # nothing was drawn
