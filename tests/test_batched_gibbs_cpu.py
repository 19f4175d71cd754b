"""CPU: the batched Gibbs label pass without a GPU — loud failures of the new entry points on a null context, and the
argument validation of BatchedHipEngine.gibbs_labels / label_stats and of resample_batched that happens before any library
call.  (The label modes live in mimo_batched.hip, whose ISA tests/test_batched_cpu.py already checks for barriers.)"""
import numpy as np
import numpy.random as npr
import pytest

from conftest import load_golden
import model_checks as mc
from oracle_engine import OracleEngine
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.mixtures.batched import resample_batched


def test_batched_gibbs_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _lib.load()
    seeds = np.array([1], dtype=np.uint64)
    assert lib.mimo_gibbs_labels_batched(None, None, None, None, 1, seeds.ctypes.data, 0, None, 0, None, None) == _lib.E_INVALID
    assert lib.mimo_label_stats_batched(None, None, 1, 0, None) == _lib.E_INVALID


def _offline(rows, D):
    """An engine object without a context: only the host-side validation runs."""
    eng = object.__new__(BatchedHipEngine)
    eng._ctx, eng.B, eng.D = None, len(rows), D
    eng.row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return eng


def test_batched_gibbs_argument_validation():
    eng = _offline([5, 3], 2)
    K = 4
    c, b, W = np.zeros((2, K)), np.zeros((2, K, 2)), np.zeros((2, K, 2, 2))
    bad = [dict(),                                            # neither uniforms nor seeds
           dict(seeds=[1]), dict(seeds=[1, 2, 3]),            # one seed per problem
           dict(u=[np.zeros(5)]),                             # one uniform array per problem
           dict(u=[np.zeros(5), np.zeros(4)]), dict(u=[np.zeros((1, 4)), np.zeros(3)])]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.gibbs_labels(c, b, W, **kw)
    with pytest.raises(ValueError):
        eng.gibbs_labels(c[:1], b, W, seeds=[1, 2])
    for labels in ([np.zeros(5, np.int32)], [np.zeros(5, np.int32), np.zeros(4, np.int32)],
                   [np.zeros(5, np.int32), np.array([0, 4, 1])], [np.array([0, 0, -1, 0, 0]), np.zeros(3, np.int32)]):
        with pytest.raises(ValueError):
            eng.label_stats(labels, K)


def test_resample_batched_argument_validation():
    g = load_golden("gibbs_c1_trace")
    engine = OracleEngine()
    models = [mc.build_gmm(g, engine)[1] for _ in range(2)]
    data = [g["X"], g["X"][:100]]
    ilr = mc.build_ilr(load_golden("ilr_svi_dx2_dy1_k8"), engine)[1]
    state = npr.get_state()
    for kw in (dict(init_labels='kmeans'), dict(label_rng='torch'), dict(seeds=[1]), dict(param_rngs=[None] * 3),
               dict(numpy_seeds=[1, 2, 3]), dict(maxiter=-1)):
        with pytest.raises(ValueError):
            resample_batched(models, data, **kw)
    with pytest.raises(ValueError):
        resample_batched(models, data[:1])
    with pytest.raises(ValueError):
        resample_batched([models[0], ilr], [data[0], data[1]])
    after = npr.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]      # nothing was drawn
