"""A parameter block the library refuses — NaN or +inf in c, NaN or infinity in b or W, a W that breaks the structure hint —
on one shape per Theta image: the error code and the text of mimo_last_error are part of the ABI (the strings below are those
of the entry points, written out here and not read from the library), and a refused block leaves no state behind: the valid
call right after it returns the bits a fresh engine returns."""
import ctypes as C

import numpy as np
import pytest

from mimo_amd import _lib
from mimo_amd.engine import _ptr

pytestmark = pytest.mark.gpu

N = 4096
KINDS = {1: "fused", 2: "two-stage", 3: "small", 4: "rowwave", 5: "rowwave-vi", 6: "narrow", 7: "mid"}
# (image, Dz, K, label pass, family of mimo_plan, what mimo_plan_shape's description must name)
SHAPES = [
    ("small", 2, 4, False, "small", "small_kernel"),
    ("narrow", 2, 50, False, "narrow", "narrow_kernel"),
    ("narrow grouped", 16, 4, False, "narrow", "grouped"),
    ("mid", 20, 16, False, "mid", "mid_kernel"),
    ("mid labels", 20, 16, True, "mid", "label draw"),
    ("row-owner", 8, 64, True, "rowwave", "gibbs_rowwave_kernel"),
    ("generic, fused", 16, 64, False, "fused", "fused_kernel"),
    ("generic, two-stage", 32, 128, False, "two-stage", "wide_estep_kernel"),
]


def _model(rng, K, D, lead=()):
    A = rng.standard_normal(lead + (K, D, D))
    W = A @ np.swapaxes(A, -1, -2) / D + 0.3 * np.eye(D)
    return rng.standard_normal(lead + (K,)), rng.standard_normal(lead + (K, D)), np.ascontiguousarray(W)


def _refused(lib, ctx, call, text):
    rc = call()
    assert rc == _lib.E_INVALID, (rc, lib.mimo_last_error(ctx).decode())
    assert lib.mimo_last_error(ctx).decode() == text


@pytest.mark.parametrize("image,D,K,gibbs,kind,names", SHAPES, ids=[s[0] for s in SHAPES])
def test_refused_parameters_single(image, D, K, gibbs, kind, names):
    from mimo_amd.engine import HipEngine
    rng = np.random.default_rng(100 * D + K)
    Z = rng.standard_normal((N, D)) * 1.5
    c, b, W = _model(rng, K, D)
    eng, fresh = HipEngine(0), HipEngine(0)
    lib, ctx = eng._lib, eng._ctx
    eng.upload(Z)
    assert eng.plan(K, gibbs=gibbs)["kind"] == kind
    out, desc = (C.c_int64 * 8)(), C.create_string_buffer(256)
    assert lib.mimo_plan_shape(D, K, 0, N, 1 if gibbs else 0, out, desc, 256) == 0
    assert KINDS[out[0]] == kind and names in desc.value.decode(), desc.value.decode()

    S, sc, labels = np.empty((K, 1 + D + D * D)), np.empty(3), np.empty(N, dtype=np.int32)

    def call(c_, b_, W_):
        c_, b_, W_ = (np.ascontiguousarray(x) for x in (c_, b_, W_))
        if gibbs:
            return lambda: lib.mimo_gibbs_labels(ctx, _ptr(c_), _ptr(b_), _ptr(W_), K, 5, 1, None, 0, _ptr(labels), _ptr(S))
        return lambda: lib.mimo_estep(ctx, _ptr(c_), _ptr(b_), _ptr(W_), K, 0, _ptr(S), _ptr(sc))

    def spoiled(x, idx, v):
        y = x.copy()
        y[idx] = v
        return y

    _refused(lib, ctx, call(spoiled(c, 1, np.nan), b, W), "c[1] is NaN or +inf")
    _refused(lib, ctx, call(spoiled(c, 1, np.inf), b, W), "c[1] is NaN or +inf")
    _refused(lib, ctx, call(c, spoiled(b, (2, 1), np.nan), W), "b or W holds a NaN or an infinity")
    _refused(lib, ctx, call(c, b, spoiled(W, (2, 0, 1), np.inf)), "b or W holds a NaN or an infinity")
    # the two structure rules: under a reduced map the shape takes whatever route serves that map, which for the mid and the grouped
    # narrow rows is NOT the image the row is named after (both exist for the full structure only) — what is checked there is that
    # the one enumerator words the refusal the same on every route; the images themselves are read back in theta_image_check.cpp
    tied = np.ascontiguousarray(np.broadcast_to(W[0], W.shape))
    eng.set_structure('linear')
    _refused(lib, ctx, call(c, b, spoiled(tied, (2, 1, 1), 7.0)),
             "linear structure is set (mimo_set_structure) but W[2] differs from W[0]")
    eng.set_structure('diag')
    Wd = W * np.eye(D)
    _refused(lib, ctx, call(c, b, spoiled(Wd, (1, 0, D - 1), 0.5)),
             f"diagonal structure is set (mimo_set_structure) but W[1] has the off-diagonal entry (0,{D - 1})")
    eng.set_structure('full')

    fresh.upload(Z)
    if gibbs:
        got, want = eng.gibbs_labels(c, b, W, seed=5, sweep=1), fresh.gibbs_labels(c, b, W, seed=5, sweep=1)
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(got[1].packed(), want[1].packed())
    else:
        got, want = eng.estep(c, b, W), fresh.estep(c, b, W)
        assert np.array_equal(got[0].packed(), want[0].packed())
        assert np.array_equal(got[1], want[1], equal_nan=True)
    eng.close()
    fresh.close()


def test_refused_parameters_batched():
    """The batched passes lead the text with their own name and index a component as [problem][k]."""
    from mimo_amd.batched import BatchedHipEngine
    B, D, K = 2, 4, 8
    rng = np.random.default_rng(7)
    Zs = [rng.standard_normal((N // B, D)) * 1.5 for _ in range(B)]
    c, b, W = _model(rng, K, D, (B,))
    eng, fresh = BatchedHipEngine(0), BatchedHipEngine(0)
    lib, ctx = eng._lib, eng._ctx
    eng.upload(Zs)
    S, sc = np.empty((B, K, 1 + D + D * D)), np.empty((B, 3))
    labels, seeds = np.empty(N, dtype=np.int32), np.array([11, 12], dtype=np.uint64)

    def calls(c_, b_, W_):
        return (("mimo_estep_batched", lambda: lib.mimo_estep_batched(ctx, _ptr(c_), _ptr(b_), _ptr(W_), K, 0, _ptr(S), _ptr(sc))),
                ("mimo_gibbs_labels_batched", lambda: lib.mimo_gibbs_labels_batched(ctx, _ptr(c_), _ptr(b_), _ptr(W_), K, _ptr(seeds), 1, None,
                                                                                     0, _ptr(labels), _ptr(S))))

    for v in (np.nan, np.inf):
        bad = c.copy()
        bad[1, 2] = v
        for what, call in calls(bad, b, W):
            _refused(lib, ctx, call, f"{what}: c[1][2] is NaN or +inf")
    bad = b.copy()
    bad[1, 3, 0] = np.nan
    for what, call in calls(c, bad, W):
        _refused(lib, ctx, call, f"{what}: b or W of problem 1 holds a NaN or an infinity")
    bad = W.copy()
    bad[0, 5, 1, 2] = -np.inf
    for what, call in calls(c, b, bad):
        _refused(lib, ctx, call, f"{what}: b or W of problem 0 holds a NaN or an infinity")

    fresh.upload(Zs)
    got, want = eng.estep(c, b, W), fresh.estep(c, b, W)
    assert all(np.array_equal(g.packed(), w.packed()) for g, w in zip(got[0], want[0]))
    assert np.array_equal(got[1], want[1], equal_nan=True)
    got, want = eng.gibbs_labels(c, b, W, seeds=seeds, sweep=1), fresh.gibbs_labels(c, b, W, seeds=seeds, sweep=1)
    assert all(np.array_equal(g, w) for g, w in zip(got[0], want[0]))
    assert all(np.array_equal(g.packed(), w.packed()) for g, w in zip(got[1], want[1]))
    eng.close()
    fresh.close()
