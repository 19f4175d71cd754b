"""Every label draw of the library, held at its CDF boundaries, per component, at every magnitude from 1 down to e^-700.

The other label tests ask for "labels equal to the oracle's, bit for bit" under random or Philox uniforms: a random u lies within
1e-13 (relative) of a CDF boundary with probability 1e-13, so a cumulative sum wrong by 1e-12 — or the reduction constant the
2048-entry exponentials carried before it was the nearest double (9e-12 at |x| = 640) — changes no label there, and a component of
weight 1e-40 is never drawn at all.  Here the uniforms sit ON the boundaries (tests/cdf_ladder.py: the ladder problem in a rising
order, a flat one and flat ones with components switched off; a longdouble reference; the bound relB_k(n) from the
exponentials' contract in mimo_device.h and the float64 format, not from any kernel's output): u = F_k (1 - relB_k) must give
label k, u = F_k (1 + relB_k) label k + 1, 20 bisection launches measure where the device really switches, u = 0, u = 1 - 2^-53
and random u stay inside the bracket the bound allows, and no u > 0 ever returns a switched-off component.  Every case prints
its figures under [cdf-ladder] before it asserts.

Measured on an MI355X: the worst |u* / F_k - 1| / relB_k of the bisected switching point over the route's shapes ("rising": both
tops; the float64 oracle of the reference's own arithmetic, on the CPU, for comparison: rising 0.01 - 0.02 at K <= 16 and 0.31 -
0.46 above, flat 0.03 - 0.11).  Steps 1 and 3 passed on every route from the start: no cumulative sum, chunk base, lane prefix
or part scan is off by more than a seventh of the bound, at any rung down to e^-690.

    route                                                         rising    flat     flat-off
    small_kernel                                                  0.148     0.092    0.087
    narrow_kernel: label draw / grouped / 64 slots                0.143 / 0.148 / 0.109    0.043 / 0.081 / 0.009    0.058 / 0.087 / 0.010
    narrow_kernel: label draw + statistics                        0.146     0.055    0.065
    gibbs_rowwave_kernel (4, 14, 16 row blocks)                   0.137     0.025    0.032
    gibbs_stream_kernel                                           0.134     0.022    0.025
    mid_kernel, label draw (1, 2, 3 row blocks)                   0.146     0.068    0.063
    fused_kernel (keep_logp): normalise_tile                      0.141     0.040    0.036
    fused_kernel (keep_logp): normalise_tile_chunked<2> / <4>     0.131 / 0.116    0.020 / 0.009    0.020 / 0.010
    wide_estep_kernel (keep_logp): its own draw                   0.117     0.015    0.018
    fused_kernel, kFastGibbs (diagonal / linear structure)        0.145 / 0.131    0.068 / 0.020    0.074 / 0.020
    sample_table_kernel (sample_from_log)                         0.147     0.089    0.085
    batched kernel, label mode (rising-640 / -320, flat)          0.147     0.050    0.073
    nested batch                                                  0.140     0.029    -

What did fail, on every route but sample_from_log and the small-shape kernel with one or two lanes per row: step 4.  With the
last component switched off, u = 1 - 2^-53 returned it on 4 - 12 % of the rows (15 of the 26 flat-off cases); with a switched-off
component in the first slot of a lane, chunk, quarter or row block (flat-off-even) the bisection found it on every route, 30 -
2700 times per case.  The kernels compare u cum_K - prefix with LOCAL cumulative sums, and the prefix scans over lanes do not add
up to the last bit (incl_p of a butterfly scan is not fl(incl_{p-1} + cum_p)), so the count of sums below the threshold can stop
on a component that adds nothing.  Since then every draw hands its count to draw_label (mimo_device.h): with switched-off
components the count goes through a table to the nearest live component below.  flat-off-even has no testable boundary (ratio
0 by construction); its cases hold the bracket and step 4 on every launch.
"""
import ctypes as C

import numpy as np
import pytest

import cdf_ladder as CL

pytestmark = pytest.mark.gpu

KINDS = {1: "fused", 2: "two-stage", 3: "small", 4: "rowwave", 5: "rowwave-vi", 6: "narrow", 7: "mid"}
PLAIN_NAMES = {"small": "small_kernel", "narrow": "narrow_kernel", "rowwave": "gibbs_rowwave_kernel", "mid": "mid_kernel (labels)"}


def check(tag, res):
    print(f"\n[cdf-ladder] {tag}: worst ratio {res.ratio:.3f} ({res})", flush=True)
    assert (res.probed > 0 or "even" in tag) and res.ok(), res
    return res


def off_of(K, order):
    return CL.off_components(K, order)


def launched(engine, call):
    """The kernel names one call launches (the profile's names: one per timed launch site)."""
    engine.profile(True)
    engine.profile_read(reset=True)
    try:
        call()
        return set(engine.profile_kernels())
    finally:
        engine.profile(False)


@pytest.mark.parametrize("order", CL.ALL_ORDERS)
@pytest.mark.parametrize("name,D,K,N,needle", CL.PLAIN_SHAPES, ids=[f"{n}-d{D}-k{K}-n{N}" for n, D, K, N, _ in CL.PLAIN_SHAPES])
def test_plain_label_pass(engine, name, D, K, N, needle, order):
    """The label kernels a plain request runs on: small_kernel, narrow_kernel (plain, grouped, 64 slots; label draw + statistics in
    one pass), gibbs_rowwave_kernel (4, 14, 16 row blocks), gibbs_stream_kernel, mid_kernel's label mode (1, 2, 3 row blocks).
    The route: the family of mimo_plan on the resident data, the kernel of mimo_plan_shape's description (the resident and the
    streamed row-owner kernel share family and profile name) and the name the launch is profiled under."""
    from mimo_amd import _lib
    Z, c, b, W, L, ref = CL.case(D, K, N, order)
    engine.upload(Z)
    out, desc = (C.c_int64 * 8)(), C.create_string_buffer(256)
    assert _lib.load().mimo_plan_shape(D, K, 0, N, 1, out, desc, 256) == 0
    kind = CL.PLAIN_KIND[name]
    assert engine.plan(K, gibbs=True)["kind"] == kind == KINDS[out[0]] and needle in desc.value.decode(), (engine.plan(K, gibbs=True), desc.value)
    stats = name == "narrow-fused"                  # (the one-pass label draw + statistics exists for a request with statistics only)
    draw = lambda u: engine.gibbs_labels(c, b, W, u=u, stats=stats)[0]
    names = launched(engine, lambda: draw(np.full(N, 0.5)))
    assert PLAIN_NAMES[kind] in names and (name != "narrow-fused" or names == {"narrow_kernel"}), names
    check(f"plain {name} Dz={D} K={K} N={N} {order} [{desc.value.decode().split(' + ')[0]}]", CL.run(draw, ref, off_of(K, order)))


@pytest.mark.parametrize("order", CL.ALL_ORDERS)
@pytest.mark.parametrize("D,K,N,kernel,body", CL.TILE_SHAPES, ids=[f"d{D}-k{K}-n{N}" for D, K, N, _, _ in CL.TILE_SHAPES])
def test_tile_kernels_label_mode(engine, D, K, N, kernel, body, order):
    """gibbs_labels(..., keep_logp=True): a label pass that also keeps the log-density table leaves the plain routes for the tile
    kernels (generic mode).  Which draw each shape reaches follows from the row blocks per wave (mimo_kernels.hip: resolve_fused):
    K <= 64 one (normalise_tile, registers), 64 < K <= 128 two, K > 128 at Dz <= 9 four (normalise_tile_chunked: the chunk of the
    crossing); from Dz = 10 the shapes with K > 64 run the wide E-step kernel, whose draw is its own (mimo_wide.hip) — CL.TILE_SHAPES."""
    Z, c, b, W, L, ref = CL.case(D, K, N, order)
    engine.upload(Z)
    draw = lambda u: engine.gibbs_labels(c, b, W, u=u, stats=False, keep_logp=True)[0]
    names = launched(engine, lambda: draw(np.full(N, 0.5)))
    assert names == {kernel}, (names, body)
    on = np.isfinite(L)
    assert np.array_equal(engine.get_logp(K)[on], L[on]), "the route rounds the logits"
    check(f"tile Dz={D} K={K} N={N} {order} [{kernel}: {body}]", CL.run(draw, ref, off_of(K, order)))


@pytest.mark.parametrize("order", CL.ALL_ORDERS)
@pytest.mark.parametrize("structure,D,K,N,body", CL.STRUCT_SHAPES, ids=[f"{s}-d{D}-k{K}-n{N}" for s, D, K, N, _ in CL.STRUCT_SHAPES])
def test_tile_kernels_fast_label_mode(engine, structure, D, K, N, body, order):
    """fused_kernel<..., kFastGibbs>: no label request of the full structure reaches it (the narrow, mid, small and row-owner
    kernels take them all: ROUTING.md); under the diagonal and the linear structure hint some shapes do.  W_k = I is diagonal and
    tied, so the ladder problem is the same problem there (the linear map drops z' W z / 2, a constant of the row)."""
    Z, c, b, W, L, ref = CL.case(D, K, N, order)
    try:
        engine.set_structure(structure)
        engine.upload(Z)
        assert engine.plan(K, gibbs=True)["kind"] == "fused", engine.plan(K, gibbs=True)
        draw = lambda u: engine.gibbs_labels(c, b, W, u=u, stats=True)[0]
        names = launched(engine, lambda: draw(np.full(N, 0.5)))
        assert names == {"fused_kernel"}, names
        check(f"structure {structure} Dz={D} K={K} N={N} {order} [fused_kernel: {body}]", CL.run(draw, ref, off_of(K, order)))
    finally:
        engine.set_structure("full")


@pytest.mark.parametrize("order", CL.ALL_ORDERS)
@pytest.mark.parametrize("D,K,N", CL.TABLE_SHAPES, ids=[f"k{K}-n{N}" for _, K, N in CL.TABLE_SHAPES])
def test_sample_from_log(engine, D, K, N, order):
    """sample_table_kernel on a host table of log-probabilities (the ladder's exact logits; -inf where switched off)."""
    Z, c, b, W, L, ref = CL.case(D, K, N, order)
    check(f"sample_from_log K={K} N={N} {order}", CL.run(lambda u: engine.sample_from_log(logp=L, u=u), ref, off_of(K, order)))


@pytest.fixture(scope="module")
def batched_engine():
    from mimo_amd.batched import BatchedHipEngine
    eng = BatchedHipEngine(0)
    yield eng
    eng.close()


def batch_procedure(eng, tag, cases, orders, K):
    """The procedure on one problem of the batch at a time, all problems in every launch (the others at u = 1 / 2)."""
    c, b, W = (np.stack([cs[i] for cs in cases]) for i in (1, 2, 3))
    rows = [cs[0].shape[0] for cs in cases]
    for i, (cs, order) in enumerate(zip(cases, orders)):
        def draw(u, i=i):
            us = [np.full(n, 0.5) for n in rows]
            us[i] = u
            return eng.gibbs_labels(c, b, W, u=us, stats=False)[0][i]
        check(f"{tag} problem {i} N={rows[i]} {order}", CL.run(draw, cs[5], off_of(K, order)))


@pytest.mark.parametrize("D,K", CL.BATCHED_SHAPES, ids=[f"d{D}-k{K}" for D, K in CL.BATCHED_SHAPES])
def test_batched_label_pass(batched_engine, D, K):
    """Three problems (257, 3 and 515 rows; rising-640, flat, rising-320) in one launch of the batched kernel's label mode (the
    draws of mimo_tile.h, one row block per wave at K <= 64)."""
    cases = [CL.case(D, K, N, order) for N, order in zip(CL.BATCHED_ROWS, CL.BATCHED_ORDERS)]
    batched_engine.upload([cs[0] for cs in cases])
    batch_procedure(batched_engine, f"batched Dz={D} K={K}", cases, CL.BATCHED_ORDERS, K)


@pytest.mark.parametrize("D,K", CL.BATCHED_SHAPES, ids=[f"d{D}-k{K}" for D, K in CL.BATCHED_SHAPES])
def test_batched_label_pass_switched_off(batched_engine, D, K):
    """The same launch with switched-off components in two of the three problems (flat-off, flat, flat-off-even): every problem
    has its own set, and the one between them none."""
    cases = [CL.case(D, K, N, order) for N, order in zip(CL.BATCHED_ROWS, CL.BATCHED_OFF_ORDERS)]
    batched_engine.upload([cs[0] for cs in cases])
    batch_procedure(batched_engine, f"batched Dz={D} K={K}", cases, CL.BATCHED_OFF_ORDERS, K)


def test_nested_label_pass(batched_engine):
    """A nested batch: ONE data set, three inner problems (rising-640, flat, rising-320) reading it; host uniforms per problem."""
    D, K = CL.NESTED_SHAPE
    cases = [CL.case(D, K, CL.NESTED_ROWS, order) for order in CL.BATCHED_ORDERS]
    assert all(np.array_equal(cs[0], cases[0][0]) for cs in cases)
    batched_engine.upload_shared(cases[0][0], len(cases))
    batch_procedure(batched_engine, f"nested Dz={D} K={K}", cases, CL.BATCHED_ORDERS, K)
