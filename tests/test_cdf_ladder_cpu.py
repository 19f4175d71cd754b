"""The CDF-boundary procedure of the GPU label-draw tests (tests/cdf_ladder.py), checked without a GPU: its longdouble reference agrees
with 50-digit values (tests/golden/cdf_ladder_hp.npz, make_cdf_ladder_golden.py), every boundary the issue of the draw's accuracy
asks for is testable, the shape list reaches every label kernel through the library's own router, the float64 oracle passes the
procedure with room, and two planted defects — the old reduction constant of the 2048-entry exponentials, a chunk prefix short by
one component — fail it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
import cdf_ladder as CL
import softmax_ladder as SL
from oracle import mimo_oracle as O

sys.path.insert(0, os.path.join(ROOT, "tools"))
LD = np.longdouble
# every problem the GPU file builds: (Dz, K, N, order)
SHAPES = sorted({(D, K, N) for _, D, K, N, _ in CL.PLAIN_SHAPES} | {(D, K, N) for D, K, N, _, _ in CL.TILE_SHAPES}
                | {(D, K, N) for _, D, K, N, _ in CL.STRUCT_SHAPES} | set(CL.TABLE_SHAPES))
PROBLEMS = ([(D, K, N, order) for D, K, N in SHAPES for order in CL.ALL_ORDERS]
            + [(D, K, N, order) for D, K in CL.BATCHED_SHAPES for orders in (CL.BATCHED_ORDERS, CL.BATCHED_OFF_ORDERS)
               for N, order in zip(CL.BATCHED_ROWS, orders)]
            + [CL.NESTED_SHAPE + (CL.NESTED_ROWS, order) for order in CL.BATCHED_ORDERS])
PROBLEMS = list(dict.fromkeys(PROBLEMS))
IDS = [f"d{D}-k{K}-n{N}-{order}" for D, K, N, order in PROBLEMS]


def test_problems_are_exact_permutations_of_the_ladder():
    """rising: component K - 1 is every row's maximum and x_kn = -a_{K-1-k} - s_{K-1-k} Z[n, 0]; flat: x in [-3, 0]; flat-off:
    the same with components {0, 5, K - 1} at -inf.  (The logits' exactness is the ladder's: test_softmax_ladder_cpu.py.)"""
    D, K, N = 3, 32, 515
    for top in (640, 700):
        Z, c, b, W, L, ref = CL.case(D, K, N, f"rising-{top}")
        a, s = SL.ladder(K, top)
        assert np.array_equal(L.argmax(axis=0), np.full(N, K - 1))
        assert np.array_equal(L - L[K - 1], -a[::-1, None] - s[::-1, None] * Z[None, :, 0])
        assert np.array_equal(L[::-1], SL.case(D, K, N, top)[4])
    Z, c, b, W, L, ref = CL.case(D, K, N, "flat")
    assert float(ref.x.min()) >= -3.0 and np.array_equal(L - L[0], -(np.arange(K) % 4)[:, None] * Z[None, :, 0])
    Lo = CL.case(D, K, N, "flat-off")[4]
    off = list(CL.off_components(K))
    assert np.all(Lo[off] == -np.inf) and np.array_equal(np.delete(Lo, off, axis=0), np.delete(L, off, axis=0))


@pytest.mark.parametrize("order", CL.ORDERS)
def test_longdouble_reference_against_50_digits(order):
    """F and relB of one small problem per order agree with mpmath at 50 digits to 2^-58, relatively; a boundary below a
    switched-off component 0 is exactly 0 in both."""
    g = load_golden("cdf_ladder_hp")
    D, K, N, seed = (int(v) for v in g["shape"])
    ref = CL.case(D, K, N, order, seed)[5]
    tag = order.replace("-", "_")
    hp = lambda name: g[f"{tag}_{name}_hi"].astype(LD) + g[f"{tag}_{name}_lo"].astype(LD)
    tol = LD(2.0) ** -58
    for name, got, want in (("F", ref.F, hp("F") / LD(2.0) ** int(g["scale_log2"])), ("relB", ref.relB, hp("relB"))):
        assert want.shape == got.shape
        assert np.array_equal(want == 0, got == 0)
        nz = want > 0
        worst = float((np.abs(got[nz] - want[nz]) / want[nz]).max())
        print(f"{order} {name}: worst relative difference 2^{np.log2(max(worst, 1e-30)):.1f}")
        assert worst <= tol, name


@pytest.mark.parametrize("D,K,N,order", PROBLEMS, ids=IDS)
def test_coverage_conditions(D, K, N, order):
    """rising-640 (and the batched rising-320) and flat leave out nothing; rising-700 only the rungs below 1e-300; flat-off exactly
    the boundaries that touch a switched-off component."""
    ref = CL.case(D, K, N, order)[5]
    t = ref.testable
    assert t.shape == (K - 1, N)
    if order == "rising-700":
        small = np.asarray(ref.F[:-1] <= LD(1e-300))
        assert np.array_equal(~t, small), "something but the rungs below 1e-300 is left out"
        lost = int((~t).any(axis=1).sum())
        print(f"rising-700 K={K}: {lost} of {K - 1} boundaries lose rows, share {t.mean():.3f}")
        # (a_k + 3 >= 690.8 at a spacing of 700 / (K - 1): one boundary of seven at K = 8, four whole ones and part of a fifth at K = 256)
        assert 1 <= lost <= 5 and t[lost:].all() and t.mean() >= 6.0 / 7.0 - 1e-12, "more than the lowest rungs lose rows"
    elif order.startswith("flat-off"):
        touched = np.zeros(K - 1, dtype=bool)
        for j in CL.off_components(K, order):
            touched[[k for k in (j - 1, j) if 0 <= k < K - 1]] = True
        assert np.array_equal(t, np.broadcast_to(~touched[:, None], t.shape))
    else:
        assert t.all()
    # both shifts together probe every boundary that has a testable row at all, if the rows are at least as many as the boundaries
    if N >= K - 1:
        rows = np.arange(N)
        seen = np.zeros(K - 1, dtype=bool)
        for sh in CL.shifts(K):
            k = (rows + sh) % (K - 1)
            seen[k[t[k, rows]]] = True
        assert np.array_equal(seen, t.any(axis=1))


def route(lib, D, K, N):
    out, desc = (C.c_int64 * 8)(), C.create_string_buffer(256)
    assert lib.mimo_plan_shape(D, K, 0, N, 1, out, desc, 256) == 0
    kinds = {1: "fused", 2: "two-stage", 3: "small", 4: "rowwave", 5: "rowwave-vi", 6: "narrow", 7: "mid"}
    return kinds[out[0]], desc.value.decode()


def test_shape_list_reaches_every_label_kernel():
    """Through the library's own host-only router, at the row counts of the tests: the plain label request of every shape runs on
    the kernel its entry names, and the list covers the small kernel, the narrow kernel's plain, grouped, 64-slot and fused label
    modes, the resident and the streamed row-owner kernel and the mid kernel's label mode with one, two and three row blocks."""
    from mimo_amd import _lib
    lib = _lib.load()
    for name, D, K, N, needle in CL.PLAIN_SHAPES:
        kind, desc = route(lib, D, K, N)
        assert kind == CL.PLAIN_KIND[name] and needle in desc, (name, D, K, N, kind, desc)
    assert {n for n, *_ in CL.PLAIN_SHAPES} == set(CL.PLAIN_KIND)
    blocks = {desc.split("<")[1].split(" row")[0] for n, D, K, N, _ in CL.PLAIN_SHAPES if n == "rowwave" for desc in [route(lib, D, K, N)[1]]}
    assert blocks == {"4", "14", "16"}
    # the tile, table, batched and nested cases leave the plain request; their kernels are asserted on the device.  No plain
    # label request of the full structure is served by the single-pass tile kernel (ROUTING.md), which is why its fast label mode
    # (fused_kernel<..., kFastGibbs>) is probed under the diagonal and the linear structure: STRUCT_SHAPES
    for structure, D, K, N, _ in CL.STRUCT_SHAPES:
        out = (C.c_int64 * 8)()
        assert lib.mimo_plan_shape(D, K, {"diag": 1, "linear": 2}[structure], N, 1, out, None, 0) == 0 and out[0] == 1
        assert lib.mimo_plan_shape(D, K, 0, N, 1, out, None, 0) == 0 and out[0] != 1
    import routing_table as rt
    assert all(rt.route(lib, D, K, True)[0] != "fused" for D in rt.DS for K in rt.KS)


@pytest.mark.parametrize("D,K,N,order", PROBLEMS, ids=IDS)
def test_float64_oracle_passes_with_room(D, K, N, order):
    """The float64 oracle (sample_discrete_from_log: the reference's own arithmetic, normalised probabilities) in place of the
    device passes steps 1, 3 and 4 and switches within the bound.  It rounds p_log - lognorm at |x| up to 700, which the device
    (unnormalised sums) does not have to: its ratio is an upper mark, not the device's."""
    Z, c, b, W, L, ref = CL.case(D, K, N, order)
    off = CL.off_components(K, order)
    with np.errstate(invalid="ignore", divide="ignore"):
        res = CL.run(lambda u: O.sample_discrete_from_log(L, u), ref, off)
    print(f"\n[cdf-ladder] float64 oracle Dz={D} K={K} N={N} {order}: {res}")
    assert (res.probed > 0 or order == "flat-off-even") and res.ok(), res


@pytest.mark.parametrize("D,K,N,order", [p for p in PROBLEMS if p[3].startswith("rising")],
                         ids=[i for p, i in zip(PROBLEMS, IDS) if p[3].startswith("rising")])
def test_old_reduction_constant_fails(D, K, N, order):
    """Bounds are not slack: the float64 draw with every exponential times (1 + 1.41e-14 |x|) misses step 1 on every rising problem
    (at the top rungs 9e-12 against relB ~ 1.5e-13: some 60 bounds), and the same draw without the defect passes."""
    Z, c, b, W, L, ref = CL.case(D, K, N, order)
    assert CL.run(CL.float64_draw(L), ref).ok()
    res = CL.run(CL.float64_draw(L, "ln2"), ref)
    print(f"\n[cdf-ladder] ln2 / 2048 defect Dz={D} K={K} N={N} {order}: {res}")
    assert res.step1 > 0, res


@pytest.mark.parametrize("D,K,N", SHAPES, ids=[f"d{D}-k{K}-n{N}" for D, K, N in SHAPES])
def test_short_chunk_prefix_fails(D, K, N):
    """A chunk prefix that misses one flat component (every cumulative sum from component 4 on short by e_1) misses step 1."""
    Z, c, b, W, L, ref = CL.case(D, K, N, "flat")
    assert CL.run(CL.float64_draw(L), ref).ok()
    res = CL.run(CL.float64_draw(L, "prefix"), ref)
    assert res.step1 > 0, res
