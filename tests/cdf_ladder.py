"""The label draw held at its CDF boundaries: the uniforms of an inverse-CDF draw placed exactly where the draw can go wrong, on the
ladder problem of tests/softmax_ladder.py (exact dyadic logits), with a longdouble reference and a PER-BOUNDARY bound.  Imported by
tests/test_cdf_ladder_cpu.py (no GPU) and tests/test_gpu_cdf_accuracy.py.

The rule every draw of the library implements (mimo/utils/stats.py:8-21 of the reference):   label_n = #{k : u_n cum_K > cum_k},
cum_k = sum_{j <= k} exp(L_jn - max_n), strict inequality.  With F_k = cum_k / cum_{K-1} the label switches from k to k + 1 where
u crosses F_k: boundary k of row n.

Problems (one ladder, four orders; `c` and `b` permuted together, W_k = I):
    rising-<top>   component order reversed: component K - 1 is every row's maximum, x_kn = -a_{K-1-k} - s_{K-1-k} Z[n, 0], the
                   cumulative sums grow from e^-top to 1 and boundary k lives at magnitude F_k ~ e^{-a}: the comparison is relative
                   at every rung, so the exponential's error at every |x| decides a label
    flat           top = 0: every x in [-3, 0], all weights comparable, boundaries spread over (0, 1): every chunk base, lane prefix
                   and part scan takes part at full magnitude
    flat-off       flat with c_k = -inf for k in {0, 5, K - 1}: weight exactly 0, cum_k == cum_{k-1}: no u > 0 may draw them
    flat-off-even  flat with c_k = -inf for every even k and for K - 1: a switched-off component opens every lane's, chunk's, quarter's
                   and row block's run of slots, whatever the kernel's layout — where the local cumulative sums restart and the
                   prefix in front of them is another scan's.  (Every boundary touches a switched-off component: none is testable,
                   all are probed.)

Bound (u0 = 2^-53; term(j, n) = u0 (2 |x_jn| + 8) as in softmax_ladder.py: the exponentials' contract of mimo_device.h, doubled):
    relB_k(n) = sum_{j<=k} e_j term(j, n) / cum_k  +  sum_j r_jn term(j, n)  +  u0 (2 K + 12)
                (the error of cum_k)               (the error of cum_K)        (two summation chains, the product u cum_K, the
                                                                                prefix subtractions)
A correct draw compares correctly whenever |u / F_k - 1| > relB_k(n).  It comes from the contract and the float64 format, never
from a kernel's output.

Boundary k < K - 1 of row n is testable when its neighbours are far enough and it is a normal number:
    F_k - F_{k-1} > 8 relB_k F_k,   F_{k+1} - F_k > 8 relB_k F_k,   F_k (1 + 2 relB_k) < 1,   F_k > 1e-300.

Procedure (run()): row n probes boundary k = (n + shift) mod (K - 1), two shifts; `draw(u) -> labels` is the thing under test.
    1. u_lo = float64(F_k (1 - relB_k)) must give k, u_hi = float64(F_k (1 + relB_k)) must give k + 1, on every testable row
    2. 20 bisection launches between the two, all rows at once: where the draw switches, as |u* / F_k - 1| / relB_k
    3. u = 0 gives 0 everywhere; u = 1 - 2^-53 and random u (even rows: multiples of 1 / 1000, odd rows: log-uniform down to
       1e-290, so that light components are met too) give  #{k : u > F_k (1 + relB_k)} <= label <= #{k : u > F_k (1 - relB_k)}
       (k over 0 .. K - 2: u < 1 never exceeds cum_K)
    4. no launch with u > 0 returns a switched-off component
A boundary that is not testable is probed like the others wherever it is a normal number (steps 1 and 2 do not judge its rows), and
EVERY launch of steps 1 to 3 is held to the bracket of step 3 and to step 4."""
import functools

import numpy as np

import softmax_ladder as SL

U = SL.U
LD = SL.LD
ORDERS = ("rising-640", "rising-700", "flat", "flat-off")
ALL_ORDERS = ORDERS + ("flat-off-even",)
BISECTIONS = 20

# (route, Dz, K, N, what mimo_plan_shape's description of the label pass must name): the plain label request at these N
PLAIN_SHAPES = [
    ("small", 2, 8, 257, "small_kernel"), ("small", 4, 8, 515, "small_kernel"),
    ("narrow", 3, 32, 515, "label draw>"), ("narrow-grouped", 16, 8, 515, "grouped, label draw>"), ("narrow-64-slots", 3, 256, 257, "narrow_kernel<64 slots"),
    ("narrow-fused", 5, 16, 257, "label draw + statistics>"),
    ("rowwave", 8, 64, 257, "gibbs_rowwave_kernel<4 row blocks>"), ("rowwave", 4, 200, 515, "gibbs_rowwave_kernel<14 row blocks>"),
    ("rowwave", 8, 256, 515, "gibbs_rowwave_kernel<16 row blocks>"),
    ("stream", 13, 80, 515, "gibbs_stream_kernel"), ("stream", 32, 128, 257, "gibbs_stream_kernel"), ("stream", 12, 200, 515, "gibbs_stream_kernel"),
    ("mid", 14, 40, 515, "mid_kernel<Dz=14, row blocks 3, label draw>"), ("mid", 20, 24, 257, "mid_kernel<Dz=20, row blocks 2, label draw>"),
    ("mid", 24, 12, 257, "mid_kernel<Dz=24, row blocks 1, label draw>"),
]
PLAIN_KIND = {"small": "small", "narrow": "narrow", "narrow-grouped": "narrow", "narrow-64-slots": "narrow", "narrow-fused": "narrow",
              "rowwave": "rowwave", "stream": "rowwave", "mid": "mid"}
# gibbs_labels(..., keep_logp=True) leaves the plain routes for the tile kernels: (Dz, K, N, the profiled kernel, the draw it reaches)
TILE_SHAPES = [
    (8, 40, 515, "fused_kernel", "normalise_tile (one row block per wave, 6 of 8 slots per lane, 64-entry exponential)"),
    (16, 64, 515, "fused_kernel", "normalise_tile (full lanes, the 2048-entry exponential of Dz >= 14)"),
    (8, 100, 515, "fused_kernel", "normalise_tile_chunked<2> (two chunks per lane, 14 of 16 slots)"),
    (8, 200, 257, "fused_kernel", "normalise_tile_chunked<4> (four chunks per lane, 26 of 32 slots)"),
    (12, 200, 515, "wide_estep_kernel", "the wide E-step's own draw (mimo_wide.hip), not mimo_tile.h"),
]
# a plain label request reaches the tile kernels' fast label mode (fused_kernel<..., kFastGibbs>) only under a structure hint:
# (structure, Dz, K, N, the draw it reaches)
STRUCT_SHAPES = [
    ("diag", 20, 16, 515, "normalise_tile (kFastGibbs, split over the waves, 2 of 8 slots per lane)"),
    ("linear", 32, 100, 257, "normalise_tile_chunked<2> (kFastGibbs, 14 of 16 slots per lane)"),
]
TABLE_SHAPES = [(2, 8, 257), (2, 64, 257), (2, 256, 257)]          # sample_from_log on a host table (Dz only shapes the problem)
BATCHED_SHAPES = SL.BATCHED_SHAPES
BATCHED_ROWS, BATCHED_ORDERS = (257, 3, 515), ("rising-640", "flat", "rising-320")
BATCHED_OFF_ORDERS = ("flat-off", "flat", "flat-off-even")          # a second batch: switched-off components, per problem
NESTED_SHAPE, NESTED_ROWS = (8, 40), 257


def off_components(K, order="flat-off"):
    """The components an order switches off."""
    if order == "flat-off":
        return (0, 5, K - 1)
    if order == "flat-off-even":
        return tuple(sorted(set(range(0, K, 2)) | {K - 1}))
    return ()


def problem(D, K, N, order, seed=0):
    """-> (Z, c, b, W) of the ladder in the given order."""
    if order.startswith("rising-"):
        Z, c, b, W = SL.problem(D, K, N, int(order.split("-")[1]), seed)
        return Z, c[::-1].copy(), b[::-1].copy(), W
    Z, c, b, W = SL.problem(D, K, N, 0, seed)
    c = c + 0.0                                   # (-0.0 -> 0.0)
    if order not in ("flat", "flat-off", "flat-off-even"):
        raise ValueError(order)
    c[list(off_components(K, order))] = -np.inf
    return Z, c, b, W


class Reference:
    """longdouble CDF of exact logits L (K, N) (entries -inf: switched off) and the bounds of the module docstring."""

    def __init__(self, L):
        K, N = L.shape
        self.K, self.N = K, N
        self.on = np.isfinite(L)
        self.x = L.astype(LD) - L.max(axis=0).astype(LD)                 # exact; -inf where off
        e = np.exp(self.x)                                               # exp(-inf) = 0
        cum = np.cumsum(e, axis=0)
        tot = cum[-1]
        self.e, self.cum = e, cum
        self.F = cum / tot
        self.r = e / tot
        ax = np.where(self.on, np.abs(np.where(self.on, self.x, 0)), 0).astype(np.float64)
        self.term = U * (2.0 * ax + 8.0)
        own = np.cumsum(e * self.term, axis=0)
        own = np.where(cum > 0, own / np.where(cum > 0, cum, 1), 0)     # (nothing on up to k: cum_k = 0 exactly, no error)
        self.relB = own + (self.r * self.term).sum(axis=0)[None, :] + LD(U * (2 * K + 12))
        F, rB = self.F, self.relB
        below = np.vstack([np.zeros((1, N), dtype=LD), F[:-2]])
        self.testable = ((F[:-1] - below > 8 * rB[:-1] * F[:-1]) & (F[1:] - F[:-1] > 8 * rB[:-1] * F[:-1])
                         & (F[:-1] * (1 + 2 * rB[:-1]) < 1) & (F[:-1] > LD(1e-300)))          # (K - 1, N)
        self.upper = F[:-1] * (1 + rB[:-1])        # u above it: the draw must have passed boundary k
        self.lower = F[:-1] * (1 - rB[:-1])        # u not above it: the draw must not have

    def bracket(self, u):
        """-> (least, greatest) label the rule allows for the uniforms u (N,)."""
        ul = np.asarray(u, dtype=np.float64).astype(LD)[None, :]
        return (ul > self.upper).sum(axis=0), (ul > self.lower).sum(axis=0)


@functools.lru_cache(maxsize=None)
def case(D, K, N, order, seed=0):
    """-> (Z, c, b, W, L, Reference), computed once per session and shared; treat every array as read-only."""
    Z, c, b, W = problem(D, K, N, order, seed)
    with np.errstate(invalid="ignore"):
        L = SL.logits(Z, c, b, W)
    for arr in (Z, c, b, W, L):
        arr.setflags(write=False)
    return Z, c, b, W, L, Reference(L)


class Outcome:
    """What run() saw: `step1` rows that missed step 1, `ratio` the worst bisected |u* / F_k - 1| / relB_k (inf with a step-1
    miss), `step3` rows outside their bracket (u = 0 included), `off` labels of a switched-off component, `probed` rows used."""

    def __init__(self):
        self.step1, self.step3, self.off, self.probed, self.ratio, self.notes = 0, 0, 0, 0, 0.0, []

    def ok(self):
        return self.step1 == 0 and self.step3 == 0 and self.off == 0 and self.ratio < 1.0

    def __repr__(self):
        return (f"probed {self.probed}, step 1 misses {self.step1}, worst ratio {self.ratio:.3f}, step 3 misses {self.step3}, "
                f"off labels {self.off}" + ("; " + "; ".join(self.notes[:4]) if self.notes else ""))


def shifts(K):
    return (0, (K - 1) // 2 + 1) if K > 2 else (0,)


def run(draw, ref, off=(), seed=0):
    """The procedure of the module docstring on draw(u (N,) float64) -> labels (N,); off: the switched-off components."""
    K, N = ref.K, ref.N
    out = Outcome()
    rows = np.arange(N)
    offs = np.asarray(sorted(off), dtype=np.int64)

    def launch(u, name=None):
        u = np.ascontiguousarray(u, dtype=np.float64)
        lab = np.asarray(draw(u)).astype(np.int64).reshape(-1)
        assert lab.shape == (N,)
        if offs.size:
            bad = np.isin(lab, offs) & (u > 0)
            if bad.any():
                out.off += int(bad.sum())
                out.notes.append(f"row {int(np.flatnonzero(bad)[0])}: off component {int(lab[bad][0])} at u = {float(u[bad][0])!r}")
        least, greatest = ref.bracket(u)            # (holds for any u: every launch is held to it, not only those of step 3)
        bad = (lab < least) | (lab > greatest)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            out.step3 += int(bad.sum())
            out.notes.append(f"{name or 'probe'}: row {i} label {int(lab[i])} outside [{int(least[i])}, {int(greatest[i])}] at u = {float(u[i])!r}")
        return lab

    for shift in shifts(K):
        k = (rows + shift) % (K - 1)
        use = ref.testable[k, rows]
        Fk, rB = ref.F[k, rows], ref.relB[k, rows]
        # (a boundary that is not testable — it touches a switched-off component, or lies below 1e-300 — is probed all the same
        # where it is a positive normal number: steps 1 and 2 do not judge its rows, the bracket and step 4 do)
        near = np.asarray(use | ((Fk > LD(1e-300)) & (rB < 0.5)))
        u_lo = np.where(near, (Fk * (1 - rB)).astype(np.float64), 0.5)
        u_hi = np.where(near, np.minimum((Fk * (1 + rB)).astype(np.float64), 1.0 - U), 0.5)
        lab_lo, lab_hi = launch(u_lo), launch(u_hi)
        miss = use & ((lab_lo != k) | (lab_hi != k + 1))
        out.probed += int(use.sum())
        if miss.any():
            i = int(np.flatnonzero(miss)[0])
            out.step1 += int(miss.sum())
            out.notes.append(f"row {i} boundary {int(k[i])} (F = {float(Fk[i]):.3e}, relB = {float(rB[i]):.2e}): labels "
                             f"{int(lab_lo[i])} / {int(lab_hi[i])} at u_lo / u_hi")
        lo, hi = u_lo.copy(), u_hi.copy()
        for _ in range(BISECTIONS):
            mid = lo + 0.5 * (hi - lo)
            up = launch(mid) > k
            hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
        good = use & ~miss
        if good.any():
            Fg, rg = Fk[good], rB[good]
            worst = np.maximum(np.abs(lo[good].astype(LD) / Fg - 1), np.abs(hi[good].astype(LD) / Fg - 1)) / rg
            out.ratio = max(out.ratio, float(worst.max()))
        if miss.any():
            out.ratio = float("inf")

    rng = np.random.default_rng(seed)
    grid = rng.integers(1, 1000, size=N) / 1000.0
    logu = 10.0 ** (-290.0 * rng.random(N))
    for name, u in (("u = 0", np.zeros(N)), ("u = 1 - 2^-53", np.full(N, 1.0 - U)), ("random u", np.where(rows % 2 == 0, grid, logu))):
        lab = launch(u, name)
        if name == "u = 0" and (lab != 0).any():
            out.step3 += int((lab != 0).sum())
            out.notes.append(f"u = 0: row {int(np.flatnonzero(lab != 0)[0])} label {int(lab[lab != 0][0])}")
    return out


def float64_draw(L, defect=None):
    """The rule in plain NumPy float64 on the unnormalised sums, as the kernels evaluate it; `defect` plants a known one:
    'ln2'     every exponential times (1 + 1.41e-14 |x|): the reduction constant ln2 / 2048 before it was the nearest double
    'prefix'  chunks of 4 components whose prefix misses component 1: every cumulative sum from component 4 on is short by e_1"""
    with np.errstate(invalid="ignore"):
        x = L - L.max(axis=0)
    e = np.exp(x)
    if defect == "ln2":
        e = e * (1.0 + 1.41e-14 * np.where(np.isfinite(x), np.abs(x), 0.0))
    cum = np.cumsum(e, axis=0)
    if defect == "prefix":
        cum[4:] -= e[1]
    return lambda u: np.sum(np.reshape(u, (1, -1)) * cum[-1][None, :] > cum, axis=0).clip(max=L.shape[0] - 1)
