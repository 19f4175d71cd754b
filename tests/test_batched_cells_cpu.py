"""CPU: what the tables of tests/test_gpu_batched_coverage.py cover, established without a GPU.

tests/batched_checks.py restates the rules of mimo_batched.hip that pick a kernel instantiation and a tile split
(batched_covers, batched_tiles_per_wg, the (NCB, RBW) choice).  Here the restatement is pinned to the constants and
expressions of the sources (read as text), and the GPU module's cell table and row tables are checked against it: all 18
reachable (NCB, RBW) pairs — 54 kernels with the three label modes, which every cell runs — and every tile split property
the GPU tests are there for.  Removing a cell or a row count from the tables fails an assertion here unless another entry
covers the same property."""
import os
import re

import batched_checks as R
import test_gpu_batched_coverage as G
from conftest import ROOT

CSRC = os.path.join(ROOT, "mimo_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert m, f"{name} not found"
    return int(m.group(1))


def test_restated_rules_match_the_sources():
    h, k, hip = _src("mimo_batched.h"), _src("mimo_kernels.h"), _src("mimo_batched.hip")
    assert R.MAX_D == _const(h, "kBatchedMaxD")
    assert R.MAX_K == _const(h, "kBatchedMaxK")
    assert R.MAX_PAIRS == _const(h, "kBatchedMaxPairs")
    assert R.TILE == _const(k, "kTile")
    assert "inline int feat_count(int D) { return (D + 1) * (D + 2) / 2; }" in k
    flat = " ".join(hip.split())
    # batched_tiles_per_wg: ceil(tiles / 128), at least 4
    assert "const int64_t tiles = (nrows + kTile - 1) / kTile;" in flat
    assert f"const int64_t t = (tiles + {R.MAX_WG - 1}) / {R.MAX_WG};" in flat
    assert f"return (int)(t > {R.MIN_TPW} ? t : {R.MIN_TPW});" in flat
    # batched_covers and the column blocks
    assert "static int batched_ncb(int D) { return (feat_count(D) + 15) / 16; }" in flat
    assert "if (D < 1 || D > kBatchedMaxD || K < 1 || K > kBatchedMaxK) return false;" in flat
    assert "return ((K + 15) / 16) * batched_ncb(D) <= kBatchedMaxPairs;" in flat
    # the (NCB, RBW) choice: RBW = 1 up to four row blocks; NCB 9 and 10 exist for RBW = 1 only
    assert "batched_fn fn = a.K16 <= 4 ? pick_batched<1, LM>(ncb) : pick_batched<2, LM>(ncb);" in flat
    cases = sorted(int(x) for x in re.findall(r"case (\d+): return batched_kernel<\1, RBW, LM>;", flat))
    assert cases == list(range(1, 9))
    assert "if constexpr (RBW == 1) { if (ncb == 9) return batched_kernel<9, 1, LM>; if (ncb == 10) return batched_kernel<10, 1, LM>; }" in flat
    # the Philox batch covers eight tiles
    assert f"if (pb.used == {R.PHILOX_BATCH})" in _src("mimo_tile.h")


def test_restated_rules_by_hand():
    """The edges the issue of this module names, worked by hand."""
    assert [R.ncb_of(D) for D in range(1, 17)] == [1, 1, 1, 1, 2, 2, 3, 3, 4, 5, 5, 6, 7, 8, 9, 10]
    assert [R.kmax(D) for D in range(1, 17)] == 11 * [128] + [96, 80, 80, 64, 64]
    assert not R.covers(129, 2) and not R.covers(65, 16) and not R.covers(97, 12) and not R.covers(4, 17)
    assert [R.tiles_per_wg(n) for n in (0, 1, 4099, 16384, 16385, 32768, 32769, 100000)] == [4, 4, 4, 4, 5, 8, 9, 25]
    assert R.split(100) == [(0, 4)] and R.split(16385)[:3] == [(0, 5), (5, 5), (10, 5)] and R.split(0) == []


def reachable_pairs():
    return [(ncb, rbw) for rbw in (1, 2) for ncb in range(1, 11) if R.pair_kmax(ncb, rbw)
            and any(R.ncb_of(D) == ncb for D in range(1, R.MAX_D + 1))]


def test_cells_cover_every_instantiation():
    pairs = reachable_pairs()
    assert len(pairs) == 18 and pairs == [(n, 1) for n in range(1, 11)] + [(n, 2) for n in range(1, 9)]
    assert len(set(G.CELLS)) == len(G.CELLS)
    assert all(R.covers(K, D) for D, K in G.CELLS)
    by_pair = {}
    for D, K in G.CELLS:
        by_pair.setdefault(R.pair_of(D, K), []).append((D, K))
    assert sorted(by_pair) == sorted(pairs)
    for (ncb, rbw), cells in by_pair.items():
        top = R.pair_kmax(ncb, rbw)
        assert top % 16 == 0 and any(K == top for _, K in cells), f"no cell at the largest K = {top} of (NCB, RBW) = {(ncb, rbw)}"
        assert any(K % 16 for _, K in cells), f"no ragged K for (NCB, RBW) = {(ncb, rbw)}"
    # K16 = 4 RBW (the FULL branch of the normalise helpers) for both RBW
    assert any(R.pair_of(D, K)[1] == 1 and K == 64 for D, K in G.CELLS)
    assert any(R.pair_of(D, K)[1] == 2 and K == 128 for D, K in G.CELLS)
    assert sorted({D for D, _ in G.CELLS}) == list(range(1, 17))
    # every cell's batch: an empty problem, a one-row problem, a tile boundary on either side, many workgroups
    assert {0, 1, 31, 32, 33} <= set(G.CELL_ROWS) and max(G.CELL_ROWS) > 4 * R.TILE * R.MIN_TPW
    # the statistics blocks a wave holds at most: 10, reached at K16 NCB = 40
    assert max(-(-K // 16) * R.ncb_of(D) for D, K in G.CELLS) == R.MAX_PAIRS


def _props(n):
    """Tile split properties of a problem of n rows."""
    runs = R.split(n)
    tpw = R.tiles_per_wg(n)
    p = set()
    if not runs:
        return p
    if tpw == R.MIN_TPW and R.tiles_per_wg(n + 1) > R.MIN_TPW:
        p.add("last N with four tiles per workgroup")
    if tpw == R.MIN_TPW + 1 and [t0 for t0, _ in runs[1:3]] == [5, 10]:
        p.add("five tiles: tile0 not a multiple of four")
    if R.PHILOX_BATCH < tpw <= 2 * R.PHILOX_BATCH:
        p.add("one Philox refill")
    if tpw > 2 * R.PHILOX_BATCH:
        p.add("two Philox refills")
    if any(t0 % R.PHILOX_BATCH for t0, _ in runs):
        p.add("tile0 not a multiple of eight")
    if runs[-1][1] < tpw:
        p.add("ragged last workgroup")
    if R.PHILOX_BATCH < runs[-1][1] < tpw:
        p.add("ragged last workgroup with a refill")
    if n % R.TILE == 1:
        p.add("one-row last tile")
    if len(runs) == R.MAX_WG:
        p.add("128 workgroups")
    if len(runs) == R.MAX_WG and tpw > R.MIN_TPW:
        p.add("128 workgroups of more than four tiles")
    if len(runs) > 33:
        p.add("reduce chain over more than 33 blocks")
    assert len(runs) <= R.MAX_WG and all(nt >= 1 for _, nt in runs)
    return p


ROW_PROPERTIES = ["last N with four tiles per workgroup", "five tiles: tile0 not a multiple of four", "one Philox refill",
                  "two Philox refills", "tile0 not a multiple of eight", "ragged last workgroup",
                  "ragged last workgroup with a refill", "one-row last tile", "128 workgroups",
                  "128 workgroups of more than four tiles", "reduce chain over more than 33 blocks"]


def test_row_tables_cover_every_tile_split():
    got = {n: _props(n) for n in G.LARGE_ROWS}
    for prop in ROW_PROPERTIES:
        assert any(prop in p for p in got.values()), f"no row count with: {prop}"
    # each row count is there for a property of its own
    assert R.tiles_per_wg(16384) == 4 and len(R.split(16384)) == 128
    assert (R.tiles_per_wg(16385), len(R.split(16385)), R.split(16385)[-1]) == (5, 103, (510, 3))
    assert (R.tiles_per_wg(20480), len(R.split(20480))) == (5, 128)
    assert (R.tiles_per_wg(20449), len(R.split(20449)), 20449 - 639 * 32) == (5, 128, 1)
    assert (-(-32801 // 32), R.tiles_per_wg(32801)) == (1026, 9)
    assert (-(-70001 // 32), R.tiles_per_wg(70001), len(R.split(70001)), R.split(70001)[-1]) == (2188, 18, 122, (2178, 10))
    for n in (16384, 16385, 20480, 20449, 32801, 70001):
        assert n in G.LARGE_ROWS
    # the mixed batch of the tile split test: every large problem, with empty and tiny problems between them
    rows = G.split_rows()
    assert [n for n in rows if n in G.LARGE_ROWS] == G.LARGE_ROWS
    small = [n for n in rows if n not in G.LARGE_ROWS]
    assert 0 in small and 1 in small and all(R.tiles_per_wg(n) == R.MIN_TPW and len(R.split(n)) <= 1 for n in small)
    assert rows[0] in G.LARGE_ROWS and all(a in G.LARGE_ROWS or b in G.LARGE_ROWS for a, b in zip(rows, rows[1:]))
    # one RBW = 1 shape (the Philox batch is only used there) and one RBW = 2 shape; oracle calls stay in memory
    assert sorted(R.pair_of(D, K)[1] for D, K in G.SPLIT_SHAPES) == [1, 2]
    assert all(8192 * K * D < 1e8 for D, K in G.SPLIT_SHAPES)


def test_chain_rows_give_every_chain_length():
    assert [len(R.split(n)) for n in G.CHAIN_ROWS] == list(range(9))
    assert all(R.covers(K, D) for D, K in G.CHAIN_SHAPES)
    # the four-chain sum: lengths with and without a remainder, and the empty chain
    assert {len(R.split(n)) % 4 for n in G.CHAIN_ROWS} == {0, 1, 2, 3}
