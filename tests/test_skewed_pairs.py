"""The heterogeneous families of tests/skewed_pairs.py have the properties they are there for -- asserted from the scaled
integer coordinates with the index's constants (rj_device.h) restated, as conditions on the inputs -- and the CPU oracle
is consistent with itself on them: the grid equals brute force where no edge exceeds 1/256 of the range, and is a
strict subset of it on the families with long x long crossings (the reference's documented wrap regime)."""
import os
import re

import numpy as np
import pytest

from rayjoin_amd import maps

import skewed_pairs as S

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rayjoin_amd", "csrc", "rj_device.h")


@pytest.fixture(scope="module", autouse=True)
def _threads(oracle):
    """rj_oracle.c runs on one thread unless told otherwise (the brute-force pairs below: tens of seconds on one)"""
    was = oracle.num_threads()
    oracle.lib().rjo_set_num_threads(16)
    yield
    oracle.lib().rjo_set_num_threads(was)


def test_restated_constants_are_the_headers():
    src = open(HDR).read()

    def const(name):
        return int(re.search(r"constexpr int %s = (\d+)" % name, src).group(1))
    assert (const("kQuantShift"), const("kOccShift"), const("kSkyShift")) == (S.QUANT_SHIFT, S.OCC_SHIFT, S.SKY_SHIFT)
    assert (const("kStripMaxSpan"), const("kSkyMaxSpan"), const("kStripYBits")) == (S.STRIP_MAX_SPAN, S.SKY_MAX_SPAN, 31 - S.STRIP_Y_SHIFT)
    assert re.search(r"kStripShiftMin = 15, kStripShiftMax = 17", src) and S.STRIP_SHIFTS == (15, 16, 17)
    assert "kCoordOffset = (int64_t) 1 << 46" in src and S.COORD_OFFSET == 1 << 46
    assert const("kOccMaxCellsPerSeg") == S.OCC_MAX_CELLS
    assert S.MAX_EDGE == maps.INTERNAL_RANGE // 256


@pytest.mark.parametrize("name", S.NAMES)
def test_family_is_a_valid_pair_inside_the_scaled_range(name):
    ctx = S.family(name)
    for m in ctx.maps:
        assert m.pts.min() >= maps.INTERNAL_MIN and m.pts.max() <= maps.INTERNAL_MAX
        assert np.all(np.diff(m.row_index.astype(np.int64)) >= 2) and m.n_edges > 0
        s = m.segments()
        assert np.all((s[:, 0] != s[:, 2]) | (s[:, 1] != s[:, 3]))   # no zero-length edge (planar_graph.h:85)
        assert m.n_edges <= 52000   # (brute force stays a matter of seconds)
    long_edge = max(S.longest_edge(m) for m in ctx.maps) > S.MAX_EDGE
    assert long_edge == (not ctx.skew["grid_ok"]), name
    if name in S.OVERLAY_VALID:
        assert ctx.skew["grid_ok"]


@pytest.mark.parametrize("name", ["skew_lattice", "skew_rings", "skew_short_chains"])
def test_skewed_families_are_dense_in_a_corner(name):
    ctx = S.family(name)
    box = ctx.skew["dense"]
    assert (box[2] - box[0]) * (box[3] - box[1]) <= 0.05
    for m in ctx.maps:
        assert S.dense_share(m, box) >= 0.80, (name, m.map_id, S.dense_share(m, box))
    m0 = ctx.maps[0]
    chain_len = np.diff(m0.row_index.astype(np.int64)) - 1
    if name == "skew_lattice":     # long chains, mostly open: no column index at the build (the lazy build's map)
        assert m0.n_edges // m0.n_chains >= 16
    if name == "skew_rings":
        closed = np.all(m0.pts[m0.row_index[:-1].astype(np.int64)] == m0.pts[m0.row_index[1:].astype(np.int64) - 1], axis=1)
        assert 2 * int(closed.sum()) >= m0.n_chains
        assert 16 < S.strip_span(m0, 17).max() <= S.STRIP_MAX_SPAN and S.strip_span(m0, 15).max() <= S.STRIP_MAX_SPAN
        # what the re-count test of tests/test_gpu_skewed.py relies on: at 2^15 the entries exceed the build's estimate,
        # min(2 slots, 2.5 edges + 64), whatever the slot count
        assert S.column_entries(m0, 15) > 5 * m0.n_edges // 2 + 64
    if name == "skew_short_chains":
        assert m0.n_edges // m0.n_chains < 16 and chain_len.max() >= 150
        assert int((chain_len >= 150).sum()) >= 20
        assert all(S.column_entries(m0, sh) is not None for sh in S.STRIP_SHIFTS)


@pytest.mark.parametrize("name", ["rings_frame", "short_chains_frame", "outlier"])
def test_frames_are_too_wide_for_the_strips_and_the_skyline(oracle, name):
    ctx = S.family(name)
    assert ctx.skew["frame"]
    for im in ctx.skew["frame"]:
        m = ctx.maps[im]
        for sh in S.STRIP_SHIFTS:
            assert S.strip_span(m, sh).max() > S.STRIP_MAX_SPAN and S.column_entries(m, sh) is None
        assert S.strip_span(m, S.SKY_SHIFT).max() > S.SKY_MAX_SPAN
    m0 = ctx.maps[0]
    if name == "rings_frame":
        # the frame's oblique edges are NOT rasterised into the occupancy bitmap (their boxes cover more than kOccMaxCellsPerSeg
        # cells), every other edge of map 0 is; short edges of map 1 cross the frame with their whole box in cells that no
        # rasterised edge touches: there only the bitmap's "not rasterised" flag keeps the LSI pre-filter from dismissing them
        cells = S.box_cells(m0)
        small = np.arange(m0.n_edges) < m0.n_edges - 4   # (the frame is the last chain)
        assert cells[~small].min() > 20 * S.OCC_MAX_CELLS and cells[small].max() <= S.OCC_MAX_CELLS
        x0, y0, x1, y1 = (v >> S.OCC_SHIFT for v in S.edge_boxes(m0))
        occupied = np.zeros((4096, 4096), dtype=bool)   # the cells the rasterised boxes set
        for dx in range(int((x1 - x0)[small].max()) + 1):
            for dy in range(int((y1 - y0)[small].max()) + 1):
                occupied[np.minimum(y0[small] + dy, y1[small]), np.minimum(x0[small] + dx, x1[small])] = True
        om = S.oracle_maps(oracle, ctx)
        pairs = oracle.lsi_brute(om[0], om[1])
        e = np.unique(pairs[pairs[:, 0] >= m0.n_edges - 4][:, 1].astype(np.int64))
        assert len(e) >= 100
        qx0, qy0, qx1, qy1 = (v >> S.OCC_SHIFT for v in S.edge_boxes(ctx.maps[1]))
        # (k_lsi's pre-filter judges a query box of up to 2 x 2 cells -- occ_verdict_code -- and leaves larger ones to the tree)
        e = e[((qx1 - qx0)[e] <= 1) & ((qy1 - qy0)[e] <= 1)]
        clear = np.ones(len(e), dtype=bool)
        for dx in range(-1, 3):   # (the box and a margin of one cell around it)
            for dy in range(-1, 3):
                clear &= ~occupied[qy0[e] + dy, qx0[e] + dx]
        assert int(clear.sum()) >= 100, int(clear.sum())
        closed = np.all(m0.pts[m0.row_index[:-1].astype(np.int64)] == m0.pts[m0.row_index[1:].astype(np.int64) - 1], axis=1)
        assert 2 * int(closed.sum()) >= m0.n_chains
    if name == "short_chains_frame":
        assert m0.n_edges // m0.n_chains < 16
    if name in ("short_chains_frame", "outlier"):
        # an AXIS-PARALLEL frame is rasterised however long it is: the box of an edge is one cell thick, at most 4096 cells
        for im in ctx.skew["frame"]:
            assert S.box_cells(ctx.maps[im])[-4:].max() <= S.OCC_MAX_CELLS
    if name == "outlier":   # map 0's oblique long edges are not (the flag is raised; every short query edge lies in set cells, though)
        assert S.box_cells(m0).max() > S.OCC_MAX_CELLS


def _share_of_the_fullest(cells):
    _, counts = np.unique(cells, return_counts=True)
    return counts.max() / len(cells), len(counts)


def test_outlier_squeezes_the_map_into_a_few_cells():
    ctx = S.family("outlier")
    for m in ctx.maps:
        x0, y0, x1, y1 = S.edge_boxes(m)
        cell = ((y0 >> S.OCC_SHIFT) << 12) | (x0 >> S.OCC_SHIFT)
        share, _ = _share_of_the_fullest(cell)
        assert share >= 0.25, (m.map_id, share)
        # nearly every edge lies within 4 x 4 cells of the 4096 x 4096
        tiny = ((x1 >> S.OCC_SHIFT) - np.median(x0 >> S.OCC_SHIFT) <= 3) & ((y1 >> S.OCC_SHIFT) - np.median(y0 >> S.OCC_SHIFT) <= 3)
        assert tiny.mean() >= 0.99
    # long edges in BOTH maps (long x long crossings), and map 0's long chains leave the strips possible at no width
    assert all(S.longest_edge(m) > 16 * S.MAX_EDGE for m in ctx.maps)


def test_long_long_has_domain_spanning_segments_in_both_maps():
    ctx = S.family("long_long")
    for im, m in enumerate(ctx.maps):
        s = m.segments()
        ext = np.maximum(np.abs(s[:, 2] - s[:, 0]), np.abs(s[:, 3] - s[:, 1]))
        assert int((ext > maps.INTERNAL_RANGE // 4).sum()) == ctx.skew["n_long"][im] >= 4
        small = ext <= maps.INTERNAL_RANGE // 4
        # the small ones share ONE Morton cell (16 bits per axis of the 31-bit quantised coordinate: 2^15 quanta) or its neighbour
        q = S.quant(s[small][:, :2]) >> 15
        assert np.ptp(q[:, 0]) <= 1 and np.ptp(q[:, 1]) <= 1
        assert S.column_entries(m, 17) is None   # one-edge chains want columns; the long ones decline them
        assert S.box_cells(m).max() > S.OCC_MAX_CELLS   # ... and are not rasterised into the occupancy bitmap


def test_thin_band_lies_in_one_height_bucket():
    ctx = S.family("thin_band")
    for m in ctx.maps:
        x0, y0, x1, y1 = S.edge_boxes(m)
        inside = (y0 >> S.STRIP_Y_SHIFT) == (y1 >> S.STRIP_Y_SHIFT)
        share, _ = _share_of_the_fullest((y0 >> S.STRIP_Y_SHIFT)[inside])
        assert inside.mean() * share >= 0.95, (m.map_id, share)
        assert (x0 >> 17).max() - (x0 >> 17).min() >= 0.9 * (1 << 14)   # ... over (nearly) all of the 16 384 widest strips
        assert np.ptp(y0) >= 0.95 * (1 << 31)                            # the outliers fix the bounding box
        assert all(S.column_entries(m, sh) is not None for sh in S.STRIP_SHIFTS)


@pytest.mark.parametrize("name", S.NAMES)
def test_oracle_is_consistent_with_itself(oracle, name):
    ctx = S.family(name)
    om = S.oracle_maps(oracle, ctx)
    brute = oracle.lsi_brute(om[0], om[1])
    grid = oracle.lsi_grid(om[0], om[1], 256)["eid"]
    assert len(brute) >= 100, (name, len(brute))
    if ctx.skew["grid_ok"]:
        assert np.array_equal(grid, brute), (name, len(grid), len(brute))
        for base in (0, 1):
            q = ctx.maps[1 - base].pts
            assert np.array_equal(oracle.pip_grid(om[base], base, q, 256), oracle.pip_brute(om[base], 1 - base, q)), (name, base)
    key = lambda p: set((p[:, 0].astype(np.int64) << 32 | p[:, 1]).tolist())
    if name in ("outlier", "long_long"):
        # long x long crossings fall in the wrap regime of the grid path's rational<__int128>: the grid misses some of them
        assert key(grid) < key(brute), (name, len(grid), len(brute))
        print("%s: %d pairs by brute force, %d from the grid" % (name, len(brute), len(grid)))
    if name == "outlier":   # the figures INTEGRATION.md section 5 quotes
        assert (len(brute), len(grid)) == (3801, 3788)
    if name == "outlier":   # PIP does not hang on the grid's intersection points
        for base in (0, 1):
            q = ctx.maps[1 - base].pts
            assert np.array_equal(oracle.pip_grid(om[base], base, q, 256), oracle.pip_brute(om[base], 1 - base, q)), (name, base)


def test_fuzz_boxes_span_two_orders_of_magnitude():
    for seed in range(20):
        rng = np.random.default_rng(seed)
        for n in (2, 3, 4):
            boxes = S.fuzz_boxes(rng, n)
            for i, a in enumerate(boxes):
                assert 0 < a[0] < a[2] < 1 and 0 < a[1] < a[3] < 1
                for b in boxes[i + 1:]:
                    assert a[2] <= b[0] or b[2] <= a[0] or a[3] <= b[1] or b[3] <= a[1]
