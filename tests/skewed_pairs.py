"""Input families for the index on HETEROGENEOUS maps (test infrastructure, not collected by pytest): every other map of
the suite fills its bounding box uniformly, while the index fixes its resolutions relative to the scaled domain (the
4096^2 occupancy bitmap, the 2^13-quanta skyline buckets, strips of 2^15..2^17 quanta with 1024 height buckets, Morton
keys of 16 bits per axis) and decides several things once per map (one strip width, columns for rings or short chains,
one run cap, the LSI launch form by the bitmap's density).  The families here are dense in one corner and nearly empty
elsewhere, squeezed into a few cells by an outlier, crossed by edges as long as the domain, or flat inside one height
bucket.  One function per family returning a maps.Context whose .skew dict says what the family is for:

  grid_ok   no edge is longer than MAX_EDGE (1/256 of the scaled range): the grid oracle equals brute force and the
            overlay is inside its validity domain.  Where it is False some edge is in the documented wrap regime of the
            reference's rational<__int128> (DESIGN.md "Validity domain"): the pair list is held to lsi_brute alone.
  frame     the map ids that hold a frame (a closed 4-edge ring around the domain): the column index declines there.

tests/test_skewed_pairs.py asserts each family's defining property from the scaled integer coordinates alone, with the
index's constants restated below, so a generator change that loses the skew fails on the CPU."""
import numpy as np

from rayjoin_amd import maps, synth

MAX_EDGE = maps.INTERNAL_RANGE // 256
# rj_device.h, restated (tests/test_skewed_pairs.py checks them against the header)
QUANT_SHIFT, COORD_OFFSET = 16, 1 << 46
OCC_SHIFT, SKY_SHIFT, STRIP_Y_SHIFT = 19, 13, 21
STRIP_MAX_SPAN, SKY_MAX_SPAN = 1024, 2048
STRIP_SHIFTS = (15, 16, 17)


def quant(v):
    """the 31-bit quantised coordinate of the boxes (rj_device.h quant())"""
    return (np.asarray(v, dtype=np.int64) + COORD_OFFSET) >> QUANT_SHIFT


def edge_boxes(m):
    """quantised (x0, y0, x1, y1) of every edge of a ScaledMap, in eid order: the leaves' boxes (k_build_leaves)"""
    s = quant(m.segments())
    return np.minimum(s[:, 0], s[:, 2]), np.minimum(s[:, 1], s[:, 3]), np.maximum(s[:, 0], s[:, 2]), np.maximum(s[:, 1], s[:, 3])


def strip_span(m, shift):
    """strips of 2^shift quanta every edge's box touches (k_strip_count)"""
    x0, _, x1, _ = edge_boxes(m)
    return (x1 >> shift) - (x0 >> shift) + 1


def column_entries(m, shift):
    """entries of the column index at this strip width, or None where build_strips declines"""
    c = strip_span(m, shift)
    return None if c.max() > STRIP_MAX_SPAN else int(c.sum())


def longest_edge(m):
    s = m.segments()
    return int(max(np.abs(s[:, 2] - s[:, 0]).max(), np.abs(s[:, 3] - s[:, 1]).max()))


# what Scaling(US_BBOX) maps onto the whole scaled range: the box with the reference's margin of one unit around it
DOMAIN = (synth.US_BBOX[0] - maps.SCALING_BOUNDING_BOX_MARGIN, synth.US_BBOX[1] - maps.SCALING_BOUNDING_BOX_MARGIN,
          synth.US_BBOX[2] + maps.SCALING_BOUNDING_BOX_MARGIN, synth.US_BBOX[3] + maps.SCALING_BOUNDING_BOX_MARGIN)


def sub_bbox(fx0, fy0, fx1, fy1, bbox=DOMAIN):
    """the part of bbox between these fractions of its extent (of DOMAIN: fractions of the scaled range)"""
    x0, y0, x1, y1 = bbox
    return (x0 + fx0 * (x1 - x0), y0 + fy0 * (y1 - y0), x0 + fx1 * (x1 - x0), y0 + fy1 * (y1 - y0))


def compose(parts):
    """one PlanarGraph of several: chains and points concatenated, chain ids renumbered, point indices offset, the
    nonzero face ids of every part offset past those of the parts before it"""
    chains, rows, pts = [], [np.zeros(1, np.int64)], []
    np_off = nc_off = face_off = 0
    for g in parts:
        c = g.chains.copy()
        c[:, 0] = np.arange(g.n_chains) + nc_off
        c[:, 1] += np_off
        c[:, 2] += np_off
        for col in (3, 4):
            c[:, col] = np.where(c[:, col] != 0, c[:, col] + face_off, 0)
        chains.append(c)
        rows.append(g.row_index[1:].astype(np.int64) + np_off)
        pts.append(g.points)
        np_off += g.n_points
        nc_off += g.n_chains
        face_off = max(face_off, int(c[:, 3:5].max()) if len(c) else 0)
    return maps.PlanarGraph(np.concatenate(chains), np.concatenate(rows).astype(np.uint32), np.concatenate(pts))


def frame(bbox, face=1, skew=0.0):
    """one closed ring of 4 edges inside bbox, counter-clockwise, `face` on its left (inside).  skew = 0: the box itself,
    axis-parallel edges whose boxes are one cell thick.  skew > 0: every corner moved along its side by that share of the
    side -- a slightly rotated frame, OBLIQUE long edges whose boxes cover a whole band of cells"""
    x0, y0, x1, y1 = bbox
    dx, dy = skew * (x1 - x0), skew * (y1 - y0)
    pts = np.array([[x0, y0 + dy], [x1 - dx, y0], [x1, y1 - dy], [x0 + dx, y1], [x0, y0 + dy]], dtype=np.float64)
    return maps.PlanarGraph(np.array([[0, 0, 4, face, 0]], np.int64), np.array([0, 5], np.uint32), pts)


def _tick(at, d=0.002, face=0):
    """an open chain of two short edges at the fractions `at` of the domain (an outlier that fixes a bounding box)"""
    b = sub_bbox(at[0], at[1], at[0] + d, at[1] + d)
    pts = np.array([[b[0], b[1]], [b[2], b[1]], [b[2], b[3]]], dtype=np.float64)
    return maps.PlanarGraph(np.array([[0, 0, 2, face, 0]], np.int64), np.array([0, 3], np.uint32), pts)


def _context(g0, g1, **what):
    """two planar graphs under ONE Scaling, that of synth.US_BBOX (every family stays inside it)"""
    sc = maps.Scaling(synth.US_BBOX)
    ctx = maps.Context([None, None])
    ctx.scaling = sc
    ctx.bb = synth.US_BBOX
    for im, g in enumerate((g0, g1)):
        ctx.set_map(im, maps.ScaledMap(im, sc.scale(g.points), g.row_index, g.chains[:, 3], g.chains[:, 4]))
    ctx.skew = dict(what, frame=what.get("frame", ()))
    return ctx


# the dense corner of the skewed families: 3.2 % of the domain's area (4.4 % with the 0.3 cell its vertices jitter past it)
DENSE = (0.02, 0.02, 0.20, 0.20)
DENSE_AREA = (0.005, 0.005, 0.215, 0.215)
SPARSE = ((0.35, 0.08, 0.65, 0.38), (0.58, 0.52, 0.94, 0.90))
L = synth.lattice_map


def _skew_lattice_map(which):
    """a dense lattice in DENSE plus two coarse ones elsewhere; which = 0 / 1: the two maps of a pair (different cell
    counts, so that their lines cross); every edge stays below MAX_EDGE"""
    dense = ((18, 40), (25, 32))[which]
    coarse = ((4, 64), (3, 96)) if which == 0 else ((5, 56), (4, 72))
    return compose([L(dense[0], dense[1], 300 + which, bbox=sub_bbox(*DENSE))]
                   + [L(G, k, 310 + 2 * which + i, bbox=sub_bbox(*SPARSE[i])) for i, (G, k) in enumerate(coarse)])


def skew_lattice():
    """85 % / 87 % of the two maps' edges in 3.2 % of the area: the occupancy bitmap, the Morton keys and the leaf tables see
    a few cells of the domain; long chains, so no columns at build time (the lazy build's map)"""
    return _context(_skew_lattice_map(0), _skew_lattice_map(1), family="skew_lattice", grid_ok=True, dense=DENSE_AREA)


def skew_rings():
    """map 0: 3500 small rings in DENSE plus 40 large rings over the rest -- ONE strip width from a mean the sparse part
    does not share: its widest segments span tens of strips at 2^17 and hundreds at 2^15; map 1: a skewed lattice"""
    g0 = compose([synth.ring_map(3500, 35000, 321, bbox=sub_bbox(*DENSE)),
                  synth.ring_map(40, 6000, 322, bbox=sub_bbox(0.3, 0.3, 0.8, 0.8), clusters=8)])
    return _context(g0, _skew_lattice_map(1), family="skew_rings", grid_ok=True, dense=DENSE_AREA)


def skew_short_chains():
    """map 0: a dense lattice of 6-edge chains plus two coarse lattices of chains of 150 and 200 edges: the mean chain
    length (below 16) decides for columns and one run cap on a map whose sparse part has long chains"""
    g0 = compose([L(50, 6, 331, bbox=sub_bbox(*DENSE)), L(3, 150, 332, bbox=sub_bbox(*SPARSE[0])), L(2, 200, 333, bbox=sub_bbox(*SPARSE[1]))])
    return _context(g0, _skew_lattice_map(1), family="skew_short_chains", grid_ok=True, dense=DENSE_AREA)


INNER = (0.03, 0.03, 0.97, 0.97)   # where a framed map's content lies (the lattices' vertices jitter by 0.3 cell), and rings_frame's frame
FRAME = (0.004, 0.004, 0.996, 0.996)
FRAME_SKEW = 0.0106                # rings_frame: corners moved by 1 % of the side, edges 41 bitmap cells off the axes
OCC_MAX_CELLS = 4096               # kOccMaxCellsPerSeg: a box of more cells is not rasterised, the bitmap's flag word is raised


def box_cells(m):
    """cells of the occupancy bitmap every edge's box covers (mark_occupancy_wave: more than OCC_MAX_CELLS: not rasterised)"""
    x0, y0, x1, y1 = (v >> OCC_SHIFT for v in edge_boxes(m))
    return (x1 - x0 + 1) * (y1 - y0 + 1)


def rings_frame():
    """a homogeneous ring map inside one slightly ROTATED frame: its long edges span 15 000 strips at every width, so the
    column index the ring rule wants is not built, and the skyline is filled from the leaf boxes with its "too wide to
    register" word set.  The frame's edges are oblique: the box of each covers 150 000 cells of the occupancy bitmap, so
    none is rasterised and the bitmap's flag word says so (an axis-parallel frame's box is one cell thick, at most 4096
    cells: rasterised).  Map 1's lattice reaches past the frame, and six FINE lattices of map 1 (edges of half a cell: the
    pre-filter judges boxes of up to 2 x 2 cells and leaves larger ones to the tree) straddle the frame's bottom edge:
    its edges cross the frame in cells that no rasterised edge of map 0 touches -- there only the flag keeps the LSI
    pre-filter from dismissing them"""
    g0 = compose([synth.ring_map(3000, 30000, 341, bbox=sub_bbox(0.08, 0.08, 0.92, 0.92)), frame(sub_bbox(*INNER), skew=FRAME_SKEW)])
    inside = (INNER[0] + FRAME_SKEW, INNER[1] + FRAME_SKEW, INNER[2] - FRAME_SKEW, INNER[3] - FRAME_SKEW)
    side = INNER[2] - INNER[0]
    bottom = lambda x: INNER[1] + FRAME_SKEW * side * (1 - (x - INNER[0]) / (side * (1 - FRAME_SKEW)))   # the frame's bottom edge over x
    fine = [L(10, 16, 343 + i, bbox=sub_bbox(x - 0.01, bottom(x) - 0.01, x + 0.01, bottom(x) + 0.01)) for i, x in enumerate((0.2, 0.3, 0.4, 0.5, 0.6, 0.7))]
    g1 = compose([L(24, 24, 342, bbox=sub_bbox(0.015, 0.015, 0.985, 0.985))] + fine)
    return _context(g0, g1, family="rings_frame", grid_ok=False, frame=(0,), frame_box=inside,
                    frame_top=INNER[3])


def short_chains_frame():
    """a lattice of 9-edge chains plus the frame: the short-chain rule wants columns, the frame makes the build decline.
    Map 1 has a frame of its own that CROSSES map 0's (long x long in the reference's wrap regime)"""
    g0 = compose([L(48, 9, 351, bbox=sub_bbox(*INNER)), frame(sub_bbox(*FRAME))])
    g1 = compose([L(32, 24, 352, bbox=sub_bbox(*INNER)), frame(sub_bbox(0.001, 0.012, 0.999, 0.990))])
    return _context(g0, g1, family="short_chains_frame", grid_ok=False, frame=(0, 1), frame_box=FRAME, frame_top=FRAME[3])


TINY = 1.0 / 3000   # of the range per axis: about one and a half occupancy cells
KNOT = 1e-8         # ... and a lattice inside 21 quanta: every box of it overlaps most of the others


def outlier(tiny=TINY, knot=KNOT):
    """each map: a lattice of about 15 k edges inside 1/3000 of the range per axis -- a quarter of the edges share one
    cell of the 16.7 M of the occupancy bitmap, and nearly all share a handful of Morton keys and x-buckets -- and beside
    it a KNOT, a small lattice inside 10^-8 of the range (a few quanta: the integer boxes of its edges cannot tell them
    apart, a point's candidate list overflows there); map 0 adds lattice_map(2, 3) over the whole range, map 1 a frame
    over 0.1 .. 0.9 (long x long crossings)"""
    at = (0.4003, 0.4003)
    box = sub_bbox(at[0], at[1], at[0] + tiny, at[1] + tiny)
    kbox = sub_bbox(at[0] + 1.6 * tiny, at[1] + 0.5 * tiny, at[0] + 1.6 * tiny + knot, at[1] + 0.5 * tiny + knot)
    g0 = compose([L(30, 8, 361, bbox=box), L(12, 4, 364, bbox=kbox), L(2, 3, 362, bbox=sub_bbox(0.12, 0.12, 0.88, 0.88))])
    g1 = compose([L(43, 4, 363, bbox=box), L(9, 5, 365, bbox=kbox), frame(sub_bbox(0.1, 0.1, 0.9, 0.9))])
    return _context(g0, g1, family="outlier", grid_ok=False, frame=(1,), tiny=box)


def long_long():
    """integer segments: thousands of small ones around the origin (all of them inside ONE 16-bit Morton cell) and in
    each map several segments as long as the domain that cross the other map's (tests/test_gpu_parity.py
    test_domain_spanning_segments has them in one map only)"""
    B, H = 1 << 45, 1 << 44
    big0 = np.array([[-B, -B + 7, B, B - 3], [-B, H, B, -H], [5, -B, 9, B], [-B + 11, 3 * H // 2, B - 5, 3 * H // 2 + 1001]], dtype=np.int64)
    big1 = np.array([[-B, B - 70001, B, -B + 31], [-H, -B, H + 3, B], [-B, -H - 5, B - 1, H // 2], [B - 77, -B, -B + 1013, B - 9], [3 * H // 2, -B, 3 * H // 2 - 999, B]],
                    dtype=np.int64)
    a = np.concatenate([synth.adversarial_segments(2000, 1 << 30, 371), big0.reshape(-1, 2)])
    b = np.concatenate([synth.adversarial_segments(2500, 1 << 30, 372), big1.reshape(-1, 2)])
    ctx = maps.Context([None, None])
    ctx.scaling = maps.Scaling(synth.US_BBOX)
    ctx.bb = synth.US_BBOX
    ctx.maps = [maps.ScaledMap.from_segments(0, a), maps.ScaledMap.from_segments(1, b)]
    ctx.skew = dict(family="long_long", grid_ok=False, frame=(), n_long=(len(big0), len(big1)))
    return ctx


BAND = (501.25 / 1024, 501.75 / 1024)   # in y, of the range: the middle half of height bucket 501


def thin_band():
    """nearly all edges of both maps inside ONE height bucket of the strips (2^21 quanta in y, 1/1024 of the range),
    spread over the whole x-range: a strip's 1024-bucket table is one step function, every entry of a strip lies in one
    bucket.  Two outlier chains per map fix the bounding box"""
    band = sub_bbox(0.02, BAND[0], 0.98, BAND[1])
    ticks = [_tick((0.003, 0.003)), _tick((0.994, 0.994))]
    g0 = compose([L(40, 12, 381, bbox=band, seg_jitter=0.01)] + ticks)   # (the jitter across a chain is a share of its LENGTH: rows overlap)
    g1 = compose([L(48, 10, 382, bbox=band, seg_jitter=0.01)] + ticks)
    return _context(g0, g1, family="thin_band", grid_ok=True, band=BAND)


FAMILIES = (("skew_lattice", skew_lattice), ("skew_rings", skew_rings), ("skew_short_chains", skew_short_chains), ("rings_frame", rings_frame),
            ("short_chains_frame", short_chains_frame), ("outlier", outlier), ("long_long", long_long), ("thin_band", thin_band))
NAMES = [n for n, _ in FAMILIES]
OVERLAY_VALID = ("skew_lattice", "skew_rings")

_cache = {}


def family(name):
    """the family's Context (kept: the generators are deterministic and a module's tests share them)"""
    if name not in _cache:
        _cache[name] = dict(FAMILIES)[name]()
    return _cache[name]


def oracle_maps(oracle, ctx):
    return [oracle.Map(m.pts, m.row_index, m.left, m.right) for m in ctx.maps]


def dense_share(m, box):
    """share of the map's edges whose mid-point lies in the part `box` (fractions) of the scaled range"""
    s = m.segments()
    mx, my = (s[:, 0] + s[:, 2]) // 2, (s[:, 1] + s[:, 3]) // 2
    lo, rng = maps.INTERNAL_MIN, maps.INTERNAL_RANGE
    fx, fy = (mx - lo) / rng, (my - lo) / rng
    return float(((fx >= box[0]) & (fx <= box[2]) & (fy >= box[1]) & (fy <= box[3])).mean())


# ---- the heterogeneous fuzz: parts of tests/test_gpu_fuzz.py's kinds in random disjoint boxes -------------------------------
def _in_box(g, box):
    """the planar graph g (over US_BBOX, vertices possibly jittered a little past it) mapped affinely into `box`"""
    x0, y0, x1, y1 = synth.US_BBOX
    lo = np.minimum(g.points.min(axis=0), [x0, y0])
    hi = np.maximum(g.points.max(axis=0), [x1, y1])
    p = (g.points - lo) / (hi - lo)
    pts = np.stack([box[0] + p[:, 0] * (box[2] - box[0]), box[1] + p[:, 1] * (box[3] - box[1])], 1)
    return maps.PlanarGraph(g.chains, g.row_index, pts)


def fuzz_boxes(rng, n):
    """n disjoint boxes (fractions of the domain) whose areas span at least two orders of magnitude: one per cell of a
    2 x 2 split of (0.02 .. 0.98)^2, the first tiny (side 0.01 .. 0.04), the last filling its cell"""
    cells = [(i, j) for i in range(2) for j in range(2)]
    order = rng.permutation(4)[:n]
    out = []
    for k, c in enumerate(order):
        i, j = cells[int(c)]
        cx0, cy0 = 0.02 + 0.48 * i, 0.02 + 0.48 * j
        side = float(rng.uniform(0.01, 0.04)) if k == 0 else 0.44 if k == n - 1 else float(10 ** rng.uniform(-1.3, -0.4))
        ox, oy = float(rng.uniform(0, 0.44 - side)), float(rng.uniform(0, 0.44 - side))
        out.append((cx0 + ox, cy0 + oy, cx0 + ox + side, cy0 + oy + side))
    areas = [(b[2] - b[0]) * (b[3] - b[1]) for b in out]
    assert max(areas) >= 100 * min(areas)
    return out


def fuzz_pair(rng, draw_map):
    """-> Context of a random heterogeneous pair: each map 2-4 parts drawn by draw_map(rng) (test_gpu_fuzz._maps) in
    the SAME random boxes (so that the maps cross), a frame added to either map with probability 1/3 -- axis-parallel or
    slightly rotated (oblique long edges: not rasterised into the occupancy bitmap), half and half"""
    n = int(rng.integers(2, 5))
    boxes = fuzz_boxes(rng, n)
    gs, frames = [], []
    for im in range(2):
        parts = [_in_box(draw_map(rng), sub_bbox(*b)) for b in boxes]
        if rng.integers(0, 3) == 0:
            d = float(rng.uniform(0.001, 0.015))
            parts.append(frame(sub_bbox(d, d, 1 - d, 1 - d), skew=float(rng.integers(0, 2) * rng.uniform(0.002, 0.02))))
            frames.append(im)
        gs.append(compose(parts))
    return _context(gs[0], gs[1], family="fuzz", grid_ok=False, frame=tuple(frames), boxes=boxes)
