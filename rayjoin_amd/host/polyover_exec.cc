// polyover_exec -- RayJoin's polygon-overlay driver (src/overlay.cc, src/run_overlay.cu:143-228)
// on the MI355X-native LSI / PIP path.  Same flags, phases and stderr timing format.
//   MapOverlayLBVH::{Init, BuildIndex, IntersectEdge, LocateVerticesInOtherMap,
//                    ComputeOutputPolygons, WriteResult}     src/app/map_overlay_lbvh.h:25-270
//   -mode=grid (MapOverlayGrid, src/app/map_overlay_grid.h) runs the same stages on the device-side
//   uniform grid; -check compares the LBVH results with the grid's, as run_overlay.cu:18-141 does.
//   -face_table <path> (ours): the overlay's face table computed on the device from the same records
//   (rj_overlay_faces) -- "f0 f1 area" per row, area in input units.
//   -output_map <path> (ours): the output map computed on the device (rj_overlay_map) and written as a CDB file: the
//   device map's chains and points (unscaled, "%.6f"), its ordered-pair face ids, end points numbered over the distinct
//   scaled end points in order of first use.  -output stays the host writer's file.
//   -how intersection|union|difference|symmetric_difference|identity, -by pair|map0|map1 (ours): the overlay operation
//   of -face_table and -output_map (rj_overlay_faces_op / rj_overlay_map_op): which (face of map 0, face of map 1) pairs
//   are faces of the result and what names a face; a face id in the files may then be 0 ("outside that map").  Without
//   either flag the two files are the intersection's (the calls without _op), byte for byte what they were.
//   -merge (ours): -output_map with RJ_OVM_MERGE_PIECES: adjacent pieces of one source chain that have the same two
//   faces and touch are written as one chain (what a dissolve leaves of a chain the other map cut).
//   -polygons <path> (ours): the polygons of the result, on the device: the output map (under -how, -by, -merge), its
//   rings without those of face 0 (rj_map_rings, RJ_RINGS_SKIP_FACE0), every hole assigned to its outer ring
//   (rj_rings_polygons).  One line per polygon: "f0 f1 area2 POLYGON ((shell), (hole), ...)" -- (f0, f1) the polygon's row
//   of face_pairs, area2 twice its area in scaled units^2 (exact), the points unscaled ("%.6f"), every ring closed.
//   -coarse_map <path> (ours): the map of -output_map (under -how, -by, -merge) without its degenerate pieces, taken through
//   its rings (rj_map_rings) and back (rj_rings_map): the same faces and boundaries with maximal chains -- a chain ends
//   only where three or more boundaries meet or the faces change -- written as -output_map writes.
#include <iostream>
#include <unordered_map>

#include "context.h"
#include "flags.h"
#include "output_chain.h"
#include "timer.h"

using namespace rayjoin;

namespace {

class MapOverlayLBVH {
 public:
  MapOverlayLBVH(Context& ctx, double xsect_factor, bool grid = false, int grid_size = 2048, bool keep_xsects = false)
      : ctx_(ctx), xsect_factor_(xsect_factor), grid_(grid), grid_size_(grid_size), keep_xsects_(keep_xsects) {}
  // -how / -by: the files of -face_table / -output_map come from the _op calls
  void SetOperation(const std::string& how, const std::string& by) {
    static const char* hows[] = {"intersection", "union", "difference", "symmetric_difference", "identity"};
    static const char* bys[] = {"pair", "map0", "map1"};
    auto index = [](const std::string& v, const char* const* names, int n, const char* flag) {
      if (v.empty()) return 0u;
      for (int i = 0; i < n; i++)
        if (v == names[i]) return (uint32_t) i;
      throw std::invalid_argument(std::string("bad value '") + v + "' for -" + flag);
    };
    how_ = index(how, hows, 5, "how");
    by_ = index(by, bys, 3, "by");
    use_op_ = !how.empty() || !by.empty();
  }
  void SetMerge(bool merge) { map_flags_ = merge ? RJ_OVM_MERGE_PIECES : 0; }
  ~MapOverlayLBVH() {
    rj_handle h = ctx_.handle();
    if (pairs_) rj_dev_free(h, pairs_);
    for (int im = 0; im < 2; im++) {
      if (closest_[im]) rj_dev_free(h, closest_[im]);
      if (faces_[im]) rj_dev_free(h, faces_[im]);
      if (xsects_dev_[im]) rj_dev_free(h, xsects_dev_[im]);
    }
  }
  void Init() {  // map_overlay_lbvh.h:25-40
    rj_handle h = ctx_.handle();
    size_t n_edges = ctx_.get_map(0)->n_edges() + ctx_.get_map(1)->n_edges();
    cap_ = (size_t) (xsect_factor_ * n_edges);
    rj_check(h, rj_dev_alloc(h, 8 * (cap_ ? cap_ : 1), (void**) &pairs_), "rj_dev_alloc");
    for (int im = 0; im < 2; im++) {
      size_t np = ctx_.get_map(im)->n_points();
      rj_check(h, rj_dev_alloc(h, 4 * (np ? np : 1), (void**) &closest_[im]), "rj_dev_alloc");
      rj_check(h, rj_dev_alloc(h, 4 * (np ? np : 1), (void**) &faces_[im]), "rj_dev_alloc");
    }
  }
  void BuildIndex() {  // :42-58: an LBVH over each map (grid mode: AddMapsToGrid)
    for (int im = 0; im < 2; im++) {
      if (grid_) rj_check(ctx_.handle(), rj_build_grid(ctx_.handle(), im, grid_size_), "rj_build_grid");
      else rj_check(ctx_.handle(), rj_build_lbvh(ctx_.handle(), im), "rj_build_lbvh");
    }
  }
  void IntersectEdge(int query_map_id) {  // :60-71
    uint64_t n = 0;
    int rc = grid_ ? rj_lsi_query_grid(ctx_.handle(), cap_, pairs_, &n)
                   : rj_lsi_query(ctx_.handle(), 1 - query_map_id, query_map_id, 0,
                                  ctx_.get_map(query_map_id)->n_edges(), cap_, pairs_, &n);
    rj_check(ctx_.handle(), rc, "rj_lsi_query");
    n_xsects_ = n;
    std::cerr << "Intersections: " << n << std::endl;
  }
  void LocateVerticesInOtherMap(int query_map_id) {  // :73-107
    const size_t np = ctx_.get_map(query_map_id)->n_points();
    rj_check(ctx_.handle(),
             grid_ ? rj_pip_query_grid(ctx_.handle(), 1 - query_map_id, query_map_id, nullptr, 0, np,
                                       closest_[query_map_id], faces_[query_map_id])
                   : rj_pip_query(ctx_.handle(), 1 - query_map_id, query_map_id, nullptr, 0, np,
                                  closest_[query_map_id], faces_[query_map_id]),
             "rj_pip_query");
  }
  void ComputeOutputPolygons() {  // :109-265
    rj_handle h = ctx_.handle();
    for (int im = 0; im < 2; im++) {
      rj_xsect* d = nullptr;
      rj_check(h, rj_dev_alloc(h, 48 * (n_xsects_ ? n_xsects_ : 1), (void**) &d), "rj_dev_alloc");
      int rc = rj_overlay_edge_xsects(h, im, pairs_, n_xsects_, d);
      xsects_[im].resize(n_xsects_);
      if (rc == RJ_OK) rc = rj_memcpy_d2h(h, xsects_[im].data(), d, 48 * n_xsects_);
      if (keep_xsects_) xsects_dev_[im] = d;  // (the face table and the output map read them)
      else rj_dev_free(h, d);
      rj_check(h, rc, "rj_overlay_edge_xsects");
    }
  }
  // the face table on the device (rj_overlay_faces): rows to the host, one sync for the count (and a second run only
  // when the first guess of the row count was too small)
  void ComputeFaceTable() {
    rj_handle h = ctx_.handle();
    uint64_t cap = 4 * (uint64_t) n_xsects_ + 1024, n = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
      rj_overlay_face* d = nullptr;
      rj_check(h, rj_dev_alloc(h, sizeof(rj_overlay_face) * cap, (void**) &d), "rj_dev_alloc");
      int rc = use_op_ ? rj_overlay_faces_op(h, xsects_dev_[0], xsects_dev_[1], n_xsects_, faces_[0], faces_[1], cap, d, &n, how_, by_)
                       : rj_overlay_faces(h, xsects_dev_[0], xsects_dev_[1], n_xsects_, faces_[0], faces_[1], cap, d, &n);
      if (rc == RJ_E_OVERFLOW && attempt == 0) {
        rj_dev_free(h, d);
        cap = n;
        continue;
      }
      face_rows_.resize(n);
      if (rc == RJ_OK && n) rc = rj_memcpy_d2h(h, face_rows_.data(), d, sizeof(rj_overlay_face) * n);
      rj_dev_free(h, d);
      rj_check(h, rc, "rj_overlay_faces");
      break;
    }
  }
  // one line per row: "f0 f1 area", the area in input units (area2 / 2 * rrx * rry)
  void WriteFaceTable(const char* path) const {
    FILE* fp = fopen(path, "w");
    if (!fp) throw std::runtime_error(std::string("Cannot open ") + path);
    const Scaling& sc = ctx_.get_scaling();
    const double k = 0.5 * sc.get_rrx() * sc.get_rry();
    for (const rj_overlay_face& r : face_rows_) {
      const __int128 a2 = (__int128) (((unsigned __int128) (uint64_t) r.area2_hi << 64) | r.area2_lo);
      fprintf(fp, "%d %d %.17g\n", r.face[0], r.face[1], (double) a2 * k);
    }
    fclose(fp);
  }
  // a chain map read back for its file
  struct HostMap {
    std::vector<int64_t> xy;
    std::vector<uint32_t> row;
    std::vector<int32_t> left, right;
    int Fetch(rj_handle h, const int64_t* xy_dev, const uint32_t* row_dev, const int32_t* left_dev, const int32_t* right_dev, uint64_t n_chains,
              uint64_t n_points) {
      xy.resize(2 * n_points);
      row.resize(n_chains + 1);
      left.resize(n_chains);
      right.resize(n_chains);
      int rc = rj_memcpy_d2h(h, xy.data(), xy_dev, 16 * n_points);
      if (rc == RJ_OK) rc = rj_memcpy_d2h(h, row.data(), row_dev, 4 * (n_chains + 1));
      if (rc == RJ_OK) rc = rj_memcpy_d2h(h, left.data(), left_dev, 4 * n_chains);
      if (rc == RJ_OK) rc = rj_memcpy_d2h(h, right.data(), right_dev, 4 * n_chains);
      return rc;
    }
  };
  // the output map on the device (rj_overlay_map): a sizing call, then the arrays, which stay with the caller
  struct DeviceMap {
    rj_overlay_map_counts c{};
    int64_t* xy = nullptr;
    uint32_t* row = nullptr;
    int32_t *left = nullptr, *right = nullptr, *pairs = nullptr;
  };
  DeviceMap RunOutputMap(uint32_t more_flags = 0) {
    rj_handle h = ctx_.handle();
    DeviceMap m;
    const uint32_t flags = map_flags_ | more_flags;
    auto overlay_map = [&](uint64_t cc, uint64_t pc, uint64_t fc) {
      return use_op_ ? rj_overlay_map_op(h, xsects_dev_[0], xsects_dev_[1], n_xsects_, faces_[0], faces_[1], flags, cc, pc, fc, m.xy, m.row,
                                         m.left, m.right, m.pairs, nullptr, &m.c, how_, by_)
                     : rj_overlay_map(h, xsects_dev_[0], xsects_dev_[1], n_xsects_, faces_[0], faces_[1], flags, cc, pc, fc, m.xy, m.row,
                                      m.left, m.right, m.pairs, nullptr, &m.c);
    };
    int rc = overlay_map(0, 0, 0);
    if (rc != RJ_E_OVERFLOW) rj_check(h, rc, "rj_overlay_map");
    const rj_overlay_map_counts c = m.c;
    rj_check(h, rj_dev_alloc(h, 16 * (c.n_points ? c.n_points : 1), (void**) &m.xy), "rj_dev_alloc");
    rj_check(h, rj_dev_alloc(h, 4 * (c.n_chains + 1), (void**) &m.row), "rj_dev_alloc");
    rj_check(h, rj_dev_alloc(h, 4 * (c.n_chains ? c.n_chains : 1), (void**) &m.left), "rj_dev_alloc");
    rj_check(h, rj_dev_alloc(h, 4 * (c.n_chains ? c.n_chains : 1), (void**) &m.right), "rj_dev_alloc");
    rj_check(h, rj_dev_alloc(h, 8 * (c.n_faces ? c.n_faces : 1), (void**) &m.pairs), "rj_dev_alloc");
    rc = overlay_map(c.n_chains, c.n_points, c.n_faces);
    if (rc != RJ_OK) FreeMap(m);
    rj_check(h, rc, "rj_overlay_map");
    return m;
  }
  void FreeMap(DeviceMap& m) {
    rj_handle h = ctx_.handle();
    rj_dev_free(h, m.xy); rj_dev_free(h, m.row); rj_dev_free(h, m.left); rj_dev_free(h, m.right); rj_dev_free(h, m.pairs);
  }
  // ... to the host for the file
  void ComputeOutputMap() {
    rj_handle h = ctx_.handle();
    DeviceMap m = RunOutputMap();
    const rj_overlay_map_counts c = m.c;
    const int rc = om_.Fetch(h, m.xy, m.row, m.left, m.right, c.n_chains, c.n_points);
    FreeMap(m);
    rj_check(h, rc, "rj_overlay_map");
    std::cerr << "Output map: " << c.n_chains << " chains, " << c.n_points << " points, " << c.n_faces << " faces" << std::endl;
  }
  // the output map without its degenerate pieces -> its rings, those of face 0 included (rj_map_rings) -> the map the rings
  // bound (rj_rings_map, the faces read from the ring records in place); a sizing call before each.  The output map is
  // computed again here even when -output_map has just computed it: that one may hold degenerate pieces and is already
  // freed; one more rj_overlay_map call is cheap next to reading the two input files.
  void ComputeCoarseMap() {
    rj_handle h = ctx_.handle();
    DeviceMap m = RunOutputMap(RJ_OVM_DROP_DEGENERATE);
    rj_rings_counts ring_counts{};
    rj_rings_map_counts mc{};
    rj_ring* rings = nullptr;
    uint32_t *ring_first = nullptr, *ring_half = nullptr, *ring_row = nullptr, *row = nullptr;
    int64_t *ring_xy = nullptr, *xy = nullptr;
    int32_t *left = nullptr, *right = nullptr;
    auto free_all = [&]() {
      FreeMap(m);
      rj_dev_free(h, rings); rj_dev_free(h, ring_first); rj_dev_free(h, ring_half); rj_dev_free(h, ring_row); rj_dev_free(h, ring_xy);
      rj_dev_free(h, xy); rj_dev_free(h, row); rj_dev_free(h, left); rj_dev_free(h, right);
    };
    auto must = [&](int rc, const char* what) {
      if (rc != RJ_OK) free_all();
      rj_check(h, rc, what);
    };
    int rc = rj_map_rings(h, m.xy, m.c.n_points, m.row, m.left, m.right, m.c.n_chains, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &ring_counts);
    if (rc != RJ_E_OVERFLOW) must(rc, "rj_map_rings");
    must(rj_dev_alloc(h, sizeof(rj_ring) * (ring_counts.n_rings ? ring_counts.n_rings : 1), (void**) &rings), "rj_dev_alloc");
    must(rj_dev_alloc(h, 4 * (ring_counts.n_rings + 1), (void**) &ring_first), "rj_dev_alloc");
    must(rj_dev_alloc(h, 4 * (ring_counts.n_halves ? ring_counts.n_halves : 1), (void**) &ring_half), "rj_dev_alloc");
    must(rj_dev_alloc(h, 4 * (ring_counts.n_rings + 1), (void**) &ring_row), "rj_dev_alloc");
    must(rj_dev_alloc(h, 16 * (ring_counts.n_points ? ring_counts.n_points : 1), (void**) &ring_xy), "rj_dev_alloc");
    must(rj_map_rings(h, m.xy, m.c.n_points, m.row, m.left, m.right, m.c.n_chains, 0, ring_counts.n_rings, ring_counts.n_halves, ring_counts.n_points, rings, ring_first,
                      ring_half, ring_row, ring_xy, &ring_counts),
         "rj_map_rings");
    rc = rj_rings_map(h, ring_row, ring_xy, ring_counts.n_points, rings, sizeof(rj_ring), ring_counts.n_rings, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, &mc);
    if (rc != RJ_E_OVERFLOW) must(rc, "rj_rings_map");
    must(rj_dev_alloc(h, 16 * (mc.n_points ? mc.n_points : 1), (void**) &xy), "rj_dev_alloc");
    must(rj_dev_alloc(h, 4 * (mc.n_chains + 1), (void**) &row), "rj_dev_alloc");
    must(rj_dev_alloc(h, 4 * (mc.n_chains ? mc.n_chains : 1), (void**) &left), "rj_dev_alloc");
    must(rj_dev_alloc(h, 4 * (mc.n_chains ? mc.n_chains : 1), (void**) &right), "rj_dev_alloc");
    must(rj_rings_map(h, ring_row, ring_xy, ring_counts.n_points, rings, sizeof(rj_ring), ring_counts.n_rings, 0, mc.n_chains, mc.n_points, xy, row, left, right, &mc),
         "rj_rings_map");
    must(cm_.Fetch(h, xy, row, left, right, mc.n_chains, mc.n_points), "rj_memcpy_d2h");
    const uint64_t source_chains = m.c.n_chains;
    free_all();
    std::cerr << "Coarse map: " << mc.n_chains << " chains (" << mc.n_closed << " closed), " << mc.n_points << " points of " << source_chains
              << " chains; " << mc.n_conflicts << " conflicts" << std::endl;
  }
  // the polygons of the output map on the device: the map, its rings without those of face 0, the holes to their outer
  // rings (a sizing call before each); what the file needs goes to the host
  void ComputePolygons() {
    rj_handle h = ctx_.handle();
    DeviceMap m = RunOutputMap();
    rj_rings_counts ring_counts{};
    rj_ring* rings = nullptr;
    uint32_t *ring_first = nullptr, *ring_half = nullptr, *ring_row = nullptr, *poly_first = nullptr, *poly_ring = nullptr;
    int64_t* ring_xy = nullptr;
    rj_polygon* polygons = nullptr;
    auto free_all = [&]() {
      FreeMap(m);
      rj_dev_free(h, rings); rj_dev_free(h, ring_first); rj_dev_free(h, ring_half); rj_dev_free(h, ring_row); rj_dev_free(h, ring_xy);
      rj_dev_free(h, polygons); rj_dev_free(h, poly_first); rj_dev_free(h, poly_ring);
    };
    auto must = [&](int rc, const char* what) {
      if (rc != RJ_OK) free_all();
      rj_check(h, rc, what);
    };
    int rc = rj_map_rings(h, m.xy, m.c.n_points, m.row, m.left, m.right, m.c.n_chains, RJ_RINGS_SKIP_FACE0, 0, 0, 0, nullptr, nullptr, nullptr,
                          nullptr, nullptr, &ring_counts);
    if (rc != RJ_E_OVERFLOW) must(rc, "rj_map_rings");
    must(rj_dev_alloc(h, sizeof(rj_ring) * (ring_counts.n_rings ? ring_counts.n_rings : 1), (void**) &rings), "rj_dev_alloc");
    must(rj_dev_alloc(h, 4 * (ring_counts.n_rings + 1), (void**) &ring_first), "rj_dev_alloc");
    must(rj_dev_alloc(h, 4 * (ring_counts.n_halves ? ring_counts.n_halves : 1), (void**) &ring_half), "rj_dev_alloc");
    must(rj_dev_alloc(h, 4 * (ring_counts.n_rings + 1), (void**) &ring_row), "rj_dev_alloc");
    must(rj_dev_alloc(h, 16 * (ring_counts.n_points ? ring_counts.n_points : 1), (void**) &ring_xy), "rj_dev_alloc");
    must(rj_map_rings(h, m.xy, m.c.n_points, m.row, m.left, m.right, m.c.n_chains, RJ_RINGS_SKIP_FACE0, ring_counts.n_rings, ring_counts.n_halves, ring_counts.n_points,
                      rings, ring_first, ring_half, ring_row, ring_xy, &ring_counts),
         "rj_map_rings");
    rj_polygons_counts pc{};
    rc = rj_rings_polygons(h, rings, ring_counts.n_rings, ring_row, ring_xy, ring_counts.n_points, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, &pc);
    if (rc != RJ_E_OVERFLOW) must(rc, "rj_rings_polygons");
    must(rj_dev_alloc(h, sizeof(rj_polygon) * (pc.n_polygons ? pc.n_polygons : 1), (void**) &polygons), "rj_dev_alloc");
    must(rj_dev_alloc(h, 4 * (pc.n_polygons + 1), (void**) &poly_first), "rj_dev_alloc");
    must(rj_dev_alloc(h, 4 * (pc.n_members ? pc.n_members : 1), (void**) &poly_ring), "rj_dev_alloc");
    must(rj_rings_polygons(h, rings, ring_counts.n_rings, ring_row, ring_xy, ring_counts.n_points, 0, pc.n_polygons, pc.n_members, nullptr, polygons, poly_first,
                           poly_ring, &pc),
         "rj_rings_polygons");
    pg_polygons_.resize(pc.n_polygons);
    pg_first_.resize(pc.n_polygons + 1);
    pg_ring_.resize(pc.n_members);
    pg_row_.resize(ring_counts.n_rings + 1);
    pg_xy_.resize(2 * ring_counts.n_points);
    pg_pairs_.resize(2 * m.c.n_faces);
    must(rj_memcpy_d2h(h, pg_polygons_.data(), polygons, sizeof(rj_polygon) * pc.n_polygons), "rj_memcpy_d2h");
    must(rj_memcpy_d2h(h, pg_first_.data(), poly_first, 4 * (pc.n_polygons + 1)), "rj_memcpy_d2h");
    must(rj_memcpy_d2h(h, pg_ring_.data(), poly_ring, 4 * pc.n_members), "rj_memcpy_d2h");
    must(rj_memcpy_d2h(h, pg_row_.data(), ring_row, 4 * (ring_counts.n_rings + 1)), "rj_memcpy_d2h");
    must(rj_memcpy_d2h(h, pg_xy_.data(), ring_xy, 16 * ring_counts.n_points), "rj_memcpy_d2h");
    must(rj_memcpy_d2h(h, pg_pairs_.data(), m.pairs, 8 * m.c.n_faces), "rj_memcpy_d2h");
    free_all();
    std::cerr << "Polygons: " << pc.n_polygons << " polygons, " << pc.n_holes << " holes, " << pc.n_orphans << " orphans of " << ring_counts.n_rings
              << " rings" << std::endl;
  }
  // one line per polygon: "f0 f1 area2 POLYGON ((shell), (hole), ...)"
  void WritePolygons(const char* path) const {
    FILE* fp = fopen(path, "w");
    if (!fp) throw std::runtime_error(std::string("Cannot open ") + path);
    const Scaling& sc = ctx_.get_scaling();
    for (size_t k = 0; k < pg_polygons_.size(); k++) {
      const rj_polygon& g = pg_polygons_[k];
      const bool known = g.face >= 1 && 2 * (size_t) g.face <= pg_pairs_.size();
      unsigned __int128 a2 = ((unsigned __int128) (uint64_t) g.area2_hi << 64) | g.area2_lo;
      const bool negative = g.area2_hi < 0;
      if (negative) a2 = (unsigned __int128) 0 - a2;
      char digits[48];
      int nd = 0;
      do {
        digits[nd++] = (char) ('0' + (int) (a2 % 10));
        a2 /= 10;
      } while (a2);
      std::string area(negative ? "-" : "");
      while (nd) area.push_back(digits[--nd]);
      fprintf(fp, "%d %d %s POLYGON (", known ? pg_pairs_[2 * (size_t) (g.face - 1)] : g.face, known ? pg_pairs_[2 * (size_t) (g.face - 1) + 1] : 0,
              area.c_str());
      for (uint32_t j = pg_first_[k]; j < pg_first_[k + 1]; j++) {
        const uint32_t r = pg_ring_[j], b = pg_row_[r], e = pg_row_[r + 1];
        fputs(j == pg_first_[k] ? "(" : ", (", fp);
        for (uint32_t p = b; p <= e; p++) {  // (closed: the first point again at the end)
          const size_t q = p == e ? b : p;
          fprintf(fp, "%s%.6f %.6f", p == b ? "" : ", ", sc.UnscaleX(pg_xy_[2 * q]), sc.UnscaleY(pg_xy_[2 * q + 1]));
        }
        fputs(")", fp);
      }
      fputs(")\n", fp);
    }
    fclose(fp);
  }
  void WriteOutputMapFile(const char* path) const { WriteMapFile(path, om_); }
  void WriteCoarseMapFile(const char* path) const { WriteMapFile(path, cm_); }
  // a device map as a CDB file: "id points first last left right", then the points
  void WriteMapFile(const char* path, const HostMap& hm) const {
    FILE* fp = fopen(path, "w");
    if (!fp) throw std::runtime_error(std::string("Cannot open ") + path);
    const Scaling& sc = ctx_.get_scaling();
    struct Hash {
      size_t operator()(const std::pair<int64_t, int64_t>& p) const {
        return (size_t) (((uint64_t) p.first * 0x9E3779B97F4A7C15ull) ^ ((uint64_t) p.second + ((uint64_t) p.first >> 29)));
      }
    };
    std::unordered_map<std::pair<int64_t, int64_t>, uint32_t, Hash> ids;
    auto id_of = [&](uint32_t p) {
      return ids.emplace(std::make_pair(hm.xy[2 * (size_t) p], hm.xy[2 * (size_t) p + 1]), (uint32_t) ids.size()).first->second;
    };
    for (size_t i = 0; i + 1 < hm.row.size(); i++) {
      const uint32_t b = hm.row[i], e = hm.row[i + 1];
      const uint32_t first = id_of(b), last = id_of(e - 1);
      fprintf(fp, "%zu %u %u %u %d %d\n", i + 1, e - b, first, last, hm.left[i], hm.right[i]);
      for (uint32_t p = b; p < e; p++) fprintf(fp, "%.6f %.6f\n", sc.UnscaleX(hm.xy[2 * (size_t) p]), sc.UnscaleY(hm.xy[2 * (size_t) p + 1]));
    }
    fclose(fp);
  }
  void WriteResult(const char* path) {  // :267-270
    std::vector<int32_t> pip[2];
    for (int im = 0; im < 2; im++) {
      pip[im].resize(ctx_.get_map(im)->n_points());
      rj_check(ctx_.handle(), rj_memcpy_d2h(ctx_.handle(), pip[im].data(), faces_[im], 4 * pip[im].size()), "rj_memcpy_d2h");
    }
    WriteOutputChain(ctx_, xsects_, pip, path);
  }
  // CheckResult (run_overlay.cu:18-141): the same stages through -mode=grid must give the same
  // intersections and the same located edges.  Runs the device-side grid next to the LBVH results.
  bool CheckAgainstGrid(int grid_size) {
    rj_handle h = ctx_.handle();
    bool ok = true;
    for (int im = 0; im < 2; im++) rj_check(h, rj_build_grid(h, im, grid_size), "rj_build_grid");
    uint32_t* p2 = nullptr;
    rj_check(h, rj_dev_alloc(h, 8 * (cap_ ? cap_ : 1), (void**) &p2), "rj_dev_alloc");
    uint64_t n2 = 0;
    int rc = rj_lsi_query_grid(h, cap_, p2, &n2);
    ok = rc == RJ_OK && n2 == n_xsects_;
    if (ok) {
      std::vector<uint32_t> a(2 * n2), b(2 * n2);
      rj_sort_pairs(h, p2, n2);
      rj_sort_pairs(h, pairs_, n_xsects_);
      rj_memcpy_d2h(h, a.data(), p2, 8 * n2);
      rj_memcpy_d2h(h, b.data(), pairs_, 8 * n2);
      ok = a == b;
    }
    rj_dev_free(h, p2);
    std::cerr << (ok ? "LSI passed check" : "LSI check FAILED") << std::endl;
    for (int im = 0; im < 2 && ok; im++) {
      const size_t np = ctx_.get_map(im)->n_points();
      uint32_t* c2 = nullptr;
      rj_check(h, rj_dev_alloc(h, 4 * (np ? np : 1), (void**) &c2), "rj_dev_alloc");
      rc = rj_pip_query_grid(h, 1 - im, im, nullptr, 0, np, c2, nullptr);
      std::vector<uint32_t> a(np), b(np);
      rj_memcpy_d2h(h, a.data(), c2, 4 * np);
      rj_memcpy_d2h(h, b.data(), closest_[im], 4 * np);
      rj_dev_free(h, c2);
      ok = rc == RJ_OK && a == b;
      std::cerr << "Map " << im << (ok ? ": PIP passed check" : ": PIP check FAILED") << std::endl;
    }
    return ok;
  }

 private:
  Context& ctx_;
  double xsect_factor_;
  bool grid_;
  int grid_size_;
  bool keep_xsects_;
  bool use_op_ = false;
  uint32_t how_ = 0, by_ = 0, map_flags_ = 0;
  size_t cap_ = 0, n_xsects_ = 0;
  rj_xsect* xsects_dev_[2] = {nullptr, nullptr};
  std::vector<rj_overlay_face> face_rows_;
  HostMap om_, cm_;  // the device output map on the host (-output_map), and the map of its rings (-coarse_map)
  std::vector<rj_polygon> pg_polygons_;  // the polygons on the host (-polygons), with the rings' points and the map's face pairs
  std::vector<uint32_t> pg_first_, pg_ring_, pg_row_;
  std::vector<int64_t> pg_xy_;
  std::vector<int32_t> pg_pairs_;
  uint32_t* pairs_ = nullptr;
  uint32_t* closest_[2] = {nullptr, nullptr};
  int32_t* faces_[2] = {nullptr, nullptr};
  std::vector<rj_xsect> xsects_[2];
};

void RunOverlay(const Flags& f) {  // run_overlay.cu:143-228
  PhaseTimer tm;
  tm.start();
  tm.next("Read map 0");
  auto g1 = load_from(f.poly1, f.serialize, f.v);
  tm.next("Read map 1");
  auto g2 = load_from(f.poly2, f.serialize, f.v);
  tm.next("Create App");
  Context ctx({g1, g2}, f.device, f.scale_fma);
  MapOverlayLBVH overlay(ctx, f.xsect_factor, f.mode == "grid", f.grid_size, !f.face_table.empty() || !f.output_map.empty() || !f.polygons.empty() || !f.coarse_map.empty());
  overlay.SetOperation(f.how, f.by);
  overlay.SetMerge(f.merge);
  tm.next("Load Data");
  ctx.LoadToDevice();
  tm.next("Init");
  overlay.Init();
  tm.next("Build Index");
  overlay.BuildIndex();
  tm.next("Intersection edges");
  overlay.IntersectEdge(0);
  for (int im = 0; im < 2; im++) {
    tm.next("Map " + std::to_string(im) + ": Locate vertices in other map");
    overlay.LocateVerticesInOtherMap(im);
  }
  tm.next("Computer output polygons");
  overlay.ComputeOutputPolygons();
  if (!f.face_table.empty()) {
    tm.next("Compute face table");
    overlay.ComputeFaceTable();
  }
  if (!f.output_map.empty()) {
    tm.next("Compute output map");
    overlay.ComputeOutputMap();
  }
  if (!f.polygons.empty()) {
    tm.next("Compute polygons");
    overlay.ComputePolygons();
  }
  if (!f.coarse_map.empty()) {
    tm.next("Compute coarse map");
    overlay.ComputeCoarseMap();
  }
  if (f.check && f.mode != "grid") {  // run_overlay.cu:199-204: compare with -mode=grid
    tm.next("Check result");
    if (!overlay.CheckAgainstGrid(f.grid_size)) throw std::runtime_error("result differs from -mode=grid");
  }
  if (!f.output.empty()) {
    tm.next("Write to file");
    overlay.WriteResult(f.output.c_str());
  }
  if (!f.face_table.empty()) {
    tm.next("Write face table");
    overlay.WriteFaceTable(f.face_table.c_str());
  }
  if (!f.output_map.empty()) {
    tm.next("Write output map");
    overlay.WriteOutputMapFile(f.output_map.c_str());
  }
  if (!f.polygons.empty()) {
    tm.next("Write polygons");
    overlay.WritePolygons(f.polygons.c_str());
  }
  if (!f.coarse_map.empty()) {
    tm.next("Write coarse map");
    overlay.WriteCoarseMapFile(f.coarse_map.c_str());
  }
  tm.end();
}

}  // namespace

int main(int argc, char* argv[]) {
  if (argc == 1) {
    std::cerr << "Usage: " << argv[0] << " -poly1 <map0.cdb> -poly2 <map1.cdb> -mode lbvh|grid [-grid_size 2048] [-output <result.cdb>]\n"
              << "  [-serialize <dir>] [-xsect_factor 0.2] [-check] [-device 0] [-v 1]\n"
              << "  [-face_table <rows.txt>] [-output_map <map.cdb>] [-how intersection|union|difference|symmetric_difference|identity]\n"
              << "  [-by pair|map0|map1] [-merge] [-polygons <polygons.txt>] [-coarse_map <map.cdb>]\n";
    return 1;
  }
  Flags f;
  try {
    f.Parse(argc, argv);
    if (f.poly1.empty() || f.poly2.empty()) throw std::invalid_argument("-poly1 and -poly2 are required");
    if (f.mode == "rt") throw std::runtime_error("-mode=rt needs RT cores/OptiX; MI355X (gfx950) has none: use -mode=lbvh");
    if (f.mode != "lbvh" && f.mode != "grid") throw std::runtime_error("Illegal mode: " + f.mode);
    RunOverlay(f);
  } catch (const std::invalid_argument& e) {
    std::cerr << "ERROR: " << e.what() << std::endl;
    return 2;
  } catch (const std::exception& e) {
    std::cerr << "FATAL: " << e.what() << std::endl;
    return 3;
  }
  return 0;
}
