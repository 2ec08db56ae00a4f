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
  // the output map on the device (rj_overlay_map): a sizing call, then the arrays; to the host for the file
  void ComputeOutputMap() {
    rj_handle h = ctx_.handle();
    rj_overlay_map_counts c;
    auto overlay_map = [&](uint64_t cc, uint64_t pc, uint64_t fc, int64_t* xy, uint32_t* row, int32_t* left, int32_t* right,
                           int32_t* pairs) {
      return use_op_ ? rj_overlay_map_op(h, xsects_dev_[0], xsects_dev_[1], n_xsects_, faces_[0], faces_[1], map_flags_, cc, pc, fc, xy, row,
                                         left, right, pairs, nullptr, &c, how_, by_)
                     : rj_overlay_map(h, xsects_dev_[0], xsects_dev_[1], n_xsects_, faces_[0], faces_[1], map_flags_, cc, pc, fc, xy, row, left,
                                      right, pairs, nullptr, &c);
    };
    int rc = overlay_map(0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc != RJ_E_OVERFLOW) rj_check(h, rc, "rj_overlay_map");
    int64_t* xy = nullptr;
    uint32_t* row = nullptr;
    int32_t *left = nullptr, *right = nullptr, *pairs = nullptr;
    rj_check(h, rj_dev_alloc(h, 16 * (c.n_points ? c.n_points : 1), (void**) &xy), "rj_dev_alloc");
    rj_check(h, rj_dev_alloc(h, 4 * (c.n_chains + 1), (void**) &row), "rj_dev_alloc");
    rj_check(h, rj_dev_alloc(h, 4 * (c.n_chains ? c.n_chains : 1), (void**) &left), "rj_dev_alloc");
    rj_check(h, rj_dev_alloc(h, 4 * (c.n_chains ? c.n_chains : 1), (void**) &right), "rj_dev_alloc");
    rj_check(h, rj_dev_alloc(h, 8 * (c.n_faces ? c.n_faces : 1), (void**) &pairs), "rj_dev_alloc");
    rc = overlay_map(c.n_chains, c.n_points, c.n_faces, xy, row, left, right, pairs);
    om_xy_.resize(2 * c.n_points);
    om_row_.resize(c.n_chains + 1);
    om_left_.resize(c.n_chains);
    om_right_.resize(c.n_chains);
    if (rc == RJ_OK) rc = rj_memcpy_d2h(h, om_xy_.data(), xy, 16 * c.n_points);
    if (rc == RJ_OK) rc = rj_memcpy_d2h(h, om_row_.data(), row, 4 * (c.n_chains + 1));
    if (rc == RJ_OK) rc = rj_memcpy_d2h(h, om_left_.data(), left, 4 * c.n_chains);
    if (rc == RJ_OK) rc = rj_memcpy_d2h(h, om_right_.data(), right, 4 * c.n_chains);
    rj_dev_free(h, xy); rj_dev_free(h, row); rj_dev_free(h, left); rj_dev_free(h, right); rj_dev_free(h, pairs);
    rj_check(h, rc, "rj_overlay_map");
    std::cerr << "Output map: " << c.n_chains << " chains, " << c.n_points << " points, " << c.n_faces << " faces" << std::endl;
  }
  // the device map as a CDB file: "id points first last left right", then the points
  void WriteOutputMapFile(const char* path) const {
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
      return ids.emplace(std::make_pair(om_xy_[2 * (size_t) p], om_xy_[2 * (size_t) p + 1]), (uint32_t) ids.size()).first->second;
    };
    for (size_t i = 0; i + 1 < om_row_.size(); i++) {
      const uint32_t b = om_row_[i], e = om_row_[i + 1];
      const uint32_t first = id_of(b), last = id_of(e - 1);
      fprintf(fp, "%zu %u %u %u %d %d\n", i + 1, e - b, first, last, om_left_[i], om_right_[i]);
      for (uint32_t p = b; p < e; p++) fprintf(fp, "%.6f %.6f\n", sc.UnscaleX(om_xy_[2 * (size_t) p]), sc.UnscaleY(om_xy_[2 * (size_t) p + 1]));
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
  std::vector<int64_t> om_xy_;  // the device output map on the host (-output_map)
  std::vector<uint32_t> om_row_;
  std::vector<int32_t> om_left_, om_right_;
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
  MapOverlayLBVH overlay(ctx, f.xsect_factor, f.mode == "grid", f.grid_size, !f.face_table.empty() || !f.output_map.empty());
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
  tm.end();
}

}  // namespace

int main(int argc, char* argv[]) {
  if (argc == 1) {
    std::cerr << "Usage: " << argv[0] << " -poly1 <map0.cdb> -poly2 <map1.cdb> -mode lbvh|grid [-grid_size 2048] [-output <result.cdb>]\n"
              << "  [-serialize <dir>] [-xsect_factor 0.2] [-check] [-device 0] [-v 1]\n"
              << "  [-face_table <rows.txt>] [-output_map <map.cdb>] [-how intersection|union|difference|symmetric_difference|identity]\n"
              << "  [-by pair|map0|map1] [-merge]\n";
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
