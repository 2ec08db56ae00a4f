/*
 * rayjoin_amd.h -- C ABI of the MI355X-native LSI / PIP query path (librayjoin_amd.so).
 *
 * The reference (pwrliang/RayJoin @ /root/reference) has no FFI layer: its seam is C++ virtual
 * dispatch chosen by the -mode string -- LSI<CONTEXT_T>::{Init,Query,get_xsects,CopyTo}
 * (src/app/lsi.h:8-43), PIP<CONTEXT_T>::{Init,Query,get_closest_eids} (src/app/pip.h:9-38),
 * with the per-mode index handed over through QueryConfigLBVH (src/app/query_config.h:24-28) and
 * built in RunLSIQuery/RunPIPQuery (src/run_query.cu:273-290,422-438).  A "-mode=lbvh" drop-in
 * therefore needs exactly the entry points below; INTEGRATION.md shows the LSILBVH/PIPLBVH
 * subclasses a maintainer would write on top of them.
 *
 * Conventions
 *   - every function returns an rj_status (0 = ok) and never throws or aborts;
 *     rj_last_error_string() describes the last failure on that handle;
 *   - one handle per device; a handle is not thread-safe, different handles may be used from
 *     different threads (the reference is single-threaded with one stream, src/context.h:119);
 *   - plain pointers and sizes only; "_dev" pointers are device memory owned by the CALLER
 *     (hipMalloc / rj_dev_alloc / a torch tensor's data_ptr), all others are host memory;
 *   - coordinates are the reference's scaled integers: int64 in [-2^46, 2^46) produced on the
 *     host by Scaling (src/map/scaling.h:79-93); the library never sees floating-point input;
 *   - queries are synchronous like the reference's (Query ends with stream.Sync(),
 *     src/app/lsi_lbvh.h:89, src/app/pip_lbvh.h:136) unless the _async form is used.
 */
#ifndef RAYJOIN_AMD_H
#define RAYJOIN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rj_handle_s* rj_handle;

typedef enum {
  RJ_OK = 0,
  RJ_E_INVALID = 1,   /* bad argument / call order (e.g. query before rj_build_lbvh) */
  RJ_E_HIP = 2,       /* a HIP runtime call failed; see rj_last_error_string */
  RJ_E_OVERFLOW = 3,  /* result queue capacity exceeded; *n_found holds the true count.
                         (The reference only asserts here: src/util/queue.h:37.) */
  RJ_E_NOMEM = 4,
  RJ_E_INTERNAL = 5   /* a traversal stack of the query kernels overflowed: results incomplete.  The
                         stacks cover the worst case of every index rj_build_lbvh accepts, so this is
                         a defect report, not an input error.  (The reference: a fixed 64-entry stack
                         per thread, unchecked -- deps/lbvh/lbvh/query.cuh:16.)  Reported by the call
                         that synchronises: rj_lsi_query(_finish), rj_pip_query, rj_sync. */
} rj_status;

#define RJ_MISS_EID 0xFFFFFFFFu /* static_cast<index_t>(DONTKNOW), src/app/pip_lbvh.h:44 */
#define RJ_EXTERIOR_FACE_ID 0   /* src/config.h:8 */

/* dev::Intersection<int64_t> as the reference's queue stores it (src/algo/lsi.h:10-26):
 * two rational<int64_t> (denominators are always 1 after the narrowing store,
 * src/util/rational.h:84-85,190-192), eid[2] = (map-0 edge, map-1 edge), 48 bytes. */
typedef struct {
  int64_t x_num, x_den;
  int64_t y_num, y_den;
  uint32_t eid[2];
  int32_t mid_point_polygon_id; /* DONTKNOW (-1) */
  int32_t _pad;
} rj_xsect;

/* ---- lifetime ------------------------------------------------------------------------- */
/* replaces: Context() + Stream (src/context.h:31-74,119; src/util/stream.h:13-27) */
int rj_create(int device_id, rj_handle* out);
int rj_destroy(rj_handle h);
/* run all work of this handle on a caller-owned hipStream_t; NULL is HIP's null (legacy default)
 * stream.  A new handle uses a private non-blocking stream (rj_set_option(h,"own_stream",1)
 * returns to it).  Queries on one stream are ordered by the stream, and each query kernel prepares
 * the counters of the next, so a CHANGE of stream first drains the old one (and the handle's second
 * stream); setting the stream the handle already uses costs nothing. */
int rj_set_stream(rj_handle h, void* hip_stream);
int rj_sync(rj_handle h);
const char* rj_last_error_string(rj_handle h);
const char* rj_version(void);

/* ---- maps ----------------------------------------------------------------------------- */
/* replaces: Context::LoadToDevice -> Map::LoadFrom (src/context.h:76-88, src/map/map.h:162-233).
 * xy: np scaled points (x,y interleaved); row_index[nc+1]: first point of each chain + sentinel;
 * left/right[nc]: face ids of each chain (truncated to 32 bits like dev::Edge, map.h:45).
 * Edge eid of chain c, point p is p - c (map.h:200-203).  Host arrays are copied.
 * Both uploads also prepare the map for being the QUERY map of rj_pip_query*: its vertices quantised (8 bytes each) and
 * the extent of every 64 of them (16 bytes), which a PIP query over a range of the map's own vertices then reads
 * instead of the int64 points ("pip_last_prepared").  That is 8 np + 16 ceil(np / 64) bytes of device memory per map
 * on top of the map itself -- 245 MB for a map of 30 M vertices -- for EACH of the two map slots, whether or not the
 * map is ever the query map of a PIP query: two maps of 30 M vertices pay it twice.  When they cannot be allocated the
 * upload still succeeds and such queries read the int64 points, as they do for a caller's array. */
int rj_upload_map(rj_handle h, int map_id, const int64_t* xy, uint64_t np,
                  const uint32_t* row_index, const int64_t* left, const int64_t* right,
                  uint64_t nc);
/* extends: Map::LoadFrom -- rj_upload_map for a map that is already in device memory (an rj_overlay_map output, a map
 * another library built there).  The same contract, but xy_dev[2 np], row_index_dev[nc + 1], left_dev[nc], right_dev[nc]
 * (int32) are caller-owned device memory, copied device to device; they may be freed when the call returns.  What
 * rj_upload_map checks in host loops -- row_index starts at 0, ends at np, every chain has at least 2 points, every
 * coordinate lies in [-2^46, 2^46) -- one kernel checks here: RJ_E_INVALID with a message, and the map that was in
 * place stays.  Resets the same handle state (index, grid, cached orders of map_id). */
int rj_upload_map_dev(rj_handle h, int map_id, const int64_t* xy_dev, uint64_t np,
                      const uint32_t* row_index_dev, const int32_t* left_dev, const int32_t* right_dev,
                      uint64_t nc);
int rj_map_num_edges(rj_handle h, int map_id, uint64_t* ne);
int rj_map_num_points(rj_handle h, int map_id, uint64_t* np);
/* device pointer to the uploaded scaled points (int64 x,y pairs), owned by the handle */
int rj_map_points_dev(rj_handle h, int map_id, const int64_t** pts_dev);
/* inspection: device pointers to what the upload prepared of the map's vertices (see rj_upload_map), owned by the handle
 * and valid until the next upload of map_id: qpts[np][2] = (x + 2^46) >> 16, (y + 2^46) >> 16 of every vertex, and
 * qext[ceil(np / 64)][4] = {min x, max x, min y, 0} of those over the vertices 64 b .. 64 b + 63 that exist.  Both
 * NULL when there was no memory for them; either argument may be NULL. */
int rj_map_prepared_dev(rj_handle h, int map_id, const int32_t** qpts_dev, const int32_t** qext_dev);
/* inspection: the polyline runs rj_build_lbvh cut for this map on the device ("leaf_order" 1; the analogue of the
 * reference's RT grouping, src/rt/primitive.h:120-260) -- piece p = eids [piece_begin[p], + piece_len[p]), run r =
 * pieces [run_first[r], run_first[r + 1]).  Host arrays, any of them NULL to fetch only the counts. */
int rj_map_runs(rj_handle h, int map_id, uint32_t* piece_begin, uint32_t* piece_len, uint32_t* run_first,
                uint64_t* nruns, uint64_t* npieces);

/* replaces: Scaling(bb) + the scale pass of Map::LoadFrom (src/map/scaling.h:56-93, src/map/map.h:171-180)
 * for hosts that do not scale themselves: xy[2n] doubles -> out_xy[2n] scaled int64, bb = {min_x, min_y,
 * max_x, max_y} of BOTH maps (src/context.h:37-47).  Host code, no GPU involved.
 * fused = 0: a separate multiply and add, what scaling.h spells out and what its host build computes
 * (the arithmetic every parity test of this repository is pinned to); fused = 1: one std::fma, what
 * nvcc's default -fmad=true makes of the same expression inside the reference's device lambda -- the
 * two differ by one unit for about 0.14 % of points.  Use the same setting for both maps. */
int rj_scale_points(const double bb[4], const double* xy, uint64_t n, int64_t* out_xy, int fused);

/* ---- index ---------------------------------------------------------------------------- */
/* replaces: FillPrimitivesLBVH + lbvh::bvh::assign/construct (src/tree/primtive.h:34-57,
 * deps/lbvh/lbvh/bvh.cuh:277-481) as called at src/run_query.cu:273-290,422-438. */
int rj_build_lbvh(rj_handle h, int base_map_id);

/* ---- LSI ------------------------------------------------------------------------------ */
/* replaces: LSILBVH::Query (src/app/lsi_lbvh.h:27-98) + Queue::Clear/size (src/util/queue.h).
 * Intersects query-map edges [query_eid_begin, query_eid_end) with all edges of the base map.
 * Writes (eid of map 0, eid of map 1) pairs, unordered, into pairs_dev[2*capacity].
 * The predicate is always evaluated as intersect_test(e1 = map-0 edge, e2 = map-1 edge)
 * whichever side is indexed, which is -mode=grid's operand order (src/app/lsi_grid.h:103-104). */
int rj_lsi_query(rj_handle h, int base_map_id, int query_map_id, uint64_t query_eid_begin,
                 uint64_t query_eid_end, uint64_t capacity, uint32_t* pairs_dev,
                 uint64_t* n_found);
/* same without the final count read-back/sync; pair with rj_lsi_query_finish */
int rj_lsi_query_async(rj_handle h, int base_map_id, int query_map_id, uint64_t query_eid_begin,
                       uint64_t query_eid_end, uint64_t capacity, uint32_t* pairs_dev);
int rj_lsi_query_finish(rj_handle h, uint64_t capacity, uint64_t* n_found);
/* Device-side Queue::size (src/util/queue.h:125-129 reads the tail counter back to the host):
 * enqueue, on the handle's stream, a copy of the last rj_lsi_query_async's result count (the TRUE
 * count, which exceeds the capacity after an overflow) into n_found_dev[0] (device memory, 8 bytes).
 * A multi-GPU caller puts it at the head of its exchange buffer and ships count + pairs in one
 * collective with no host round trip between the LSI kernel and the exchange. */
int rj_lsi_count_to(rj_handle h, uint64_t* n_found_dev);
/* The count of the last rj_lsi_query_async read back behind an event instead of a stream sync (two slots): a caller
 * that pipelines steps launches step k + 1 -- into other buffers -- before it looks at step k's count, so the GPU
 * never idles while the host wakes up.  rj_lsi_count_wait: *n_found, RJ_E_OVERFLOW / RJ_E_INTERNAL as
 * rj_lsi_query_finish; it waits for that query (and whatever was enqueued before rj_lsi_count_async) only. */
int rj_lsi_count_async(rj_handle h, int slot);
int rj_lsi_count_wait(rj_handle h, int slot, uint64_t capacity, uint64_t* n_found);

/* replaces: the intersection-point half of dev::intersect_test + the narrowing store into
 * Intersection<int64_t> (src/algo/lsi.h:107-143, src/app/lsi_lbvh.h:71-78).
 * pairs_dev: n (eid map 0, eid map 1) pairs; out_dev: n rj_xsect records. */
int rj_lsi_points(rj_handle h, const uint32_t* pairs_dev, uint64_t n, rj_xsect* out_dev);
/* The same for the result of the last rj_lsi_query_async, enqueued behind it on the handle's stream:
 * the number of records is read on the device from the queue's counter (min(count, capacity)), so
 * that "Query" leaves complete 48-byte records like the reference's (src/app/lsi_lbvh.h:71-78)
 * without a host round trip between the two kernels.  pairs_dev / capacity: what the query was given;
 * out_dev[capacity].  Complete after rj_lsi_query_finish / rj_sync. */
int rj_lsi_points_async(rj_handle h, const uint32_t* pairs_dev, uint64_t capacity, rj_xsect* out_dev);

/* sort n pairs in place by (eid0, eid1) -- the canonical order of the reference's checker
 * (src/run_overlay.cu:38-52) */
int rj_sort_pairs(rj_handle h, uint32_t* pairs_dev, uint64_t n);

/* ---- PIP ------------------------------------------------------------------------------ */
/* replaces: PIPLBVH::Query (src/app/pip_lbvh.h:25-142) and the get_face_id transform
 * (src/map/map.h:79-87, src/app/map_overlay_lbvh.h:96-104).
 * pts_dev: n scaled query points, or NULL to use points [pt_begin, pt_begin+n) of the query map
 * (RunPIPQuery queries every vertex of map 1, src/run_query.cu:346).
 * closest_eid_dev[n]: eid of the lowest base-map edge above each point, RJ_MISS_EID when none.
 * face_id_dev[n] (nullable): face below that edge, RJ_EXTERIOR_FACE_ID on a miss. */
int rj_pip_query(rj_handle h, int base_map_id, int query_map_id, const int64_t* pts_dev,
                 uint64_t pt_begin, uint64_t n, uint32_t* closest_eid_dev, int32_t* face_id_dev);
int rj_pip_query_async(rj_handle h, int base_map_id, int query_map_id, const int64_t* pts_dev,
                       uint64_t pt_begin, uint64_t n, uint32_t* closest_eid_dev,
                       int32_t* face_id_dev);
/* Caller-owned point arrays (pts_dev != NULL -- the reference's PIP::Query(Stream&, int, ArrayView<point_t>),
 * src/app/pip.h:23, handed a separate device vector by src/run_query.cu:346,441-443): the handle remembers, per
 * (pointer, n), whether the array needs re-ordering along the Morton curve and the permutation if so.  The first
 * query over an array pays one host round trip for the estimate; every later one is enqueued without any
 * synchronisation, pairs with an LSI query in flight exactly like a map-owned range, and refreshes the estimate
 * with a one-block kernel behind its own kernels, so contents that change are followed one query late.  None of
 * it can affect results (any permutation of [0, n) is a valid processing order).  rj_invalidate forgets what was
 * learned, e.g. before a buffer is reused for unrelated points. */
int rj_invalidate(rj_handle h);

/* ---- -mode=grid on the device (the reference's third index, for the grid / lbvh / rt comparison)
 * replaces: UniformGrid::AddMapsToGrid / AddMapToGrid (src/grid/uniform_grid.h:132-349): one CSR per
 * map over grid_size x grid_size cells of the scaled domain (calculate_cell, src/grid/cell.h:16-22);
 * inside a cell the eids are ascending.  Costs one entry per (cell, edge) incidence; fails with
 * RJ_E_INVALID when those exceed 2^32 (grid too fine for the map's longest edges). */
int rj_build_grid(rj_handle h, int map_id, int grid_size);
/* replaces: LSIGrid::Query + intersect_one_cell (src/app/lsi_grid.h:19-131): needs the grids of BOTH
 * maps at the same grid_size; every cell tests its (map-0 edge, map-1 edge) pairs and reports a hit
 * only from the cell that contains the computed intersection point.  Output and overflow behaviour
 * as rj_lsi_query. */
int rj_lsi_query_grid(rj_handle h, uint64_t capacity, uint32_t* pairs_dev, uint64_t* n_found);
/* replaces: PIPGrid::Query (src/app/pip_grid.h:37-70, cell acceptance src/algo/pip.h:98-114): needs
 * the grid of the base map.  Arguments and outputs as rj_pip_query. */
int rj_pip_query_grid(rj_handle h, int base_map_id, int query_map_id, const int64_t* pts_dev,
                      uint64_t pt_begin, uint64_t n, uint32_t* closest_eid_dev, int32_t* face_id_dev);

/* ---- multi-GPU: RCCL over xGMI ---------------------------------------------------------- */
/* New design (the reference is single-GPU: no NCCL/MPI anywhere).  One process and
 * one handle per GPU; the query map is sharded by chain range (rj_lsi_query's eid range / the point
 * range of rj_pip_query), the base map + LBVH are replicated, and the result queues are exchanged
 * with an all-gather-v.  Every exchange below is made of ncclAllGather alone and takes no
 * rank-dependent branch between two collectives: what a rank does next is a function of the
 * gathered words, which are the same everywhere.
 * rj_comm_unique_id: call on ONE rank, hand the 128 bytes to the others out of band (file, env,
 * MPI, torch.distributed store ...).  rj_comm_init is collective (it makes two communicators: pair
 * queues and point queues travel on streams of their own and never wait for each other). */
#define RJ_COMM_ID_BYTES 128
int rj_comm_unique_id(uint8_t id[RJ_COMM_ID_BYTES]);
int rj_comm_init(rj_handle h, int nranks, int rank, const uint8_t id[RJ_COMM_ID_BYTES]);
int rj_comm_destroy(rj_handle h);

/* The exchange of a STEP, off the critical path (bench.py, query_exec -nranks).  rj_exchange_init registers one or two
 * CALLER-OWNED exchange buffers of RJ_EXCHANGE_HEAD_WORDS + 2 * capacity 32-bit words each (buf1_dev nullable; every rank
 * must pass the same capacity and slot): the handle keeps a head in front -- count (u64), capacity (u64) -- and the
 * caller hands bufK_dev + RJ_EXCHANGE_HEAD_WORDS to rj_lsi_query_async as pairs_dev.  Per step:
 *   rj_lsi_query_async(h, ..., capacity, bufK_dev + RJ_EXCHANGE_HEAD_WORDS);
 *   rj_exchange_pairs_begin(h, K);        the device-side count goes into the buffer's head and ONE ncclAllGather of
 *                                         head + `slot` pairs per rank starts on the communication stream behind an
 *                                         event: no host round trip between the LSI kernel and the collective
 *   ... rj_lsi_points_async, rj_pip_query_async, the next step into the other buffer ...
 *   rj_exchange_pairs_finish(h, K, counts, slices, &total);   the step's one host sync on the LSI side: counts_out
 *                                         [nranks] (host), slices_dev[nranks] = device pointers to every rank's pairs
 *                                         (handle-owned, valid until the buffer's next begin), *n_total = sum.
 * `slot` (pairs shipped per rank) follows twice the largest count seen; a step in which some rank found more is gathered
 * again with a larger slot -- by every rank, which all see the same counts.  RJ_E_OVERFLOW, on EVERY rank, when some
 * rank's queue overflowed its capacity. */
#define RJ_EXCHANGE_HEAD_WORDS 4
int rj_exchange_init(rj_handle h, uint64_t capacity, uint64_t slot, uint32_t* buf0_dev, uint32_t* buf1_dev);
int rj_exchange_pairs_begin(rj_handle h, int buf);
int rj_exchange_pairs_finish(rj_handle h, int buf, uint64_t* counts_out, const uint32_t** slices_dev, uint64_t* n_total);
/* The PIP result queues of contiguous point shards: every rank ships n_per_rank words (its shard, padded: the same
 * n on every rank), recv_dev[nranks * n_per_rank].  Starts behind everything enqueued so far on the handle's streams, on
 * the second communicator's stream; rj_exchange_u32_finish waits for it. */
int rj_exchange_u32_begin(rj_handle h, const uint32_t* src_dev, uint64_t n_per_rank, uint32_t* recv_dev);
int rj_exchange_u32_finish(rj_handle h);
/* what every rank concludes from the gathered (count, capacity) words -- a pure host function (no GPU, no
 * communicator), so that the branch after a collective can be tested without one: RJ_E_OVERFLOW when some rank's count
 * exceeds its capacity (*first_bad = the lowest such rank, else -1), *max_count = the largest count. */
int rj_exchange_verdict(const uint64_t* counts, const uint64_t* capacities, int nranks, uint64_t* max_count, int* first_bad);

/* Synchronous all-gather-v with exact, contiguous output (hosts that want one flat queue).
 * pairs_dev: this rank's n_local (eid0, eid1) pairs; out_dev[2 * out_capacity]: all ranks' pairs in
 * rank order; counts_out[nranks] (host, nullable); *n_total = sum.  Two collectives: (count, capacity) of every rank,
 * then every slice padded to the largest.  RJ_E_OVERFLOW (with *n_total set) on EVERY rank when the total exceeds the
 * SMALLEST out_capacity any rank passed -- no rank enters the second collective alone. */
int rj_allgather_pairs(rj_handle h, const uint32_t* pairs_dev, uint64_t n_local, uint32_t* out_dev,
                       uint64_t out_capacity, uint64_t* counts_out, uint64_t* n_total);
/* The layout of an all-gather-v, as a pure host function (no GPU, no communicator; what rj_allgather_* compute
 * between their two collectives): offsets[r] = counts[0] + ... + counts[r-1] (rank r's slice starts there, zero
 * counts take no room), *total = the sum.  RJ_E_OVERFLOW (offsets and *total still set) when total > capacity,
 * RJ_E_INVALID for nranks < 1, null arrays or a sum that does not fit 64 bits. */
int rj_allgatherv_plan(const uint64_t* counts, int nranks, uint64_t capacity, uint64_t* offsets, uint64_t* total);
/* same for a queue of 32-bit values (closest eids / face ids of a point shard) */
int rj_allgather_u32(rj_handle h, const uint32_t* src_dev, uint64_t n_local, uint32_t* out_dev,
                     uint64_t out_capacity, uint64_t* counts_out, uint64_t* n_total);

/* ---- overlay support ------------------------------------------------------------------- */
/* replaces: the per-map body of MapOverlayLBVH::ComputeOutputPolygons
 * (src/app/map_overlay_lbvh.h:109-265).  For map `im`: the n intersections (eid map 0, eid map 1)
 * become 48-byte records ordered by eid[im] and, on one edge, by squared distance of the stored
 * point from that edge's first endpoint (:204-213; the reference's unstable ties are resolved by
 * the other map's eid); the mid-point of each consecutive pair on an edge (:215-227) is located
 * in the other map (query map id = im, :232-236) and the face found is stored in the FIRST record
 * of the pair (mid_point_polygon_id, :238-262); the last record of an edge keeps DONTKNOW (-1).
 * Needs rj_build_lbvh(1 - im).  xsects_dev[n] is caller-owned device memory. */
int rj_overlay_edge_xsects(rj_handle h, int im, const uint32_t* pairs_dev, uint64_t n,
                           rj_xsect* xsects_dev);

/* One row of the overlay's face table: a face of map 0 and a face of map 1 that overlap, and twice the signed area of
 * their overlap in scaled units^2 (exact: a two's-complement int128, value = area2_hi * 2^64 + area2_lo). */
typedef struct {
  int32_t face[2];   /* face of map 0, face of map 1; both != RJ_EXTERIOR_FACE_ID */
  uint64_t area2_lo;
  int64_t area2_hi;
} rj_overlay_face;   /* 24 bytes */

/* extends: WriteOutputChain (src/app/output_chain.h:42-205) -- what a caller of the overlay wants from the output map,
 * computed on the device instead of written as text.  The pieces are the output map's (every chain cut at its records,
 * each piece labelled with the face of the other map it lies in); every consecutive point pair a -> b of a kept piece
 * adds cross(a, b) to (the chain's left face, the piece's other face) and -cross(a, b) to (right face, other face), a
 * side with face 0 adding nothing.  Rows (face of map 0, face of map 1) with at least one contribution, ascending by
 * ((uint64)(uint32)face[0] << 32) | (uint32)face[1].  On maps in general position every area2 is positive; where the
 * maps share boundary the table inherits the output map's labels, like the CDB file.  The unordered pairs {min, max} of
 * the rows are the output map's faces (its "Total faces").  Face ids are nonnegative.
 * xsectsK_dev: the n records of rj_overlay_edge_xsects(h, K, ...) (both from the same pairs, LBVH or grid);
 * vertex_faceK_dev: face_id_dev of rj_pip_query(h, 1 - K, K, NULL, 0, np_K, ...) (or rj_pip_query_grid) -- the face in
 * the other map of every vertex of map K.  n == 0 is valid (disjoint maps, a map inside one face of the other).
 * out_dev[capacity] is caller-owned device memory; RJ_E_OVERFLOW when there are more rows: *n_faces holds the true count
 * and nothing beyond capacity is written.  One host sync, at the end, to read the count. */
int rj_overlay_faces(rj_handle h, const rj_xsect* xsects0_dev, const rj_xsect* xsects1_dev, uint64_t n,
                     const int32_t* vertex_face0_dev, const int32_t* vertex_face1_dev,
                     uint64_t capacity, rj_overlay_face* out_dev, uint64_t* n_faces);

/* rj_overlay_map flags */
#define RJ_OVM_DROP_DEGENERATE 1u /* leave out the pieces with fewer than two points, together with their points */
#define RJ_OVM_MERGE_PIECES    2u /* adjacent pieces of one source chain with equal faces that touch leave as one chain */

typedef struct {
  uint64_t n_chains, n_points, n_faces;
} rj_overlay_map_counts;

/* extends: WriteOutputChain (src/app/output_chain.h:42-205) -- the output map itself as device arrays, in scaled
 * integers, so that it can be read without parsing a file or become an input map (rj_upload_map_dev) without leaving
 * the GPU.  Inputs as rj_overlay_faces.
 *   chains  the pieces the writer keeps, in its order: map 0's pieces in chain order, then map 1's.  A piece is kept when
 *           its other-map face is nonzero and its chain has a nonzero face on at least one side.
 *   points  of a piece: head cut point (x_num, y_num of the record), the chain's vertices inside it, tail cut point;
 *           consecutive equal points once (equality of the integer coordinates; the text writer compares unscaled
 *           doubles).  xy_dev: int64 x,y pairs; piece k = points [row_index_dev[k], row_index_dev[k + 1]).
 *   faces   numbered from 1 by the ordered pair (face of map 0, face of map 1), ascending by
 *           ((uint64)(uint32)f0 << 32) | (uint32)f1; face_pairs_dev[2 (k - 1)], [2 (k - 1) + 1] is the pair of face k:
 *           row k - 1 of rj_overlay_faces on the same inputs.  left_dev / right_dev: the face on each side of a piece,
 *           0 without one.  (Not the text writer's numbering, which numbers unordered pairs in order of first use.)
 *   origin_dev[k] = (im << 31) | the chain of map im piece k was cut from; may be NULL.
 * RJ_OVM_DROP_DEGENERATE leaves out the pieces with fewer than two points (a cut on a vertex of its own chain) and their
 * points -- what rj_upload_map_dev needs; the faces and their numbers do not change with it.
 * RJ_OVM_MERGE_PIECES returns merge(M), M being the map the same call returns without the flag (so
 * RJ_OVM_DROP_DEGENERATE, when set, is applied first).  Chain k > 0 of M JOINS chain k - 1 when origin[k] == origin[k - 1],
 * left[k] == left[k - 1], right[k] == right[k - 1] and the last point of chain k - 1 equals the first point of chain k
 * (both integer coordinates).  A rule on M's arrays: two kept pieces with a dropped piece between them merge exactly when
 * they touch.  The chains of merge(M) are the maximal runs of joined chains, in M's order; a run's points are its chains'
 * points in order without the first point of every joining chain (the duplicate of the point before it); left, right,
 * origin are the run's common values; face_pairs, n_faces and the face numbers do not change; counts holds the merged
 * n_chains and n_points (also in the sizing call and with RJ_E_OVERFLOW).  Without RJ_OVM_DROP_DEGENERATE one-point
 * pieces take part by the same rule (a run of them on one point becomes a one-point chain); with both flags no chain has
 * fewer than two points.  NOT merged: the last piece of a closed source chain with its first (the seam stays a chain
 * boundary), and pieces of different source chains, whatever their faces.  Another flag bit is RJ_E_INVALID.
 * Caller-owned device memory: xy_dev[2 point_capacity], row_index_dev[chain_capacity + 1], left_dev, right_dev,
 * origin_dev[chain_capacity], face_pairs_dev[2 face_capacity].  RJ_E_OVERFLOW when a count exceeds its capacity:
 * *counts holds the three true counts and nothing beyond any capacity is written; all capacities 0 (arrays may be
 * NULL) is the sizing call.  n == 0 is valid.  The points of both maps and four per record must number fewer than 2^32
 * (row_index is 32-bit).  One host sync, at the end, to read the counts. */
int rj_overlay_map(rj_handle h, const rj_xsect* xsects0_dev, const rj_xsect* xsects1_dev, uint64_t n,
                   const int32_t* vertex_face0_dev, const int32_t* vertex_face1_dev, uint32_t flags,
                   uint64_t chain_capacity, uint64_t point_capacity, uint64_t face_capacity,
                   int64_t* xy_dev, uint32_t* row_index_dev, int32_t* left_dev, int32_t* right_dev,
                   int32_t* face_pairs_dev, uint32_t* origin_dev, rj_overlay_map_counts* counts);

/* ---- overlay operations: union, difference, symmetric difference, identity; dissolved forms (clip) ------------ */
/* extends: rj_overlay_faces / rj_overlay_map know one operation, the intersection (what the reference's CDB writer
 * keeps).  A side of a piece has the ordered pair (f0, f1) = (face of map 0, face of map 1): the chain's face on that
 * side and the piece's label.  `how` says which pairs are faces of the result: */
#define RJ_OV_INTERSECTION 0u /* f0 != 0 and f1 != 0 */
#define RJ_OV_UNION        1u /* f0 != 0 or  f1 != 0 */
#define RJ_OV_DIFFERENCE   2u /* f0 != 0 and f1 == 0: map 0 minus map 1 */
#define RJ_OV_SYMDIFF      3u /* (f0 != 0) != (f1 != 0) */
#define RJ_OV_IDENTITY     4u /* f0 != 0: all of map 0, split by map 1 */
/* `by` says what names a face: */
#define RJ_OV_BY_PAIR 0u /* (f0, f1) */
#define RJ_OV_BY_MAP0 1u /* (f0, 0): map 1's boundaries inside a face of map 0 dissolve (INTERSECTION + BY_MAP0 = clip) */
#define RJ_OV_BY_MAP1 2u /* (0, f1) */
/* A side's key is by(f0, f1) when the pair is selected and the key is not (0, 0), else "no face".  A piece is kept when
 * the keys of its two sides differ (so at least one side has a face; a piece with the same face on both sides after a
 * dissolve is dropped).  Adjacent kept pieces of one chain stay apart unless RJ_OVM_MERGE_PIECES is set.  Everything else is as the call without _op
 * documents: piece order, points, duplicate removal, faces numbered from 1 ascending by ((uint32)f0 << 32) | (uint32)f1
 * of the KEY, RJ_OVM_DROP_DEGENERATE, RJ_OVM_MERGE_PIECES, RJ_E_OVERFLOW with the true counts, the sizing call, n == 0.
 * The face table: a kept piece adds +cross per point pair to its left key and -cross to its right key; one row per key
 * with a contribution, face[] holding the key -- so a face id may be 0 here: (f0, 0) is "f0 outside map 1" under
 * BY_PAIR and "the selected part of f0" under BY_MAP0.  Under (RJ_OV_UNION, RJ_OV_BY_PAIR) the rows (f, *) sum to
 * twice the area of face f of map 0 over its cut boundary, and the rows (*, g) to that of face g of map 1.
 * (RJ_OV_INTERSECTION, RJ_OV_BY_PAIR) gives what the call without _op gives on maps whose chains have different faces
 * on their two sides (a chain with one nonzero face on both sides is kept there and dropped here).
 * An unknown `how` or `by` is RJ_E_INVALID.  Same cost class as the calls without _op: the same passes over the same
 * edges, the operation being a kernel argument. */
int rj_overlay_faces_op(rj_handle h, const rj_xsect* xsects0_dev, const rj_xsect* xsects1_dev, uint64_t n,
                        const int32_t* vertex_face0_dev, const int32_t* vertex_face1_dev,
                        uint64_t capacity, rj_overlay_face* out_dev, uint64_t* n_faces, uint32_t how, uint32_t by);
int rj_overlay_map_op(rj_handle h, const rj_xsect* xsects0_dev, const rj_xsect* xsects1_dev, uint64_t n,
                      const int32_t* vertex_face0_dev, const int32_t* vertex_face1_dev, uint32_t flags,
                      uint64_t chain_capacity, uint64_t point_capacity, uint64_t face_capacity,
                      int64_t* xy_dev, uint32_t* row_index_dev, int32_t* left_dev, int32_t* right_dev,
                      int32_t* face_pairs_dev, uint32_t* origin_dev, rj_overlay_map_counts* counts,
                      uint32_t how, uint32_t by);

/* ---- face rings -------------------------------------------------------------------------- */
/* rj_map_rings flags */
#define RJ_RINGS_SKIP_FACE0 1u /* leave out the rings whose face is 0, with their half-chains and points */
#define RJ_RINGS_NO_POINTS  2u /* ring_row_dev / ring_xy_dev are not written and point_capacity is ignored; n_points is still counted */
/* rj_ring flags */
#define RJ_RING_MIXED 1u /* some half-chain of the ring has another face than the ring's */

typedef struct {
  int32_t face;
  uint32_t flags;
  uint32_t leader;
  uint32_t _pad;
  uint64_t area2_lo; /* twice the signed area, a two's-complement int128 like rj_overlay_face's */
  int64_t area2_hi;
} rj_ring; /* 32 bytes */

typedef struct {
  uint64_t n_rings, n_halves, n_points, n_mixed, n_skipped;
} rj_rings_counts;

/* extends: the polygons of a chain map -- the closed boundaries (rings) that the chains form, computed on the device
 * from a map in caller-owned device memory with the contract of rj_upload_map_dev (an rj_overlay_map output, an input
 * map): xy_dev[2 np], row_index_dev[nc + 1], left_dev[nc], right_dev[nc]; left is the face on the left of a chain walked
 * from its first point to its last, y up (the convention under which rj_overlay_faces' areas are positive).
 * nc < 2^31, np < 2^32 and 2 (np - nc) < 2^32.  The definition, in full in rayjoin_amd/csrc/rj_rings.h:
 *   half-chain h = 2 c is chain c walked forward (face left[c]), h = 2 c + 1 chain c walked backward (face right[c]),
 *   h ^ 1 its twin; a chain whose points are all equal is skipped (n_skipped) and belongs to no ring.  Incidence h is the
 *   start vertex of h with the direction to the first different point of the chain.  The incidences on one point are
 *   ordered counter-clockwise from the positive x axis, exactly (int128 cross products), equal directions by ascending h;
 *   h arrives at the junction of h ^ 1 and goes on with the clockwise neighbour of h ^ 1 there (h ^ 1 itself at a dead
 *   end), which keeps the face on the left.  The cycles of that permutation are the rings.
 *   A ring: leader = its smallest h; face = the leader's face; RJ_RING_MIXED when a half-chain of it has another face
 *   (only where chains overlap or the map's labels are inconsistent); its half-chains in walk order from the leader; its
 *   points = every half-chain's points in its direction without the last (as many points as edges, the first point is
 *   not repeated); area2 = the sum of cross(a, b) over consecutive points including the closing pair, exact: positive
 *   for a counter-clockwise ring (the outer boundary of its face), negative for a hole of its face or a boundary of
 *   face 0.  Rings ascend by ((uint64)(uint32)face << 32) | leader: the rings of a face are contiguous.
 * Output, all caller-owned device memory: rings_dev[ring_capacity]; ring_first_dev[ring_capacity + 1], the CSR of the
 * rings into ring_half_dev[half_capacity]; ring_row_dev[ring_capacity + 1], the CSR into ring_xy_dev[2 point_capacity].
 * RJ_E_OVERFLOW when a count exceeds its capacity: *counts holds the true counts and nothing beyond any capacity is
 * written; all capacities 0 (arrays may be NULL) is the sizing call.  nc == 0 is valid.  A malformed map (the checks of
 * rj_upload_map_dev, but a chain may have a single point: an output map without RJ_OVM_DROP_DEGENERATE has such
 * chains, they are skipped) and an unknown flag bit are RJ_E_INVALID, with nothing written; RJ_E_INTERNAL when a round budget
 * runs out (33 doubling steps: cannot happen below 2^32 half-chains).  Runs on the handle's stream with one host sync, at the end, to read
 * the counts; scratch (352 bytes per chain plus the sorts' temporary storage) is allocated per call and freed; no
 * state of the handle (maps, indexes, plans) changes. */
int rj_map_rings(rj_handle h, const int64_t* xy_dev, uint64_t np, const uint32_t* row_index_dev,
                 const int32_t* left_dev, const int32_t* right_dev, uint64_t nc, uint32_t flags,
                 uint64_t ring_capacity, uint64_t half_capacity, uint64_t point_capacity,
                 rj_ring* rings_dev, uint32_t* ring_first_dev, uint32_t* ring_half_dev, uint32_t* ring_row_dev,
                 int64_t* ring_xy_dev, rj_rings_counts* counts);

/* ---- polygons ---------------------------------------------------------------------------- */
#define RJ_POLY_NONE 0xFFFFFFFFu /* parent_dev: a ring of face 0, or a hole without a shell round it (an orphan) */

typedef struct {
  int32_t face;
  uint32_t shell;   /* the ring index of its outer ring */
  uint32_t n_holes;
  uint32_t _pad;
  uint64_t area2_lo; /* twice the area: the shell's area2 plus its holes', a two's-complement int128 like rj_ring's */
  int64_t area2_hi;
} rj_polygon; /* 32 bytes */

typedef struct {
  uint64_t n_polygons, n_members, n_holes, n_orphans, n_face0;
} rj_polygons_counts;

/* extends: the polygons of the rings that rj_map_rings gave (with points; rings_dev, ring_row_dev, ring_xy_dev as it
 * wrote them, n_rings <= 2^32 - 2): every hole ring assigned to the outer ring it lies in, on the device.  The
 * definition, in full in rayjoin_amd/csrc/rj_polygons.h:
 *   a ring of face 0 belongs to no polygon (n_face0); a ring of another face is a shell when area2 > 0, else a hole (a
 *   ring of area 0 is a dangling tree inside its face).  The top of a ring is its largest (y, x).  A ceiling edge is a
 *   ring edge u -> v with v.x < u.x (the ring's face lies below it).  above(H), for a hole H of face f with top p: among
 *   the ceiling edges of the rings of face f with v.x <= p.x < u.x whose height at p.x is strictly above p.y, the ring of
 *   the edge with the smallest height at p.x, then the smallest slope, then the smallest point slot of u (all exact,
 *   int128).  parent(H): follow above until a shell; a walk that ends at a hole with nothing above it makes H an orphan
 *   (n_orphans; none on a consistently labelled planar map).  One polygon per shell, ascending by shell index (the
 *   polygons of a face are contiguous); its members: the shell, then its holes by ascending ring index; area2 = the sum
 *   of its members' area2.
 * Output, all caller-owned device memory: parent_dev[n_rings] (may be NULL): the shell's ring index for a hole, its own
 * index for a shell, RJ_POLY_NONE for a ring of face 0 and for an orphan -- always written in full;
 * polygons_dev[polygon_capacity]; poly_first_dev[polygon_capacity + 1], the CSR of the polygons into
 * poly_ring_dev[member_capacity] (ring indices).  n_members = n_polygons + n_holes; n_holes counts the holes that have
 * a parent.  RJ_E_OVERFLOW when a count exceeds its capacity: *counts holds the true counts and nothing beyond any
 * capacity is written; all capacities 0 (arrays may be NULL) is the sizing call.  n_rings == 0 is valid.  flags must be
 * 0.  RJ_E_INVALID for a ring_row that does not start at 0, decreases or does not end at n_points, a coordinate outside
 * [-2^46, 2^46), rings that do not ascend by ((uint32) face << 32) | leader, a non-zero flags; RJ_E_INTERNAL when the
 * round budget runs out (33 jumping steps: cannot happen).  Runs on the handle's stream with one host sync, at the
 * end, to read the counts; scratch (72 bytes per point and 96 per ring plus the sorts' temporary storage) is
 * allocated per call and freed; no state of the handle changes. */
int rj_rings_polygons(rj_handle h, const rj_ring* rings_dev, uint64_t n_rings, const uint32_t* ring_row_dev,
                      const int64_t* ring_xy_dev, uint64_t n_points, uint32_t flags,
                      uint64_t polygon_capacity, uint64_t member_capacity,
                      uint32_t* parent_dev, rj_polygon* polygons_dev, uint32_t* poly_first_dev,
                      uint32_t* poly_ring_dev, rj_polygons_counts* counts);

/* ---- rings to map ------------------------------------------------------------------------ */
/* rj_rings_map flags */
#define RJ_RMAP_DISSOLVE 1u /* leave out every unique edge with the same face on both sides (n_dissolved) */

typedef struct {
  uint64_t n_chains, n_points, n_edges, n_closed, n_zero_edges, n_conflicts, n_dissolved;
} rj_rings_map_counts;

/* extends: the chain map that a set of labelled rings bounds, on the device -- the inverse of rj_map_rings, and the way
 * in for polygon data: one closed ring per boundary (every shared boundary stored twice) becomes chains with a left and
 * a right face, shared boundaries stored once, cut at junctions, and maximal.  ring_row_dev[n_rings + 1] is the CSR into
 * ring_xy_dev[2 n_points] (the layout rj_map_rings writes; a ring is a closed walk, its last point is followed by its
 * first; 0, 1 or 2 points are allowed); ring r has the 32-bit label *(int32_t*) ((char*) ring_face_dev + r face_stride)
 * on the LEFT of its walk, y up (shells counter-clockwise, holes clockwise; 0 is "no face"): face_stride 4 reads a plain
 * int32 array, sizeof(rj_ring) the face field of rj_map_rings' records in place.  n_points < 2^31.  The definition, in
 * full in rayjoin_amd/csrc/rj_ringmap.h:
 *   point slot i gives the directed edge u -> v to its successor; u == v is dropped (n_zero_edges); lo < hi its points by
 *   (x, y); forward (u == lo) it has the ring's face on the left of lo -> hi, backward on the right.  One unique edge per
 *   distinct (lo, hi), ascending by (lo.x, lo.y, hi.x, hi.y): left = the face of its forward directed edge with the
 *   smallest slot (0: none), right the same over the backward ones; more than one of a kind is counted in n_conflicts
 *   (overlapping input; the result is still determined).  Under RJ_RMAP_DISSOLVE an edge with left == right is left out
 *   (n_dissolved).  Kept edge e has the half-edges 2 e (lo -> hi, faces (left, right)) and 2 e + 1 (hi -> lo, faces
 *   swapped).  h passes the vertex it arrives at when exactly two kept half-edges start there, h ^ 1 and one other, g,
 *   with faces(g) == faces(h): next(h) = g; otherwise it ends there.  The maximal sequences under next are the walks; the
 *   leader of an open walk is its first half-edge, of a closed walk (a cycle) its smallest, which it is read from; of a
 *   walk and its twin walk the chain is the one with the smaller leader.  A chain's points: the start points of its
 *   half-edges, then the end point of the last (a closed chain repeats its first point); left / right: its leader's
 *   faces; chains ascend by leader.  n_points = n_edges + n_chains; n_closed counts the closed chains.
 * Output, all caller-owned device memory, with the contract of rj_upload_map_dev (every chain has at least 2 points):
 * xy_dev[2 point_capacity], row_index_dev[chain_capacity + 1], left_dev / right_dev[chain_capacity].  RJ_E_OVERFLOW when a
 * count exceeds its capacity: *counts holds the true counts and nothing beyond any capacity is written; all capacities
 * 0 (arrays may be NULL) is the sizing call.  n_rings == 0 is valid.  RJ_E_INVALID for a ring_row that does not start
 * at 0, decreases or does not end at n_points, a coordinate outside [-2^46, 2^46), n_points >= 2^31, a face_stride below
 * 4 or no multiple of 4, an unknown flag bit; RJ_E_INTERNAL when a round budget runs out (33 doubling steps: cannot
 * happen below 2^32 half-edges).  Runs on the handle's stream with one host sync, at the end, to read the counts;
 * scratch (288 bytes per point slot plus the sorts' temporary storage) is allocated per call and freed; no state of the
 * handle changes. */
int rj_rings_map(rj_handle h, const uint32_t* ring_row_dev, const int64_t* ring_xy_dev, uint64_t n_points,
                 const void* ring_face_dev, uint64_t face_stride, uint64_t n_rings, uint32_t flags,
                 uint64_t chain_capacity, uint64_t point_capacity,
                 int64_t* xy_dev, uint32_t* row_index_dev, int32_t* left_dev, int32_t* right_dev,
                 rj_rings_map_counts* counts);

/* ---- crossings inside one map --------------------------------------------------------------- */
/* rj_crossing kinds */
#define RJ_CROSS_PROPER 1u  /* the segments cross in a point that is an end point of neither */
#define RJ_CROSS_TOUCH 2u   /* an end point of one edge lies inside the other edge */
#define RJ_CROSS_OVERLAP 3u /* collinear, more than one point in common, the end-point sets differ */
#define RJ_CROSS_EQUAL 4u   /* the same two end points, in either direction (a chain that folds back a -> b -> a) */

typedef struct {
  uint32_t eid[2]; /* eid[0] < eid[1] */
  uint32_t kind;   /* RJ_CROSS_* */
  uint32_t _pad;
} rj_crossing; /* 16 bytes */

typedef struct {
  uint64_t n_found, n_proper, n_touch, n_overlap, n_equal, n_edges, n_zero_edges;
} rj_crossings_counts;

/* extends: the check that a chain map is a planar subdivision, which every stage of the library assumes and none makes
 * (the reference never validates a map either: Map::LoadFrom, src/map/map.h:162-233) -- all pairs of edges of ONE map
 * that meet anywhere except in a shared end point, exactly, on the device, from a map in device memory: before
 * rj_upload_map* of user polygons (self-crossing rings, overlapping polygons of one layer, a vertex inside a
 * neighbour's edge), or between two overlays on rj_overlay_map's output.  rj_lsi_query cannot do this: it refuses
 * base == query, and its simulation-of-simplicity predicate reports shared vertices.
 * Input: xy_dev[2 np], row_index_dev[nc + 1], the contract of rj_map_rings (a chain may have a single point; faces are
 * not needed).  Edge e = p - c joins points p and p + 1 of chain c (the numbering of every other call);
 * ne = np - nc < 2^32 - 1.  An edge whose two points are equal is skipped and counted in n_zero_edges.  The definition,
 * in full in rayjoin_amd/csrc/rj_crossings.h: for two distinct non-zero edges e < f let S be the intersection of their
 * closed segments.  S empty, or one point that is an end point of both (consecutive edges of a chain, a junction): no
 * record.  One point that is an end point of exactly one: RJ_CROSS_TOUCH; of neither: RJ_CROSS_PROPER.  More than one
 * point: RJ_CROSS_EQUAL when the end-point sets match, else RJ_CROSS_OVERLAP.  Decided from four orientation signs
 * (int128 cross products) and coordinate comparisons: no floating point, no division, no simulation of simplicity.
 * Output: out_dev[capacity], caller-owned device memory: one record per unordered pair with a kind, every pair exactly
 * once, ascending by ((uint64_t) eid[0] << 32) | eid[1] -- fully determined, independent of every tuning choice (the
 * candidates come from a sparse uniform grid of the map's own, whose cell size is chosen from the edges' extents).
 * counts: n_found = n_proper + n_touch + n_overlap + n_equal, n_edges = ne.  flags must be 0.  RJ_E_OVERFLOW when
 * n_found > capacity: *counts holds the true counts, nothing beyond capacity is written and the contents of out_dev
 * are unspecified; capacity 0 (out_dev may be NULL) is the sizing call.  nc == 0 and ne == 0 are valid.  RJ_E_INVALID
 * for a row_index that does not start at 0, does not ascend or does not end at np, a coordinate outside
 * [-2^46, 2^46), an unknown flag -- and for a map whose grid would need more than 2^36 pair tests (a few edges as long
 * as the map over millions of short ones: minutes of a device that may be shared): the message names the largest
 * cell and nothing is tested.  Runs on the handle's stream with four host syncs (the sums behind the grid's size, the
 * number of pair tests, the number of records, the end): a check made once per map, not a step of a pipeline.  Scratch
 * (48 bytes per edge, 33 per registration -- at most 4 ne + 1024 of them --, 24 per record up to capacity, plus the
 * sorts' temporary storage) is allocated per call and freed; no map, index or option of the handle changes.
 * For tests and tools, through rj_set_debug_option (0: the default; none can change a result): "cross_shift" 15..47
 * forces the grid's shift, "cross_pair_budget" lowers the 2^36, "cross_extent_factor" / "cross_reg_factor" replace the 8
 * and 4 of the choice of the shift (a cell is 8 mean edge extents wide; at most 4 ne + 1024 registrations).  What the
 * last call chose and took, through rj_get_option: "cross_last_shift", "cross_last_registrations",
 * "cross_last_largest_cell" (its edges), "cross_last_pair_tests", "cross_last_items", "cross_last_us0" .. "cross_last_us5"
 * (HIP-event microseconds of the stages: edges and sums, registrations and their sort, runs and work items, the pair
 * pass, the sort of the hits, all; -1: not reached). */
int rj_map_crossings(rj_handle h, const int64_t* xy_dev, uint64_t np, const uint32_t* row_index_dev, uint64_t nc,
                     uint32_t flags, uint64_t capacity, rj_crossing* out_dev, rj_crossings_counts* counts);

/* ---- noding: cut edges at the vertices that touch them ------------------------------------------ */
#define RJ_NODE_DROP_LAST 1u /* every chain is written without its last point: the ring layout rj_rings_map takes */

typedef struct {
  uint64_t n_points, n_edges;   /* of the output; n_edges = ne + n_cuts in either layout */
  uint64_t n_cuts, n_cut_edges, n_max_cuts; /* inserted points; input edges with a cut; the most on one edge */
  uint64_t n_used, n_proper, n_equal;       /* records of kind TOUCH or OVERLAP; PROPER and EQUAL records, which cut nothing */
} rj_node_counts;

/* extends: the repair behind rj_map_crossings' answer where it can be made exactly -- T-junctions and half-shared
 * borders (RJ_CROSS_TOUCH, RJ_CROSS_OVERLAP: one polygon has a vertex on a border that its neighbour's ring runs
 * straight past), the commonest reason a polygon layer is no planar subdivision.  Every point to insert is already a
 * vertex of the map; behind the call overlapping edges are equal edges, which rj_rings_map stores once.
 * RJ_CROSS_PROPER records are counted (n_proper) and left alone: their point is no integer.  RJ_CROSS_EQUAL needs no cut.
 * Input: the map as rj_map_crossings takes it, and cross_dev[n_cross], the records rj_map_crossings wrote for this very
 * map (device memory).  The definition, in full in rayjoin_amd/csrc/rj_node.h: edge e = p - c runs from a (point p) to
 * b (point p + 1); a point q lies inside e when e is not of zero length, orient(a, b, q) == 0 (an int128 cross product),
 * q is in e's closed box and is neither a nor b.  The cut set C(e): the distinct points q such that some record (e, f)
 * or (f, e) of kind TOUCH or OVERLAP exists, q is an end point of f and q lies inside e -- tested for all four (end
 * point, other edge) combinations of every such record, so a record whose kind does not fit the geometry cannot put a
 * point off an edge.
 * Output, caller-owned device memory: out_xy_dev[2 point_capacity], out_row_index_dev[nc + 1]: every chain keeps its
 * points in order, and after point p come the points of C(p - c), ascending by their distance from a (|q.x - a.x|, or
 * |q.y - a.y| on a vertical edge), equal points once.  Chains, their number and their order do not change: the
 * caller's left / right arrays stay valid.  edge_origin_dev[n_edges] (may be NULL): the input edge that output edge
 * p' - c is a part of.  Under RJ_NODE_DROP_LAST every chain must have at least 2 points and its first point must equal
 * its last; every chain is then written without its last point -- rj_rings_map's ring layout --, point slot k is
 * output edge k, and edge_origin_dev[k] still applies.  Fully determined, independent of every tuning choice.
 * point_capacity 0 (arrays may be NULL) is the sizing call; RJ_E_OVERFLOW when n_points > point_capacity: *counts holds
 * the true counts and nothing is written.  nc == 0, n_cross == 0 and cross_dev == NULL with n_cross == 0 are valid;
 * with no records the output is a copy of the input.  RJ_E_INVALID, with nothing written: the map checks of
 * rj_map_crossings, an unknown flag bit, n_cross >= 2^31, np + n_cuts >= 2^32, a record with eid[0] >= eid[1],
 * eid[1] >= ne or a kind outside 1..4, a record that names a zero-length edge, records that do not strictly ascend by
 * ((uint64_t) eid[0] << 32) | eid[1], an open or one-point chain under RJ_NODE_DROP_LAST.  Runs on the handle's stream
 * with one host sync, at the end, for the counts.  Scratch (80 bytes per record, 12 per edge, plus the sort's and the
 * scans' temporary storage) is allocated per call and freed; no map, index or option of the handle changes.
 * rj_get_option: "node_last_us0" .. "node_last_us5" (HIP-event microseconds of the stages: the check, the candidates,
 * their sort and the kept cuts, the cuts per edge and their scan, the two scatters, all; -1: not reached). */
int rj_map_node(rj_handle h, const int64_t* xy_dev, uint64_t np, const uint32_t* row_index_dev, uint64_t nc,
                const rj_crossing* cross_dev, uint64_t n_cross, uint32_t flags, uint64_t point_capacity,
                int64_t* out_xy_dev, uint32_t* out_row_index_dev, uint32_t* edge_origin_dev, rj_node_counts* counts);

/* ---- snapping: cut edges at their rounded proper crossings too ----------------------------------- */
#define RJ_SNAP_DROP_LAST 1u /* as RJ_NODE_DROP_LAST */

typedef struct {
  uint64_t n_points, n_edges;   /* as rj_node_counts: of the output; n_edges = ne + n_cuts in either layout */
  uint64_t n_cuts, n_cut_edges, n_max_cuts; /* inserted points of all kinds; input edges with a cut; the most on one edge */
  uint64_t n_used, n_proper, n_equal;       /* records of kind TOUCH or OVERLAP; PROPER records (stale ones included); EQUAL records */
  uint64_t n_exact;   /* PROPER records whose crossing point is an integer point: nothing was rounded */
  uint64_t n_at_end;  /* (PROPER record, edge) combinations left uncut because the rounded point is an end point of that edge */
  uint64_t n_stale;   /* PROPER records that do not fit the geometry: they cut nothing */
} rj_snap_counts;

/* extends: the missing link between "this map has crossings" and "a planar map" -- a layer whose polygons overlap, a
 * self-crossing ring, an overlay output whose truncated cut points made a crossing.  rj_map_node plus one cut at the
 * rounded point of every RJ_CROSS_PROPER record: both edges are cut at the same integer point and the crossing becomes a
 * shared vertex.  Moving a point by up to half a unit can make new crossings, so ONE call does not promise a planar
 * map: the caller repeats rj_map_crossings and rj_map_snap until a check finds nothing (ops.map_snap_rounds).  That the
 * rounds end is measured, not guaranteed (two or three on ordinary input, many on fans of near-parallel long
 * edges); the counts of both calls report the progress.
 * Input: the map and cross_dev[n_cross] exactly as rj_map_node takes them, with the same checks and the same codes;
 * RJ_SNAP_DROP_LAST means what RJ_NODE_DROP_LAST means.  The definition, in full in rayjoin_amd/csrc/rj_snap.h:
 * TOUCH and OVERLAP records cut exactly as in rj_map_node (four tests per record, a cut only where the geometry holds).
 * A PROPER record (e, f), e < f, with A, B the points of e, C, D the points of f, r = B - A, s = D - C: den = r x s,
 * tn = (C - A) x s, un = (C - A) x r (int128, below 2^95), all three negated when den < 0.  den == 0, or not
 * 0 < tn < den, or not 0 < un < den: the record is stale, cuts nothing and is counted in n_stale.  Otherwise
 * q = A + (rnd(r.x tn / den), rnd(r.y tn / den)) with rnd(v) = floor(v + 1/2) -- halves toward +infinity whatever the
 * direction of the edge, exact in integers, always computed from the lower-numbered edge.  q is inserted into e unless
 * it equals A or B and into f unless it equals C or D; each such drop counts once in n_at_end and the other edge is
 * still cut there.  q lies in the closed boxes of both edges: coordinates stay in range.  n_exact: the records whose
 * point needed no rounding.
 * Output, caller-owned device memory, in the layout of rj_map_node: out_xy_dev[2 point_capacity],
 * out_row_index_dev[nc + 1], edge_origin_dev[n_edges] (may be NULL).  After point p come the cuts of edge p - c,
 * ascending by the pair (|q.major - a.major|, |q.minor - a.minor|), the major axis of an edge being x when |dx| >= |dy|,
 * else y -- a monotone function of the exact parameter along the edge for points on it and for rounded crossing points;
 * equal pairs are equal points, which appear once.  Chains, their number and their order do not change: the caller's
 * left / right arrays stay valid as chain labels (what they mean where polygons overlapped is rj_map_faces' question).
 * On records without a PROPER kind the output arrays and the eight counts shared with rj_node_counts equal
 * rj_map_node's bit for bit.  Fully determined, independent of every tuning choice.
 * point_capacity 0 (arrays may be NULL) is the sizing call; RJ_E_OVERFLOW when n_points > point_capacity: *counts holds
 * the true counts and nothing is written.  nc == 0, n_cross == 0 and cross_dev == NULL with n_cross == 0 are valid;
 * with no records the output is a copy of the input.  RJ_E_INVALID, with nothing written: every case of rj_map_node
 * (the map checks of rj_map_crossings, an unknown flag bit, n_cross >= 2^31, np + n_cuts >= 2^32, a record with
 * eid[0] >= eid[1], eid[1] >= ne or a kind outside 1..4, a record that names a zero-length edge, records that do not
 * strictly ascend, an open or one-point chain under RJ_SNAP_DROP_LAST).  Runs on the handle's stream with one host
 * sync, at the end, for the counts.  Scratch (144 bytes per record -- a cut carries its point --, 12 per edge, plus the
 * sort's and the scans' temporary storage) is allocated per call and freed; no map, index or option of the handle
 * changes.  rj_get_option: "snap_last_us0" .. "snap_last_us5" (HIP-event microseconds of the stages: the check, the
 * candidates, their sort and the kept cuts, the cuts per edge and their scan, the two scatters, all; -1: not reached). */
int rj_map_snap(rj_handle h, const int64_t* xy_dev, uint64_t np, const uint32_t* row_index_dev, uint64_t nc,
                const rj_crossing* cross_dev, uint64_t n_cross, uint32_t flags, uint64_t point_capacity,
                int64_t* out_xy_dev, uint32_t* out_row_index_dev, uint32_t* edge_origin_dev, rj_snap_counts* counts);

/* ---- thinning: fewer points on every chain, the same chains ------------------------------------- */
typedef struct {
  uint64_t n_points, n_removed;  /* of the output; n_removed = np - n_points */
  uint64_t n_rounds;             /* rounds that removed something */
  uint64_t n_closed;             /* chains of 3 points or more whose first point equals the last */
  uint64_t n_pinned_extra;       /* the m1 / m2 of closed chains that were pinned */
  uint64_t n_max_round;          /* the most removals in one round */
} rj_simplify_counts;

/* extends: what makes a map smaller -- an overlay output or a layer of millions of edges is display, export or coarse
 * pre-filter material only after thinning, and thinning the CHAINS is the one way that keeps neighbours together: a
 * border that two faces share is stored once, so both polygons are thinned identically and no sliver or gap opens between
 * them (what arc-based tools do on the host, and a per-polygon simplifier cannot).  Visvalingam-Whyatt by effective area,
 * in rounds, on the device, on a map in device memory.  (The reference has no counterpart: its maps are loaded as they
 * are, Map::LoadFrom, src/map/map.h:162-233.)
 * Input: the map as rj_map_crossings takes it (a chain may have a single point), and tol = (tol_hi << 64) | tol_lo, an
 * unsigned 128-bit number: twice an area in scaled units^2, the unit of rj_overlay_face.area2.  flags must be 0.
 * The definition, in full in rayjoin_amd/csrc/rj_simplify.h: the first and the last point of every chain are pinned --
 * junctions and the chain graph never change.  In a closed chain (3 points or more, first equal to last) with a its
 * first point, m1, the interior point farthest from a (squared distance, ties to the lowest index), is pinned if that
 * distance is > 0, and then m2, the interior point with the greatest |cross(m1 - a, q - a)| (ties to the lowest index),
 * if that value is > 0: a ring never collapses below the triangle a, m1, m2.  A live unpinned point p between its live
 * neighbours u and w weighs W(p) = |cross(p - u, w - u)| (int128, below 2^95) and is a candidate when W(p) <= tol; its
 * key is (W(p), (uint32_t) (p * 2654435761u)), p the input point index.  A round removes, all at once, every candidate
 * whose key is smaller than the key of each live neighbour that is also a candidate; rounds repeat until one has no
 * candidate.  Integers only, exact, fully determined, independent of every tuning choice.
 * Output, caller-owned device memory: out_xy_dev[2 point_capacity] the live points in input order,
 * out_row_index_dev[nc + 1], origin_dev[n_points] (may be NULL): the input point of every output point.  Chains, their
 * number and their order do not change: the caller's left / right arrays stay valid.  Every unpinned output point weighs
 * more than tol in the output; a second call with the same tol removes nothing; tol = 2^128 - 1 leaves the pinned points
 * (2 of an open chain); tol = 0 removes collinear runs and spikes a -> b -> a.  NOT promised: that the thinned map has
 * no crossings -- thinning can push a chain across another one; rj_map_crossings tells.
 * point_capacity 0 (arrays may be NULL) is the sizing call; RJ_E_OVERFLOW when n_points > point_capacity: *counts holds
 * the true counts and nothing is written.  nc == 0 is valid.  RJ_E_INVALID, with nothing written: the map checks of
 * rj_map_crossings, a nonzero flag, np >= 2^32.  Runs on the handle's stream with one host sync per round (the points
 * it removed and the size of the next round's work list: two numbers) and one at the end.  After the first round a
 * round looks only at its work list -- the candidates that stayed and the neighbours of the points just removed --, so
 * a late round costs what it looks at, not np.  Scratch (38 bytes per point plus the scan's temporary storage) is
 * allocated per call and freed; no map, index or option of the handle changes.
 * For tests, through rj_set_debug_option: "simplify_all_points" 1 makes every round look at every point (the same
 * result).  What the last call took, through rj_get_option: "simplify_last_us0" .. "simplify_last_us5" (HIP-event
 * microseconds of the stages: the check, the links and the pins, the first round, the later rounds, the scan and the
 * scatter, all; -1: not reached), "simplify_last_syncs", "simplify_last_list_sum" / "simplify_last_list_max" (the work
 * lists behind the first round), "simplify_round_list0" .. "9" and "simplify_round_us0" .. "9" (the first ten rounds:
 * the points looked at, the host's microseconds from the first launch to the sync), "simplify_late_rounds" /
 * "simplify_late_list" / "simplify_late_us" (the rounds behind them, summed). */
int rj_map_simplify(rj_handle h, const int64_t* xy_dev, uint64_t np, const uint32_t* row_index_dev, uint64_t nc,
                    uint64_t tol_lo, uint64_t tol_hi, uint32_t flags, uint64_t point_capacity, int64_t* out_xy_dev,
                    uint32_t* out_row_index_dev, uint32_t* origin_dev /* may be NULL */, rj_simplify_counts* counts);

/* extends: the faces of a chain map computed from its geometry alone, on the device -- the label side of "a user's data
 * in, a valid planar map out".  Input: xy_dev[2 np], row_index_dev[nc + 1], the contract and the size limits of
 * rj_map_rings, without labels: chains meet only at their end points, a chain may have a single point.  flags must be 0.
 * The definition, in full in rayjoin_amd/csrc/rj_faces.h: the rings of the map are those of rj_map_rings with no face
 * involved, ascending by leader; a ring with area2 > 0 is a shell, every other ring a hole (the outside of a connected
 * component, or an isolated tree).  A hole's ray goes up from its top, its largest (y, x); the first ceiling edge above
 * it (the half-open rule and the exact order of rj_rings_polygons, over the ceiling edges of ALL rings) names the ring
 * above; following that until a shell is reached gives the hole's face, and a walk that ends with nothing above puts it
 * in face 0, the unbounded face.  Face k (1-based) is the k-th shell by ascending leader.
 * Output, caller-owned device memory: left_dev[nc] / right_dev[nc] = the face of the ring of half-chain 2 c / 2 c + 1 (0
 * for a chain whose points are all equal: n_skipped); faces_dev[face_capacity] (may be NULL), record k - 1 for face k:
 * its shell's leader, its holes, area2 = the shell's plus its holes' = twice the face's area (an exact int128), its label.
 * Counts: n_faces (shells), n_rings, n_holes (holes inside a shell), n_outer (holes of face 0), n_skipped, n_dangling
 * (chains that are not skipped with left == right: bridges and dangles), n_conflicts.
 * in_left_dev / in_right_dev: both NULL, or both given -- the labels to check.  Then label of face k = the given label of
 * its shell's leader half-chain (face 0: 0), and n_conflicts = the half-chains that are not skipped and whose given label
 * differs from the label of their computed face: 0 means the labels and the geometry describe the same partition
 * (whether label is injective the caller reads from faces_dev).  Without labels every label is 0.
 * faces_dev NULL: no records, face_capacity is ignored, nothing overflows.  Otherwise RJ_E_OVERFLOW when n_faces >
 * face_capacity: *counts holds the true counts, left_dev / right_dev are written in full, nothing is written beyond the
 * capacity.  nc == 0 is valid.  RJ_E_INVALID, with nothing written: a map that fails the checks of rj_map_rings, a
 * nonzero flag, one label pointer without the other.  RJ_E_INTERNAL when a round budget of 33 runs out.  On a map
 * without RJ_CROSS_OVERLAP / RJ_CROSS_EQUAL records the result equals rj_map_rings with one constant label followed by
 * rj_rings_polygons' parent[]; it is fully determined for every input.  Runs on the handle's stream with one host sync,
 * at the end; scratch (rj_faces.h has the bytes per chain, point and registration) is allocated per call and freed; no
 * map, index or option of the handle changes.
 * Coordinates are expected scaled to the range: the grid that keeps a hole from testing every edge has cells of at
 * least 2^15 units, so a map drawn in single units lies in one cell and costs holes x edges -- with the same result.
 * For tests, through rj_set_debug_option: "faces_shift" (15..47, 0: choose) is where the search for the grid's shift
 * starts; the registration bound can still make it coarser, never the result different.  What the last call took,
 * through rj_get_option: "faces_last_shift", "faces_last_registrations", "faces_last_ray_tests" (candidate tests),
 * "faces_last_cells" (cells that rays visited), "faces_last_us0" .. "faces_last_us5" (HIP-event microseconds: the ring
 * stages, tops and kinds, the grid, the rays, parents and faces, all; -1: not reached). */
typedef struct {
  uint32_t leader, n_holes;
  int32_t label;
  uint32_t _pad;
  uint64_t area2_lo;
  int64_t area2_hi;
} rj_face; /* 32 bytes */
typedef struct {
  uint64_t n_faces, n_rings, n_holes, n_outer, n_skipped, n_dangling, n_conflicts;
} rj_faces_counts;
int rj_map_faces(rj_handle h, const int64_t* xy_dev, uint64_t np, const uint32_t* row_index_dev, uint64_t nc,
                 const int32_t* in_left_dev, const int32_t* in_right_dev, uint32_t flags, uint64_t face_capacity,
                 int32_t* left_dev, int32_t* right_dev, rj_face* faces_dev /* may be NULL */, rj_faces_counts* counts);

/* ---- eliminating slivers: a small face joins the neighbour with the longest shared border ------------ */
#define RJ_ELIM_DROP 1u            /* write the map without the chains whose two labels became equal */
/* rj_elim_face flags */
#define RJ_ELIM_SLIVER     1u      /* 0 <= area2 <= tol */
#define RJ_ELIM_ELIMINATED 2u      /* target != label */
#define RJ_ELIM_ISLAND     4u      /* a sliver with no eligible neighbour: it stays */
#define RJ_ELIM_NEGATIVE   8u      /* area2 < 0: inconsistent labels; never a sliver, may be a target */
typedef struct { int32_t label, target, best; uint32_t flags; uint64_t area2_lo; int64_t area2_hi; } rj_elim_face; /* 32 bytes */
typedef struct { uint64_t n_faces, n_slivers, n_eliminated, n_islands, n_mutual, n_negative,
                 n_chains, n_points, n_dropped; } rj_eliminate_counts;

/* extends: what removes slivers -- the overlay truncates cut points to integers, rj_map_snap turns near misses into thin
 * triangles, two layers thinned separately and overlaid leave faces of a few units^2 along every almost-shared border.
 * This is the operation GIS users know as Eliminate: a face whose area is at most a tolerance joins the neighbour it
 * shares the longest border with, on the device, on a labelled chain map in device memory.  (The reference has no
 * counterpart: its WriteOutputChain writes whatever the cuts produced.)
 * Input: xy_dev[2 np], row_index_dev[nc + 1], left_dev[nc], right_dev[nc] with the contract, the checks and the size limits
 * of rj_map_rings (a chain may have a single point); labels are any int32.  tol = (tol_hi << 64) | tol_lo, an unsigned
 * 128-bit number: twice an area in scaled units^2, as in rj_map_simplify.
 * The definition, in full in rayjoin_amd/csrc/rj_eliminate.h:
 *   a face is a label value other than 0 that occurs in left or right (a multi-part polygon with one label is one face;
 *   faces from geometry: rj_map_faces first).  Faces are numbered by ascending (uint32_t) label, and "smaller label" means
 *   that unsigned order.  Of chain c: S(c) = the sum of cross(p_i, p_i+1) over its edges (int128), L(c) = the sum of
 *   floor(sqrt(dx^2 + dy^2)) over its edges (the exact integer square root; an unsigned 128-bit sum).
 *   area2(f) = the sum of S(c) over left[c] == f minus the sum over right[c] == f (the rule of rj_overlay_faces: exact for
 *   consistent labels, holes subtract themselves).  f is a sliver when 0 <= area2(f) <= tol; area2(f) < 0 sets
 *   RJ_ELIM_NEGATIVE and f is never a sliver.  Faces f != g, both not 0, are neighbours when some chain has
 *   {left, right} = {f, g}; w(f, g) = the sum of L(c) over those chains, and a pair with w = 0 is still a pair.  Face 0 is
 *   never a neighbour, a sliver or a target; chains with left == right contribute nothing.
 *   best(f) of a sliver = the neighbour with the largest w, ties to the smaller min(f, g), then the smaller max(f, g); a
 *   sliver without a neighbour is an island (RJ_ELIM_ISLAND) and stays; every other face has no best (its record holds
 *   its own label).  When best(f) = g and best(g) = f (a mutual pair, n_mutual) the one with the larger area2 stays as
 *   a root, a tie goes to the smaller label, and the other points at it.  target(f) = the root reached by following
 *   best; roots are the non-slivers, the islands and the winners of mutual pairs; target(0) = 0.
 *   ONE CALL IS ONE ROUND: a merged group may still be at most tol, and the caller repeats the call.
 * Output, caller-owned device memory: out_left_dev[c] = target(left[c]), out_right_dev[c] = target(right[c]);
 * faces_dev[face_capacity] (may be NULL: no records, face_capacity is ignored), record k of the k-th face: its label,
 * target, best, flags and its own area2 (a two's-complement int128).  Without RJ_ELIM_DROP out_left_dev / out_right_dev
 * are [nc] (chain_capacity >= nc), out_xy_dev, out_row_index_dev, chain_origin_dev and point_capacity are ignored,
 * n_chains = nc and n_points = np.  With RJ_ELIM_DROP a chain is dropped, and counted in n_dropped, exactly when its
 * input labels differ and its output labels are equal (bridges and dangles that came with left == right stay); the kept
 * chains are written in input order with their points into out_xy_dev[2 point_capacity] and
 * out_row_index_dev[chain_capacity + 1], their labels into out_left_dev / out_right_dev[chain_capacity], and
 * chain_origin_dev[k] (may be NULL) is the input chain of output chain k.  Chains are NOT re-joined at vertices that
 * drop to degree 2: that is rj_map_dissolve with RJ_DISS_KEEP_EQUAL, as for every other map.
 * All capacities 0 (arrays may be NULL) is the sizing call.  RJ_E_OVERFLOW when a count exceeds its capacity: *counts
 * holds the true counts and nothing is written.  nc == 0 is valid.  RJ_E_INVALID, with nothing written: the map checks
 * of rj_map_rings and an unknown flag bit.  RJ_E_INTERNAL when the budget of 33 jumping rounds runs out (the order on
 * pairs is strict, so the pointers have no cycle but the mutual pairs: cannot happen).  Integers only, exact, fully
 * determined.  Runs on the handle's stream with one host sync, at the end; scratch (rj_eliminate.h has the bytes per
 * chain) is allocated per call and freed; no map, index or option of the handle changes.  For tests and sweeps, through
 * rj_set_debug_option: "elim_point_blocks" (0: by size) is the grid of the two passes over the points, the chain sums
 * and the scatter; any grid gives the same result.  rj_get_option:
 * "elim_last_us0" .. "elim_last_us5" (HIP-event microseconds of the stages: the check and the chain sums, the faces,
 * the pairs and the choice, the pointers, the new labels and the scatter, all; -1: not reached). */
int rj_map_eliminate(rj_handle h, const int64_t* xy_dev, uint64_t np, const uint32_t* row_index_dev,
                     const int32_t* left_dev, const int32_t* right_dev, uint64_t nc,
                     uint64_t tol_lo, uint64_t tol_hi, uint32_t flags,
                     uint64_t face_capacity, uint64_t chain_capacity, uint64_t point_capacity,
                     rj_elim_face* faces_dev /* may be NULL */, int32_t* out_left_dev, int32_t* out_right_dev,
                     int64_t* out_xy_dev, uint32_t* out_row_index_dev, uint32_t* chain_origin_dev /* may be NULL */,
                     rj_eliminate_counts* counts);

/* ---- dissolve: faces that share a class become one face; chains that meet two by two become one chain ---- */
#define RJ_DISS_KEEP_EQUAL 1u   /* keep chains whose two classes are equal: join only, nothing dissolves */
typedef struct { int32_t label; uint32_t n_sides; uint64_t area2_lo; int64_t area2_hi; } rj_diss_class; /* 24 bytes */
typedef struct { uint64_t n_kept, n_dropped, n_skipped, n_chains, n_points, n_closed, n_classes, n_unmapped; } rj_dissolve_counts;

/* extends: what GIS users know as Dissolve, and the re-joining of chains that rj_map_eliminate and the overlay
 * operations leave behind, in one chain-level call on the device: it sorts the 2 nc chain ends, never an edge.
 * (The reference has no counterpart.)
 * Input: xy_dev[2 np], row_index_dev[nc + 1], left_dev[nc], right_dev[nc] with the contract, the checks and the size limits
 * of rj_map_eliminate (a chain may have a single point); labels are any int32.
 * The definition, in full in rayjoin_amd/csrc/rj_dissolve.h:
 *   class(0) = 0; with class_dev NULL class(f) = f, otherwise class(f) = class_dev[f] for 0 < f < n_labels.  A nonzero
 *   label outside that range is counted in n_unmapped: the call is RJ_E_INVALID then, nothing is written and *counts
 *   holds n_unmapped.  A nonzero label may map to 0, which erases the face into the outside.
 *   A chain whose points are all equal is skipped (n_skipped).  Of the others a chain is kept (n_kept) unless
 *   class(left) == class(right) and RJ_DISS_KEEP_EQUAL is not set (n_dropped): bridges and dangles go with the borders
 *   unless the flag keeps them.
 *   Half-chain h = 2 c walks chain c first -> last with classes (L, R), h = 2 c + 1 last -> first with (R, L).  h arrives
 *   at the start point of h ^ 1; when exactly two kept half-chains start there (h ^ 1 and one other, g) and
 *   classes(g) == classes(h), next(h) = g; otherwise h ends there (a junction, a dead end, a change of classes).  A closed
 *   chain alone at its vertex has next(h) = h.  Walks are the maximal sequences under next, open or closed; the leader
 *   of an open walk is its first half-chain, of a closed walk its smallest, and the walk is read from there.  Of a walk
 *   and its twin (the twins in reverse order) the one with the smaller leader is an output chain.
 * Output, caller-owned device memory: the chains ascend by leader into out_xy_dev[2 point_capacity],
 * out_row_index_dev[chain_capacity + 1], out_left_dev / out_right_dev[chain_capacity] (the classes of the leader).  The
 * points of a chain are every half-chain's points in its direction without its last point, then the last point of the last
 * half-chain, copied verbatim; a closed chain repeats its first point; every chain has at least 2 points: a map that
 * rj_upload_map_dev takes.  chain_origin_dev[chain_capacity] (may be NULL): the leader's input chain.
 * chain_out_dev[nc] (may be NULL): (k << 1) | reversed for a kept input chain that output chain k holds, 0xFFFFFFFF for
 * a dropped or skipped one.  classes_dev[class_capacity] (may be NULL: no records, class_capacity is ignored): one
 * record per nonzero class value on a kept chain, ascending by (uint32_t) label -- area2 the sum of S(c) over the kept
 * chains with the class on the left minus the sum over those with it on the right (S as in rj_map_eliminate, a
 * two's-complement int128), n_sides the kept chain sides that carry it.  n_points = the edges of the kept chains +
 * n_chains; n_closed: the output chains that are closed walks.
 * All capacities 0 (arrays may be NULL) is the sizing call.  RJ_E_OVERFLOW when a count exceeds its capacity: *counts
 * holds the true counts and nothing is written.  nc == 0 is valid and writes out_row_index_dev[0] = 0 where that pointer is
 * given.  RJ_E_INVALID, with nothing written: the map checks, an unknown flag bit, null arrays, class_dev with
 * n_labels == 0, unmapped labels.  RJ_E_INTERNAL when the budget of 33 doubling rounds runs out (cannot happen).
 * Integers only, exact, fully determined.  Runs on the handle's stream with one host sync, at the end; scratch
 * (rj_dissolve.h: 388 bytes per chain, none per point) is allocated per call and freed; no map, index or option of the
 * handle changes.  For tests and sweeps, through rj_set_debug_option: "dissolve_point_blocks" (0: by size) is the grid of
 * the point scatter; any grid gives the same result.  rj_get_option: "dissolve_last_us0" .. "dissolve_last_us5"
 * (HIP-event microseconds of the stages: check, classes and keep; ends sorted and next; walks; class records; totals
 * and scatter; all; -1: not reached). */
int rj_map_dissolve(rj_handle h, const int64_t* xy_dev, uint64_t np, const uint32_t* row_index_dev,
                    const int32_t* left_dev, const int32_t* right_dev, uint64_t nc,
                    const int32_t* class_dev /* may be NULL */, uint64_t n_labels, uint32_t flags,
                    uint64_t class_capacity, uint64_t chain_capacity, uint64_t point_capacity,
                    rj_diss_class* classes_dev /* may be NULL */, int32_t* out_left_dev, int32_t* out_right_dev,
                    int64_t* out_xy_dev, uint32_t* out_row_index_dev,
                    uint32_t* chain_origin_dev /* may be NULL */, uint32_t* chain_out_dev /* may be NULL */,
                    rj_dissolve_counts* counts);

/* ---- neighbours: which faces touch which, along how much border and at how many nodes ---- */
#define RJ_NB_VERTEX 1u   /* also the nodes: n_nodes of every pair, and the pairs that meet only at a vertex */
typedef struct { int32_t label; uint32_t n_sides, n_edge_nbrs, n_vertex_nbrs; uint64_t area2_lo; int64_t area2_hi;
                 uint64_t perimeter_lo, perimeter_hi, outer_lo, outer_hi; } rj_nb_face; /* 64 bytes */
typedef struct { int32_t label; uint32_t face, n_chains, n_nodes; uint64_t w_lo, w_hi; } rj_nb_entry; /* 32 bytes */
typedef struct { uint64_t n_faces, n_entries, n_edge_pairs, n_vertex_pairs, n_nodes, n_node_pairs_raw,
                 max_labels_at_node; } rj_neighbours_counts;

/* extends: the face adjacency table of a labelled chain map in device memory -- what GIS users know as Polygon
 * Neighbors, and the input of rook and queen contiguity weights, of region growing and of any merge rule other than
 * rj_map_eliminate's longest border.  rj_map_eliminate computes the shared borders for its one rule and throws them
 * away; this call returns them.  (The reference has no counterpart.)
 * Input: xy_dev[2 np], row_index_dev[nc + 1], left_dev[nc], right_dev[nc] with the contract, the checks and the size
 * limits of rj_map_eliminate (a chain may have a single point); labels are any int32.  Under RJ_NB_VERTEX also nc < 2^30.
 * xy_dev is 16-byte aligned (device allocations are): the points are read with 16-byte loads.
 * The definition, in full in rayjoin_amd/csrc/rj_neighbours.h:
 *   faces, their numbering by ascending (uint32_t) label, S(c), L(c) and area2(f) are rj_map_eliminate's; n_sides(f) = the
 *   chain sides that carry f.  Faces f != g, both not 0, are edge neighbours when some chain has {left, right} = {f, g};
 *   w(f, g) = the sum of L(c) over those chains, n_chains(f, g) their number; a pair with w = 0 is still a pair; chains
 *   with left == right add nothing to any length.  perimeter(f) = the sum of L(c) over the chains with left != right and
 *   one side f (the other may be 0), outer(f) the part whose other side is 0: perimeter = outer + the sum of w.
 *   Under RJ_NB_VERTEX a node is a chain end: a distinct point that is the first or the last point of some chain; points
 *   inside a chain are not looked at, so the call is meant for noded maps whose shared vertices are chain ends
 *   (rj_rings_map, rj_map_node, rj_map_snap, rj_map_dissolve); a pseudo-node of degree 2 counts, so rj_map_dissolve with
 *   RJ_DISS_KEEP_EQUAL first for canonical node counts.  F(P) = the nonzero labels on either side of any chain that ends
 *   at P; f != g meet at P when both are in F(P); n_nodes(f, g) = the distinct nodes where they meet; a pair with
 *   n_nodes > 0 and n_chains = 0 is a vertex-only neighbour.  Without the flag no node is looked at: every n_nodes and
 *   n_vertex_nbrs and the counts n_vertex_pairs, n_nodes, n_node_pairs_raw and max_labels_at_node are 0.
 * Output, caller-owned device memory, CSR over the faces: faces_dev[face_capacity] (may be NULL: no records), record k of
 * the k-th face -- label, n_sides, n_edge_nbrs, n_vertex_nbrs (vertex-only neighbours), area2 (a two's-complement
 * int128), perimeter and outer (unsigned 128-bit); offsets_dev[face_capacity + 1]: entry k is where the entries of face k
 * start, entry n_faces is n_entries; entries_dev[entry_capacity]: the neighbour's label and face number, n_chains,
 * n_nodes, w -- ascending by the neighbour's (uint32_t) label within a face, every pair in both directions with equal
 * values.  Counts: the pair counts are unordered; n_node_pairs_raw = the sum over nodes of m (m - 1), m = |F(P)|, which
 * is what the call has to sort; max_labels_at_node the largest m.
 * All capacities 0 (arrays may be NULL) is the sizing call.  RJ_E_OVERFLOW when n_faces > face_capacity or n_entries >
 * entry_capacity: *counts holds the true counts and nothing is written.  nc == 0 is valid and writes offsets_dev[0] = 0
 * where that pointer is given.  RJ_E_INVALID, with nothing written: the map checks, an unknown flag bit, null input
 * arrays or a null counts, a capacity without its array, and n_node_pairs_raw >= 2^32 (*counts holds that count; it
 * saturates at 2^64 - 1; below that limit memory is the practical one, 56 bytes of scratch per raw node pair, and a call
 * that does not get it fails with RJ_E_HIP).  Integers only, exact, fully determined.  Runs on the handle's stream;
 * rook only with one host sync, at the end; with RJ_NB_VERTEX one more, behind the node stage, to read n_node_pairs_raw and size the scratch of
 * the node pairs.  Scratch (rj_neighbours.h has the bytes per chain and per raw node pair) is allocated per call and
 * freed; no map, index or option of the handle changes.  For tests and sweeps, through rj_set_debug_option:
 * "neighbours_point_blocks" (0: by size) is the grid of the pass over the points; any grid gives the same result.
 * rj_get_option: "neighbours_last_us0" .. "neighbours_last_us5" (HIP-event microseconds of the stages: check and chain
 * sums, faces, edge pairs, nodes, the table, all; -1: no call yet, or the last call was refused). */
int rj_map_neighbours(rj_handle h, const int64_t* xy_dev, uint64_t np, const uint32_t* row_index_dev,
                      const int32_t* left_dev, const int32_t* right_dev, uint64_t nc, uint32_t flags,
                      uint64_t face_capacity, uint64_t entry_capacity,
                      rj_nb_face* faces_dev /* may be NULL */, uint64_t* offsets_dev, rj_nb_entry* entries_dev,
                      rj_neighbours_counts* counts);

/* ---- face points: per face the count, the sum, min, max and the members of located points ---- */
#define RJ_FP_MEMBERS 1u  /* also the CSR of the points of every face */
typedef struct { int32_t label; uint32_t first; uint64_t n_points; uint64_t sum_lo; int64_t sum_hi;
                 int64_t min, max; } rj_fp_face; /* 48 bytes */
typedef struct { uint64_t n_faces, n_members, n_outside, n_unmatched, n_runs; } rj_face_points_counts;

/* extends: the other half of a spatial join -- what GIS users know as Summarize Within, Points in Polygon count, or a
 * spatial join with aggregation.  rj_pip_query stops at one int32 per point; this call turns that array into one row
 * per face: how many points, the exact sum, the min and the max of an int64 attribute, and which points.  Its rows are
 * numbered as rj_map_neighbours numbers its faces, so "points per face" and "neighbours of a face" are columns of one
 * table.  (The reference has no counterpart.)
 * Input: label_dev[n], the label of point i < n -- what rj_pip_query wrote to face_id_dev, but any int32 is accepted;
 * n < 2^32.  value_dev (may be NULL: no values): the value of point i is value_dev[i * value_stride], value_stride >= 1
 * in int64 elements; the scaled point array with stride 2, and then that array + 1, give the sums of x and of y (the mean
 * centre per face).  face_label_dev[n_face_labels] (may be NULL), the universe: face k is face_label_dev[k]; the array
 * must ascend strictly in (uint32_t) order of its labels and must not contain 0 -- exactly the label column of
 * rj_map_neighbours' records; it is checked on the device.  Faces without a point appear with n_points = 0.  Without a
 * universe the faces are the distinct nonzero labels among the points, in the same order.
 * The definition, in full in rayjoin_amd/csrc/rj_face_points.h:
 *   per face n_points; sum, a two's-complement int128 (sum_lo, sum_hi), exact; min and max, INT64_MAX / INT64_MIN where the
 *   face has no point or there are no values (every sum is 0 then); first = the smallest point number in the face,
 *   0xFFFFFFFF where there is none.  Counts: n_members = the points whose label is a face, n_outside = the points with
 *   label 0, n_unmatched = the points with a nonzero label that is not in the universe (0 without one):
 *   n_members + n_outside + n_unmatched == n.  n_runs = the number of i with i == 0 || label[i] != label[i - 1]: the
 *   coherence of the point order, which decides the cost of the call.
 * Output, caller-owned device memory: faces_dev[face_capacity] (may be NULL: no records).  Under RJ_FP_MEMBERS
 * offsets_dev[face_capacity + 1] and members_dev[member_capacity]: the point numbers of face k lie at [offsets[k],
 * offsets[k + 1]), ascending, and offsets[n_faces] == n_members.  Without the flag neither array is touched and
 * member_capacity must be 0.
 * All capacities 0 (arrays may be NULL) is the sizing call.  RJ_E_OVERFLOW when n_faces > face_capacity or, under the
 * flag, n_members > member_capacity: *counts holds the true counts and nothing is written.  n == 0 is valid: no faces
 * without a universe, every record empty with one.  RJ_E_INVALID, with nothing written: an unknown flag bit, a null
 * label_dev with n > 0, a null counts, a capacity without its array (face_capacity needs faces_dev, or offsets_dev under
 * the flag; under the flag a face_capacity also needs offsets_dev), member_capacity without the flag, value_stride == 0
 * with values, a universe array that is NULL with n_face_labels > 0, n >= 2^32, n_face_labels >= 2^32 and a bad universe.
 * Integers only, exact, fully determined: the accumulators are integer atomics, which commute, so no grid, wave layout or
 * arrival order changes a result.  Runs on the handle's stream; with a universe one host sync, at the end; without one
 * one more, behind the compaction of the run heads, to size their sort (only the heads are sorted, never all n labels).
 * Scratch (rj_face_points.h has the bytes per face, per run head and per point) is allocated per call and freed; no map,
 * index or option of the handle changes.  For tests and sweeps, through rj_set_debug_option: "face_points_blocks" (0: by
 * size) is the grid of the table pass; any grid gives the same result.  rj_get_option: "face_points_last_us0" ..
 * "face_points_last_us4" (HIP-event microseconds of the stages: universe, table, records, members, all; -1: no call yet,
 * or the last call was refused). */
int rj_face_points(rj_handle h, const int32_t* label_dev, uint64_t n,
                   const int64_t* value_dev /* may be NULL */, uint64_t value_stride,
                   const int32_t* face_label_dev /* may be NULL */, uint64_t n_face_labels,
                   uint32_t flags, uint64_t face_capacity, uint64_t member_capacity,
                   rj_fp_face* faces_dev /* may be NULL */, uint64_t* offsets_dev, uint32_t* members_dev,
                   rj_face_points_counts* counts);
/* label_dev[k] = faces_dev[k].label for k < n_faces: the label column of rj_map_neighbours' records as an array of its
 * own, on the device -- what rj_face_points takes as its universe.  Synchronous, like the memory helpers below. */
int rj_neighbours_labels(rj_handle h, const rj_nb_face* faces_dev, uint64_t n_faces, int32_t* label_dev);

/* ---- nearest: the nearest edge of the base map for every point, and how far it is ---- */
typedef struct { uint32_t eid; uint32_t where; uint64_t num_lo; int64_t num_hi; uint64_t den_lo, den_hi; } rj_near; /* 40 bytes */

/* extends: the third query over the index of rj_build_lbvh, beside "which edge lies above a point" (rj_pip_query) and
 * "which edges cross" (rj_lsi_query): which edge of the base map is nearest to each point, and how far it is -- what GIS
 * users know as Near, sjoin_nearest or a join within a distance.  (The reference has no counterpart.)
 * Points: exactly as rj_pip_query.  pts_dev NULL: the vertices [pt_begin, pt_begin + n) of the query map; otherwise n
 * scaled points of the caller's (pt_begin is ignored), taken in the cached Morton order that rj_pip_query keeps for such
 * arrays where that pays.  The order decides speed only.  n < 2^32.
 * The definition, in full in rayjoin_amd/csrc/rj_nearest.h, in integers only: for the point P and the edge (A, B),
 * l = |B - A|^2 and dot = (P - A) . (B - A);
 *   dot <= 0      where = 1, the first end (also A == B):  d^2 = |P - A|^2
 *   dot >= l      where = 2, the second end:               d^2 = |P - B|^2
 *   otherwise     where = 0, the interior:                 d^2 = c^2 / l with c = (B - A) x (P - A)
 * The nearest edge has the smallest d^2, compared exactly as rationals (up to 285 bits); ties -- the common case: every
 * point nearest to an interior vertex of a chain -- go to the smaller eid.
 * max_dist: negative = unlimited; otherwise an edge qualifies iff d^2 <= max_dist^2, exactly, equality included (the join
 * within a distance); at most 2^48.
 * Output, caller-owned device memory: eid_dev[n], the eid of the nearest qualifying edge, RJ_MISS_EID where there is none.
 * rec_dev[n] (may be NULL): where = 0: (num_lo, num_hi) is the SIGNED cross product c as a two's-complement int128 and
 * (den_lo, den_hi) = l, so d^2 = num^2 / den, and the sign of num tells the side of the edge (positive: left of A -> B);
 * where = 1, 2: num = d^2 and den = 1; a miss: eid = RJ_MISS_EID and everything else 0.  Nothing is divided on the device.
 * dist_dev[n] (may be NULL): sqrt(d^2) in double, within 2^-50 relative of the true value (separate conversions, one
 * multiply, one divide, one square root), +inf on a miss: a convenience, no result depends on it.
 * RJ_E_INVALID, with nothing written: map ids that are not {0, 1} and different, no index on the base map, a null eid_dev
 * with n > 0, a point range outside the query map, n >= 2^32, max_dist > 2^48.  n == 0 is valid and writes nothing.
 * Runs on the handle's stream and is synchronised when it returns.  The result does not depend on the grid, the order
 * of the points, "leaf_order" or any other option.  No map, index or option of the handle changes; the cached point
 * orders are those of rj_pip_query.  rj_get_option: "nearest_last_us0" .. "nearest_last_us2" (HIP-event microseconds of
 * the stages: ordering, traversal, all; -1: no call yet, or the last call was refused or had n == 0).  Under "stats" 1
 * rj_last_stats gives [0] leaf blocks visited, summed over the points (a point visits a block that its bound admits), [1]
 * (point, edge) pairs evaluated exactly, [2] nodes expanded and [3] leaf blocks loaded, both per wave of 64 points.  For tests
 * and sweeps, through rj_set_debug_option: "nearest_blocks" (0: by size) is the grid; any grid gives the same result;
 * "nearest_order_nomem" 1 makes the ordering of the points behave as without memory: the call takes them as given, still
 * returns RJ_OK, and remembers the array (pointer, n) so as not to try again until rj_invalidate or an upload of a map. */
int rj_nearest_query(rj_handle h, int base_map_id, int query_map_id, const int64_t* pts_dev,
                     uint64_t pt_begin, uint64_t n, int64_t max_dist,
                     uint32_t* eid_dev, rj_near* rec_dev /* may be NULL */, double* dist_dev /* may be NULL */);

/* ---- k nearest: the k nearest edges of the base map for every point, in order ---- */
#define RJ_KNEAREST_MAX_K 32

/* extends: rj_nearest_query returns ONE edge, rj_within_query needs a distance that fits no two points alike; this call
 * returns the k nearest edges of every point -- the closest-count field of Near and Generate Near Table, the candidate list
 * of map matching (the three nearest road segments of a GPS fix).  The sixth query over the index of rj_build_lbvh.  (The
 * reference has no counterpart.)
 * Points, pt_begin, n and max_dist: exactly as rj_nearest_query, the cached Morton order and "nearest_order_nomem"
 * included.  1 <= k <= RJ_KNEAREST_MAX_K.
 * The definition, in full in rayjoin_amd/csrc/rj_knearest.h on the functions of rj_nearest.h: order all edges of the base
 * map by (d^2, eid) ascending, d^2 = N / D as in rj_nearest_query and compared exactly, equal distances to the smaller
 * eid; with max_dist >= 0 only edges with N <= max_dist^2 D qualify.  The answer for point i is the first
 * count[i] = min(k, qualifying edges) entries of that order, in that order.  k = 1 gives rj_nearest_query's three arrays bit
 * for bit.
 * Output, caller-owned device memory, row i at the entries [i k, i k + k) (indexed in 64 bits): count_dev[n] (may be NULL);
 * eid_dev[n][k], entry j of row i the (j + 1)-th nearest qualifying edge; rec_dev[n][k] (may be NULL) and dist_dev[n][k]
 * (may be NULL) mean what they mean in rj_nearest_query, dist within 2^-50 relative.  The entries of a row from count[i]
 * on are the miss: RJ_MISS_EID, the record with eid = RJ_MISS_EID and everything else 0, +inf.
 * RJ_E_INVALID, with nothing written: everything rj_nearest_query refuses (map ids that are not {0, 1} and different, no
 * index on the base map, a point range outside the query map, n >= 2^32, max_dist > 2^48), k == 0, k > RJ_KNEAREST_MAX_K,
 * a null eid_dev with n > 0.  n == 0 is valid and writes nothing.  RJ_E_INTERNAL when the traversal's stack overflowed
 * (cannot happen on a tree that rj_build_lbvh accepts).
 * Runs on the handle's stream and is synchronised when it returns.  The result does not depend on the grid, on which wave
 * takes which points, the order of the points, "leaf_order", "query_order", the double filter or the layout of the scratch.
 * No map, index or option of the handle changes; the cached point orders are those of rj_pip_query.
 * Scratch is allocated per call and freed.  It goes by the grid and by k, NOT by n: a list belongs to a wave of the grid,
 * not to a point.  3072 k bytes per wave (64 lists of k slots of 48 bytes), four waves per block, and by size at most four
 * blocks per compute unit -- those that are resident at once: 12 MiB x k on 256 compute units (192 MiB at k = 16, 384 MiB at
 * k = 32) for any number of points, less where n is below 256 points per block of that grid.
 * rj_get_option: "knearest_last_us0" .. "knearest_last_us2" (HIP-event microseconds of the stages: ordering, traversal,
 * all; -1: no call yet, or the last call was refused or had n == 0) and "knearest_last_scratch_bytes" (the scratch of the
 * last call; 0 where the times are -1).  Under "stats" 1 rj_last_stats gives [0] .. [3] as after rj_nearest_query and
 * [4] the candidates that entered a list (at least the sum of the counts).  For tests and
 * sweeps, through rj_set_debug_option: "knearest_blocks" (0: by size) is the grid -- and with it the scratch; any grid
 * gives the same result; "nearest_order_nomem" acts here as in rj_nearest_query.
 * Not here: k above 32 (rj_within_query is the tool there), nearest faces or chains instead of edges, sharding across
 * GPUs. */
int rj_knearest_query(rj_handle h, int base_map_id, int query_map_id, const int64_t* pts_dev,
                      uint64_t pt_begin, uint64_t n, uint32_t k, int64_t max_dist,
                      uint32_t* count_dev /* [n], may be NULL */, uint32_t* eid_dev /* [n][k] */,
                      rj_near* rec_dev /* [n][k], may be NULL */, double* dist_dev /* [n][k], may be NULL */);

/* ---- within: every edge of the base map within a distance of each point, as a CSR ---- */
typedef struct { uint64_t n_pairs, n_points_hit, max_per_point; } rj_within_counts;

/* extends: rj_nearest_query with max_dist says WHETHER an edge lies within the distance of a point; this call says WHICH
 * edges do, all of them -- what GIS users know as dwithin, "Select by distance" or "Generate Near Table (all)": every road
 * segment within 100 m of each address, how many shorelines within 1 km of each station.  The fourth query over the index
 * of rj_build_lbvh and the first whose result is a CSR, the shape that rj_face_points (RJ_FP_MEMBERS) and rj_map_neighbours
 * hand out.  (The reference has no counterpart.)
 * Points: exactly as rj_nearest_query.  pts_dev NULL: the vertices [pt_begin, pt_begin + n) of the query map; otherwise n
 * scaled points of the caller's (pt_begin is ignored), taken in the cached Morton order that rj_pip_query keeps for such
 * arrays where that pays; an ordering that finds no memory leaves the given order.  The order decides speed only.  n < 2^32.
 * The definition, in full in rayjoin_amd/csrc/rj_within.h on the functions of rj_nearest.h: edge e belongs to point i iff
 * d^2 (P_i, e) <= max_dist^2 with d^2 = N / D as in rj_nearest_query, compared exactly (N <= max_dist^2 D), equality
 * included.  A point on an interior vertex of a chain lists both edges k and k + 1: a pair list, not a nearest.
 * 0 <= max_dist <= 2^48; a negative value is refused here, "unlimited" would be n x ne pairs.
 * Output, caller-owned device memory: offsets_dev[n + 1] (may be NULL), eid_dev[pair_capacity]: the eids of point i lie at
 * eid_dev[offsets[i] .. offsets[i + 1]), ASCENDING in eid, offsets[0] == 0 and offsets[n] == n_pairs.  rec_dev[pair_capacity]
 * (may be NULL): the rj_near of pair k -- eid, where, num and den mean what they mean in rj_nearest_query, nothing is
 * divided.  dist_dev[pair_capacity] (may be NULL): sqrt(d^2) in double, within 2^-50 relative.  *counts: n_pairs,
 * n_points_hit = the points with a list that is not empty, max_per_point = the longest list.
 * pair_capacity == 0 is the counting call: eid_dev, rec_dev and dist_dev may be NULL and are not touched, offsets_dev (if
 * given) and *counts are written, RJ_OK -- also the cheap answer to "how many edges within d of each point".
 * RJ_E_OVERFLOW when pair_capacity > 0 and n_pairs > pair_capacity: *counts holds the true counts and offsets_dev (if
 * given) the true offsets; eid_dev, rec_dev and dist_dev are untouched.  n == 0 is valid: the counts are zero and
 * offsets_dev[0] = 0 if given.
 * RJ_E_INVALID, with nothing written, *counts neither: map ids that are not {0, 1} and different, no index on the base map,
 * a null counts, pair_capacity > 0 with a null eid_dev, a point range outside the query map (a wrapping end too),
 * n >= 2^32, pair_capacity >= 2^32, max_dist < 0 or > 2^48.  RJ_E_INTERNAL when the traversal's stack overflowed (cannot
 * happen on a tree that rj_build_lbvh accepts).
 * Runs on the handle's stream and is synchronised when it returns; inside it one more host sync, behind the scan of the
 * counts: the number of pairs sizes the sort.  The result does not depend on the grid, the order of the points,
 * "leaf_order" or any other option: the pairs are found in any order as 64-bit keys (point << 32 | eid) and sorted.  No
 * map, index or option of the handle changes; the cached point orders are those of rj_pip_query.
 * Scratch is allocated per call and freed: 12 bytes per point and 8 bytes per pair of capacity, then 8 bytes per pair found,
 * plus rocPRIM's temporaries of one scan and one radix sort (rayjoin_amd/csrc/rj_within.h); the counting call takes the
 * per-point part only.
 * rj_get_option: "within_last_us0" .. "within_last_us3" (HIP-event microseconds of the stages: ordering, traversal, sort
 * + outputs, all; -1: no call yet, or the last call was refused or had n == 0).  Under "stats" 1 rj_last_stats gives [0]
 * .. [3] as after rj_nearest_query and [4] the pairs appended.  For tests and sweeps, through rj_set_debug_option:
 * "within_blocks" (0: by size) is the grid of the traversal; any grid gives the same result; "nearest_order_nomem" acts
 * here as in rj_nearest_query. */
int rj_within_query(rj_handle h, int base_map_id, int query_map_id, const int64_t* pts_dev,
                    uint64_t pt_begin, uint64_t n, int64_t max_dist, uint64_t pair_capacity,
                    uint64_t* offsets_dev /* [n + 1], may be NULL */, uint32_t* eid_dev /* [pair_capacity] */,
                    rj_near* rec_dev /* [pair_capacity], may be NULL */, double* dist_dev /* [pair_capacity], may be NULL */,
                    rj_within_counts* counts);

/* ---- window: the edges of the base map that meet each rectangle, as a CSR ---- */
typedef struct { uint64_t n_pairs, n_windows_hit, max_per_window; } rj_window_counts;

/* extends: the question every spatial index is asked first -- which edges meet this rectangle: a bounding-box select,
 * sindex.query(box) / .cx[...], the linework of a tile, "which chains does this extent touch, before I clip", a bbox join
 * of a million feature envelopes against a map.  The fifth query over the index of rj_build_lbvh.  (The reference has no
 * counterpart.)
 * Windows: win_dev[nw][4] = (x0, y0, x1, y1) in device memory, in the scaled coordinates of the maps: the CLOSED rectangle
 * [x0, x1] x [y0, y1].  x0 > x1 or y0 > y1 is the empty window: it lists nothing and is no error.  A point and an
 * axis-parallel segment are valid windows.  Coordinates may lie outside the scaled range [-2^46, 2^46): a window is cut to
 * the range first, which changes no result (a window wholly beside the range lists nothing).  nw < 2^32.
 * The definition, in full in rayjoin_amd/csrc/rj_window.h: edge e = (A, B) belongs to window w iff the closed segment and
 * the closed rectangle share a point -- the bounding box of (A, B) overlaps w, and the four corners of w are not all
 * strictly on one side of the line through A and B (cross products in 128 bits, exact).  Touching counts.
 * Output, caller-owned device memory: offsets_dev[nw + 1] (may be NULL), eid_dev[pair_capacity]: the eids of window i lie
 * at eid_dev[offsets[i] .. offsets[i + 1]), ASCENDING in eid, offsets[0] == 0 and offsets[nw] == n_pairs.
 * flags_dev[pair_capacity] (may be NULL): one byte per pair, bit 0: the edge's first point lies in w (closed), bit 1: its
 * second point does -- 3: wholly inside, 0: it passes through or touches with both ends outside, 1 or 2: it leaves
 * through the border; what a clipper needs.  *counts: n_pairs, n_windows_hit = the windows with a list that is not empty,
 * max_per_window = the longest list.
 * pair_capacity == 0 is the counting call: eid_dev and flags_dev may be NULL and are not touched, offsets_dev (if given)
 * and *counts are written, RJ_OK.  RJ_E_OVERFLOW when pair_capacity > 0 and n_pairs > pair_capacity: *counts holds the
 * true counts and offsets_dev (if given) the true offsets; eid_dev and flags_dev are untouched.  nw == 0 is valid: the
 * counts are zero and offsets_dev[0] = 0 if given.
 * RJ_E_INVALID, with nothing written, *counts neither: a base map id that is not 0 or 1, no index on the base map, a null
 * counts, nw > 0 with a null win_dev, pair_capacity > 0 with a null eid_dev, nw >= 2^32, pair_capacity >= 2^32.
 * RJ_E_INTERNAL when the traversal's stack overflowed (cannot happen on a tree that rj_build_lbvh accepts).
 * Runs on the handle's stream and is synchronised when it returns; inside it one more host sync, behind the scan of the
 * counts.  The result depends on no option.  No map, index, option or cached point order of the handle changes.
 * Scratch is allocated per call and freed: 12 bytes per window and 8 bytes per pair of capacity, then 8 bytes per pair
 * found, plus rocPRIM's temporaries of one scan and one radix sort (rayjoin_amd/csrc/rj_window.h); the counting call takes
 * the per-window part only.
 * rj_get_option: "window_last_us0" .. "window_last_us2" (HIP-event microseconds of the stages: traversal, sort + outputs,
 * all; -1: no call yet, or the last call was refused or had nw == 0).  Under "stats" 1 rj_last_stats gives [0] nodes
 * expanded, [1] leaf blocks loaded, [2] pairs tested exactly, [3] pairs handed out by containment (below a box inside
 * the window: no test), [4] pairs appended.  For tests and sweeps, through rj_set_debug_option: "window_blocks" (0: by
 * size) is the grid of the traversal, "window_start_level" (0: by rule, otherwise 1 .. 5, above the tree's top: the top)
 * the level of the tree its work items start at, "window_contained" (1; 0 switches the containment shortcut off); any
 * value of any of them gives the same result.
 * Not here: the faces a window meets, clipping the geometry, sharding across GPUs. */
int rj_window_query(rj_handle h, int base_map_id, const int64_t* win_dev /* [nw][4] */, uint64_t nw,
                    uint64_t pair_capacity, uint64_t* offsets_dev /* [nw + 1], may be NULL */,
                    uint32_t* eid_dev /* [pair_capacity] */, uint8_t* flags_dev /* [pair_capacity], may be NULL */,
                    rj_window_counts* counts);

/* ---- measurement ---------------------------------------------------------------------- */
typedef enum {
  RJ_T_BUILD = 0,     /* whole rj_build_lbvh */
  RJ_T_LSI_KERNEL = 1,/* the LSI traversal+predicate kernel of the last rj_lsi_query* */
  RJ_T_PIP_KERNEL = 2,/* the PIP kernel of the last rj_pip_query* */
  RJ_T_LSI_POINTS = 3,
  RJ_T_SORT = 4,
  RJ_T_ORDER = 5,     /* Morton re-ordering of an incoherent query set inside the last query, if any */
  /* stages of the last rj_build_lbvh (the reference prints its own under -profile,
   * deps/lbvh/lbvh/bvh.cuh:464-474): sort keys, radix sort, leaf pass, upper levels + sibling order */
  RJ_T_BUILD_KEYS = 6,
  RJ_T_BUILD_SORT = 7,
  RJ_T_BUILD_LEAVES = 8,
  RJ_T_BUILD_LEVELS = 9,
  RJ_T_BUILD_RUNS = 11, /* cutting the polyline runs on the device (the first rj_build_lbvh of a map with "leaf_order" 1; inside RJ_T_BUILD) */
  RJ_T_PIP_WALK = 10  /* k_pip_walk, the integer-only first pass of the last rj_pip_query* (RJ_T_PIP_KERNEL spans both passes) */
} rj_timer;
/* HIP-event time (ms) of the last launch of that stage on the handle's stream; syncs. */
int rj_last_ms(rj_handle h, int which, float* ms);
/* every stage at once: ms[i] = rj_last_ms(h, i) for i < n (at most the number of stages), -1 for a stage that has
 * not run -- one call instead of one per stage between two steps of a timed loop */
int rj_last_ms_all(rj_handle h, float* ms, int n);
/* traversal statistics of the last LSI/PIP query (diagnostic; mirrors the reference's
 * "Total tests"/"Visited nodes" debug counters, src/app/lsi_lbvh.h:37-42,93-94):
 * stats[0] = leaf blocks visited, [1] = candidate pairs tested exactly, [2] = nodes expanded,
 * [3] = box tests in the leaf loop; [4..9] = summed per-wave cycle stamps of the instrumented
 * build (total, node expansion, leaf loop, dense predicate phase, merge rounds, max wave total).
 * Collected only after rj_set_option(h,"stats",1), which selects a separate, slower kernel. */
int rj_last_stats(rj_handle h, uint64_t stats[16]);

/* ---- options ---------------------------------------------------------------------------
 * rj_set_option(h, name, value).  NO option changes a result: they choose kernels, leaves and schedules.
 *
 * name               values (default first)   what it does
 * ------------------ ------------------------ ------------------------------------------------------------------------
 * "leaf_order"       1 / 0                    what the NEXT rj_build_lbvh makes a leaf of.  1: polyline runs -- chains
 *                                             stitched through their shared end points by straightest continuation and
 *                                             cut into near-equal runs of <= 64 edges ON THE DEVICE by the first build of
 *                                             an uploaded map (the analogue of the reference's RT grouping,
 *                                             src/rt/primitive.h:120-260); consecutive short runs of the sorted order
 *                                             share a leaf (maps of isolated rings).  0: 64 neighbours along the Hilbert
 *                                             curve.  (Environment RJ_LEAF_ORDER=0 changes the default.)
 * "skyline"          -1 / 0 / 1               the per-x-bucket top of the map that proves a PIP miss without a traversal:
 *                                             -1 built where most chains are closed rings, 0 never, 1 always.
 * "pip_columns"      -1 / 0 / 1               a second index for PIP on the NEXT rj_build_lbvh: the map's runs listed per
 *                                             vertical strip (2^15..2^17 quanta, by the mean width of a segment), sorted by height, with 1024 height buckets
 *                                             per strip -- a query point scans the entries above it in its own strip
 *                                             (k_pip_strip) instead of walking the tree.  -1 built where most chains are
 *                                             closed rings (lakes, parks: many small isolated faces) or where the map's
 *                                             chains are SHORT (mean below 16 edges: fat leaves; measured rule, round 6),
 *                                             0 never, 1 always.  -1 also builds it LATER, at the first PIP query whose point
 *                                             set (>= 2^22 points) turns out spatially incoherent -- the reference's
 *                                             GeneratePIPQueries, uniform random points: the index answers every point on its
 *                                             own where the tree walk first sorts the points and still shares little (8.4 M
 *                                             random points: 1.07 -> 0.70 ms USCounty, 1.9 -> 0.43 LakesNA; that query pays the
 *                                             build).  rj_get_plan's index[].columns_why says which rule applied.
 *                                             A map with a segment over more than 1024 strips (an edge as long as the
 *                                             domain) gets no column index, under 1 too: the build returns RJ_OK, the
 *                                             tree serves the map alone, "pip_columns_used" reads 0 and columns_why
 *                                             says "wanted, not built".
 *                                             (Environment RJ_PIP_COLUMNS=0/1 changes the default: A/B runs.)
 * "leaf_ysort"       1 / 0                    the order inside a leaf block on the NEXT rj_build_lbvh.  Blocks lie sorted by x0 with
 *                                             a bucket table on x (what an upward ray needs).  1: a block TALLER than wide also gets
 *                                             a SECOND order, by y0, with its own table -- a query segment then scans the slots over
 *                                             its y-range (a steep run of a polyline folds back and forth in x: most of its edges lie
 *                                             over every query's x-range); the PIP traversals keep the x order.  8 bytes per slot.
 *                                             0: x order only.  (Environment RJ_LEAF_YSORT=0 changes the default: A/B runs.)
 * "pip_walk"         1 / 0 / 2                a PIP query = k_pip_walk* (integer-only traversal) + k_pip_exact (exact
 *                                             predicate over the candidate lists; its first blocks locate the points
 *                                             whose list overflowed).  1: unless the last query of this size left > 30 %
 *                                             of its points over; 0: k_pip alone; 2: always the passes.
 * "pip_walk_points"  2 / 1                    query points per lane of the walk (k_pip_walk2 / k_pip_walk); 2 applies to
 *                                             query sets that fill 64-position groups.
 * "lsi_segments"     2 / 1                    query segments per lane of the LSI kernel (k_lsi2 / k_lsi); 2 applies to
 *                                             query sets of at least two full groups per resident wave.
 * "lsi_points_split" -1 / 0 / 1               how rj_lsi_points* make the 48-byte records: 1 a gcd-free kernel + the gcd
 *                                             kernel over the pairs it declines, 0 the gcd kernel for every pair, -1 two
 *                                             kernels from 384 Ki pairs on.
 * "query_order"      1 / 0 / 2                re-order a query set along the Morton curve: 1 when consecutive queries are
 *                                             spatially scattered (e.g. the generated workloads of
 *                                             src/run_query.cu:102-167), 0 never, 2 always.
 * "pip_concurrent"   0 / 1 / 2                the caller issues rj_lsi_query_async and rj_pip_query_async in PAIRS (the
 *                                             step of a join: both only read the maps and the index).  1: the two sides
 *                                             share the chip (the LSI kernel on a reduced grid, the PIP kernels on the
 *                                             handle's second stream fill the rest); 2: the handle measures the first
 *                                             four pairs -- taking turns / sharing / sharing with the neighbouring split
 *                                             / beside each other on full grids -- and keeps the fastest from the fifth
 *                                             on (the reference's five warm-up queries settle it), deciding again when
 *                                             the index, a map or the query size changes; 0: every kernel on the whole
 *                                             chip (a caller that issues one kind of query).  The PIP query's inputs must
 *                                             be complete when the call is made; its outputs are complete after rj_sync,
 *                                             rj_pip_query or rj_last_ms(RJ_T_PIP_KERNEL).
 * "pip_exact_stream" 0 / 1                    for a caller that keeps several steps in flight (step k + 1 issued before
 *                                             step k's results are read): the exact kernel of a PIP query that runs on
 *                                             the handle's second stream (see "pip_concurrent") goes to a third stream
 *                                             behind its walk, so the NEXT query's walk starts beside it instead of after
 *                                             it.  Consecutive asynchronous PIP queries must then write to DIFFERENT
 *                                             output arrays (a pipelined caller double-buffers them anyway: step k's
 *                                             answers are still being read); which kernels ran is unchanged.
 * "timers"           1 / 0                    record the stage timers behind rj_last_ms (two event records per stage,
 *                                             ~1 % of a 0.9 ms step); while "pip_concurrent" 2 is still trying schedules
 *                                             they are recorded regardless.
 * "stats"            0 / 1                    the instrumented kernels (visit counters for rj_last_stats; slower).
 * "own_stream"       1                        back to the handle's private stream (see rj_set_stream).
 * A new handle takes the defaults of six from the environment (A/B runs; a value the option refuses keeps the default):
 * RJ_LEAF_ORDER, RJ_LEAF_YSORT, RJ_PIP_COLUMNS, RJ_LSI_SEGMENTS, RJ_WALK_POINTS ("pip_walk_points"), RJ_POINTS_SPLIT ("lsi_points_split").
 * One more has no option behind it: RJ_WALK_SETS = 2 or 3, the 64-position sets a wave of the two-per-lane walk family
 * takes where the walk reads the query map's prepared points beside an LSI query in flight ("pip_concurrent", schedules
 * "shared" and "full grids"; from four 192-position groups per resident wave on).  3: k_pip_walk3_prepared -- 192
 * positions per traversal, five list slots per point and a stack of 76 in the same registers and LDS; 2: k_pip_walk2's
 * 128 everywhere; anything else: the handle's own rule -- see "pip_last_walk_sets".  Caller-owned arrays, re-ordered
 * sets, the instrumented kernel and every query that runs alone take two sets whatever it says.
 *
 * rj_get_option reads any of these, and what the handle did or decided:
 *   "leaf_order_used0/1", "leaf_slots0/1", "leaf_runs0/1", "skyline_used0/1", "closed_chains0/1",
 *   "pip_columns_used0/1", "pip_column_entries0/1", "pip_column_shift0/1", "occ_permille0/1",
 *   "leaf_ysort_used0/1"                                         the index of map 0 / 1
 *   "stitch_rounds", "stitch_loop_ends"                         the last run cutting (pointer-jumping rounds; closed loops)
 *   "pip_schedule" (0 turns, 1 shared, 2 full grids, -1 still trying), "pip_schedule_trials", "pip_schedule_us0/1/2",
 *   "lsi_share_blocks", "pip_share_blocks"                      what "pip_concurrent" 2 measured and settled on
 *   "lsi_last_segments", "pip_last_walk_points", "pip_last_passes", "lsi_points_last_split", "lsi_points_gcd_pairs",
 *   "pip_rest", "pip_rest_aux", "query_last_ordered", "pip_last_columns", "pip_last_prepared",
 *   "pip_last_walk_sets"                                        what the last query ran
 *     ("pip_last_prepared": what the walk read -- 0 the int64 points, 1 the query map's prepared points with a computed
 *     extent per group, 2 prepared points and prepared extents: a range of the query map's own vertices, in their own
 *     order, through k_pip_walk2; extents where pt_begin is a multiple of 64.
 *     "pip_last_walk_sets": 2 or 3, the 64-position sets per wave of the last walk of the k_pip_walk2 family -- see
 *     RJ_WALK_SETS above; left to itself the handle takes the sets RJ_WALK_SETS' default names and goes back to two for
 *     the rest of the epoch when a three-set query leaves far more points to the rest list than two sets did, which
 *     rj_get_plan then says why.  "pip_last_walk_points" is 2 for either, and the plan's first pass names the family,
 *     k_pip_walk2, with the sets beside it)
 *   "comm_ranks"                                                the ranks RCCL counts in the handle's communicator (0: none) */
int rj_set_option(rj_handle h, const char* name, int64_t value);
int rj_get_option(rj_handle h, const char* name, int64_t* value);
/* rj_get_plan: what the handle ran for the last query of each kind and on what grounds, as ONE JSON object (text):
 *   "epoch"     counts the events after which the handle decides again -- rj_upload_map, rj_build_lbvh, another query size,
 *               "pip_concurrent"; every record below carries the epoch it was made in ("current": still that epoch)
 *   "index"     per map: levels, slots, what a leaf is, skyline, column index
 *   "schedule"  of an LSI + PIP pair: the choice ("turns" / "shared" / "full grids" / "undecided"), the trials run, the best
 *               span per schedule, the epoch it was settled in and whether it is in force, the shared grids
 *   "lsi", "records", "pip"   kernel, grid, queries per lane, stream, processing order, passes, and -- where the
 *               handle took another path than the default -- why
 * Once settled a decision stays until the epoch moves.  Host-side state only: no synchronisation, no launch.  The text
 * is written to buf (NUL-terminated, truncated to cap) and its full length to *need; either may be NULL / 0. */
int rj_get_plan(rj_handle h, char* buf, size_t cap, size_t* need);
/* Experiment knobs for tools/ and the fault-path tests -- grids, chunk sizes, run lengths ("chunk_groups",
 * "group_lanes", "max_blocks", "lsi_share_blocks", "pip_share_blocks", "stack_cap", "walk_stack", "strip_shift", "lazy_columns_min",
 * "run_cap", "pack_solo", "pack_spread"; rj_api.hip lists their ranges).  Not needed by a host of the library, never a correctness input,
 * no promise that a name survives a round. */
int rj_set_debug_option(rj_handle h, const char* name, int64_t value);
int rj_get_debug_option(rj_handle h, const char* name, int64_t* value);

/* ---- device memory helpers (for hosts without their own allocator) -------------------- */
int rj_dev_alloc(rj_handle h, size_t bytes, void** out_dev);
int rj_dev_free(rj_handle h, void* dev);
int rj_memcpy_h2d(rj_handle h, void* dst_dev, const void* src, size_t bytes);
int rj_memcpy_d2h(rj_handle h, void* dst, const void* src_dev, size_t bytes);
/* device to device, synchronous like the two above (the faces of a map that go with a thinned copy of it) */
int rj_memcpy_d2d(rj_handle h, void* dst_dev, const void* src_dev, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* RAYJOIN_AMD_H */
