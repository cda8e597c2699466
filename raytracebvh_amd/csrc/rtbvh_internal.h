// rtbvh_internal.h -- host-side launchers shared by the translation units of
// librtbvh.so.  Not part of the public ABI (that is include/rtbvh.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtbvh_device.h"

namespace rtbvh {

// waves per SIMD of the persistent bounce walk (its launch bounds; the full grid is 256 blocks
// of 4 waves per wave/SIMD over the 1,024 SIMDs)
#ifndef RTBVH_BOUNCE_WAVES
#define RTBVH_BOUNCE_WAVES 8
#endif
constexpr uint32_t BOUNCE_WAVES = RTBVH_BOUNCE_WAVES;

// ---- radix sort (sort.hip) --------------------------------------------------
constexpr uint32_t SORT_BLOCK = 256;
#ifndef RTBVH_SORT_ITEMS
#define RTBVH_SORT_ITEMS 16
#endif
constexpr uint32_t SORT_ITEMS = RTBVH_SORT_ITEMS;   // keys per thread of a tile (A/B: 8 / 16 / 32)
constexpr uint32_t SORT_TILE = SORT_BLOCK * SORT_ITEMS;   // 4096 keys per tile
#ifndef RTBVH_RADIX_BITS
#define RTBVH_RADIX_BITS 8
#endif
constexpr uint32_t RADIX_BITS = RTBVH_RADIX_BITS;   // digit width: 8 (4 passes of 30-bit codes) or 10 (3)
constexpr uint32_t RADIX = 1u << RADIX_BITS;
constexpr size_t BOUNDS_WORDS = 8 + 6 * 1024;
constexpr uint32_t ROOTBOX_WORDS = 16;   // BuildArgs::rootbox
constexpr uint32_t ZPART = 3;            // floats per refit workgroup in BuildArgs::zpart

inline uint32_t sort_tiles(uint32_t n) { return (n + SORT_TILE - 1) / SORT_TILE; }
// scratch words needed: RADIX * tiles (per-tile digit counts) + RADIX (digit totals)
inline size_t sort_scratch_words(uint32_t n) { return (size_t)RADIX * sort_tiles(n) + RADIX; }

// Stable LSD sort of (key, val) over bits [0, key_bits), 8-bit digits.  Pass 0
// reads (kin, vin) and writes (ka, va); later passes ping-pong A <-> B, so the
// input is preserved.  Returns where the sorted pairs are (A, or B, or the
// input itself when n == 0).  Result is in A for an odd pass count, else B.
struct SortResult { uint32_t* keys; uint32_t* vals; };
SortResult radix_sort_pairs(const uint32_t* kin, const uint32_t* vin, uint32_t* ka, uint32_t* va, uint32_t* kb,
                            uint32_t* vb, uint32_t n, uint32_t key_bits, uint32_t* scratch, hipStream_t s);

// ---- build (build.hip) ------------------------------------------------------
struct BuildArgs {
    const float4* opos;       // [V]
    const uint32_t* idx;      // [3T]
    const uint32_t* matidx;   // [T] (into the clip triangle's fourth float4 for the shading)
    uint32_t V, T;
    int morton_mode, delta_mode;
    const float* cam;         // [32] device: the camera of the frame, WVP then WV (row-major, row vectors;
                              //   rtbvh_set_camera), read by the kernels -- a captured frame keeps it
    float smin[3], smax[3];   // HLSL-mode scene box
    float* bounds;            // CPUTests mode: [0..5] scene box (min xyz, max xyz), [8..] 1024 x 6 partials
    uint32_t* keys;           // [T] Morton codes (triangle order) -> sort input
    uint32_t* vals;           // [T] triangle ids
    float4* tclip;            // [TCS * T]
    const uint32_t* sorted_keys;  // [T]
    const uint32_t* sorted_vals;  // [T]
    float4* leaf;             // [4T] 64-B sorted leaf records
    Inner* inner;             // [T-1] refit hand-off boxes of nodes spanning workgroups (touched for those only)
    uint4* topo;              // [T-1] Karras node i: child_l, child_r, leaf range [lo, hi] (16 B)
    Inner* rec;               // [2T-1] node records in slots (rtbvh_device.h)
    uint32_t* pleaf;          // [T]
    uint32_t* pint;           // [T-1]
    uint32_t* refit_cnt;      // [T-1]
    uint32_t* xlist;          // [T] k_refit workgroup b's crossing nodes at [b * RBLOCK, ...)
    uint32_t* xcnt;           // [T / RBLOCK + 1] their counts
    float* rootbox;           // [ROOTBOX_WORDS] the root box (min xyz, max xyz), the leaves' depth range and
                              //   [8] the largest leaf edge bound (k_zrange; margin.h).  The region queries
                              //   (trace.hip k_region) rely on words 0..5 being the root node's own box, the
                              //   NaN-dropping union of every leaf box, exactly: they prune and take the whole
                              //   tree on it.  No padding, no finite-only box there (as word 8 is)
    QNode* qnode;             // [2T-1] quantized 4-wide nodes in slots (rtbvh_device.h), from rec
    uint4* lfp;               // [T] leaf footprints on the primary pixel grid (rtbvh_device.h leaf_footprint)
    float* zpart;             // [ZPART * refit_blocks(T)] k_refit workgroup b's leaf depth range, edge bound
    uint32_t pseudo;          // write the leaves' pseudo-records (rec at pleaf[j]; only the packet walks read them)
    uint32_t rec_on;          // write the node records (rec; a certified-only context's build writes none: api.hip)
    uint32_t* qlate;          // [T] or null: k_refit_group's crossing nodes whose QNodes k_qnodes_late builds (count at 0)
    float* nbox;              // [6 (T-1)] or null: internal node k's box (min xyz, max xyz) -- what the certified
                              //   walks' reference-order re-traces and the crossing nodes' QNodes read without records
};
void launch_bounds(const BuildArgs& a, hipStream_t s);
void launch_morton(const BuildArgs& a, hipStream_t s);
// the Morton pass without the codes: the clip-space triangles (tclip) of the current positions and camera, for a
// refit over the last build's sort order and topology (keys and vals are left alone)
void launch_clip(const BuildArgs& a, hipStream_t s);
// A vertex update (rtbvh_update_vertices_async): `count` vertices from `first` on, read from device memory
struct VertexUpdate {
    const float* pos;         // positions, 3 floats each, pos_stride floats apart
    uint32_t pos_stride;
    const float* nrm;         // normals (nrm_stride floats apart), or null: the normals stay
    uint32_t nrm_stride;
    uint32_t first, count;    // count > 0, first + count <= V
    float4* opos;             // [V] BuildArgs::opos
    float* verts;             // [8 V] TraceArgs::verts
    float* bounds;            // CPUTests Morton mode: BuildArgs::bounds, recomputed in stream order; else null
    uint32_t V;
};
void launch_update_vertices(const VertexUpdate& u, hipStream_t s);
// Karras topology (topo, pleaf, pint)
void launch_karras(const BuildArgs& a, hipStream_t s);
// leaf records + refit + node records + QNodes (zeroes the tickets it uses),
// in two parts: the leaves (k_refit: leaf records, footprints, the in-workgroup nodes; then the
// leaves' depth range rootbox[6..7]) -- all the binned primary pass reads -- and the crossing nodes
void launch_refit_leaves(const BuildArgs& a, hipStream_t s);
void launch_refit_tail(const BuildArgs& a, hipStream_t s);
// the leaves' pseudo-records alone, for a tree built without them (a.pseudo = 0)
void launch_pseudo(const BuildArgs& a, hipStream_t s);
// size of BuildArgs::xcnt for T leaves
uint32_t refit_blocks(uint32_t T);
// qnode[k] of every internal node from the record pairs
void launch_qnodes(const BuildArgs& a, hipStream_t s);
// the whole build in one workgroup for T <= small_build_max() (sorted pairs into
// a.sorted_keys / a.sorted_vals, which must be writable)
uint32_t small_build_max();
void launch_build_small(const BuildArgs& a, hipStream_t s);
// the Morton pass and the sort in one workgroup for T <= small_sort_max() (sorted pairs into
// a.sorted_keys / a.sorted_vals, which must be writable); the multi-kernel build's later stages follow
uint32_t small_sort_max();
void launch_morton_sort_small(const BuildArgs& a, hipStream_t s);
// the node records from the topology and the node boxes (a build that wrote none), and the node boxes from the
// records (one that wrote only records)
void launch_records(const BuildArgs& a, hipStream_t s);
void launch_nbox(const BuildArgs& a, hipStream_t s);
// The walk-only tree (build.hip k_wt_*): the built tree's top with every maximal subtree of <= 512
// leaves rebuilt by binned SAH over the same sorted leaves, and its QNodes in slots -- what the certified 4-wide
// bounce walk reads in place of BuildArgs::qnode on a tree that is traced again and again.  Made from the complete
// built tree (topo, pint, the node boxes a.nbox, the crossing nodes' edge bounds in a.inner, the leaf records)
struct WalkTree {
    uint4* topo;        // [T-1] child ids as BuildArgs::topo; z, w: the node's positions in its subtree's leaf order
    uint32_t* pint;     // [T-1]
    float* nbox;        // [6 (T-1)]
    float* edge;        // [T-1] the largest leaf edge bound below the node (margin.h)
    QNode* qnode;       // [2T-1]
    uint32_t* roots;    // [1 + T / 2] the rebuilt subtrees' roots: their count (kept on the device), then the list
};
void launch_walk_tree(const BuildArgs& a, const WalkTree& w, hipStream_t s);
// reference-layout export (44-B Node), 2T-1 entries
void launch_export(const BuildArgs& a, void* out_nodes, hipStream_t s);
// Karras + refit from given sorted codes and leaf boxes (n x 6 floats, device)
void launch_from_codes(const BuildArgs& a, const float* leaf_boxes, hipStream_t s);

// ---- trace (trace.hip) ------------------------------------------------------
struct TraceArgs {
    const Inner* inner;       // node records in slots (BuildArgs::rec); the 4-wide walks read the same array
    // a certified trace's reference-order re-traces walk the topology and the node boxes instead (the context's
    // build may have written no records): nb set, topo = BuildArgs::topo, nbox = BuildArgs::nbox
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;       // [4T] sorted leaf records (see build.hip)
    const float4* tclip;      // [3T] clip-space triangles in triangle order (hit shading)
    const float* verts;       // rtbvh_vertex AoS, 8 floats each
    const uint32_t* idx;
    const uint32_t* matidx;
    const Mat* mats;
    const uint32_t* texels;   // RGBA8 texels of every texture, concatenated (u32 per texel)
    const uint4* texinfo;     // per texture: {first texel, width, height, 0}
    const float* srgb;        // [256] sRGB -> linear (rtbvh_srgb_table)
    uint32_t ntex;
    uint32_t T, W, H, rank, nranks;
    uint32_t band0, bstep;    // this launch traces the rank's bands band0, band0 + bstep, ... (trace chains)
    uint32_t my_bands;        // the rank's bands under the deal (rtbvh_deal_bands)
    const uint32_t* band_list;   // the rank's bands in order (a weighted deal), or null: k * nranks + rank
    const uint32_t* band_slots;  // a weighted deal: band b is rank r's k-th band, slots[b] = r << 24 | k (or null)
    // k_primary behind k_primary_binned: the bins' tile offsets (null: k_primary traces every block),
    // their capacity and the tiles per row
    const uint32_t* pb_gate;
    uint32_t pb_cap, pb_ntx;
    const float* rootbox;     // [6] the BVH root's box (min xyz, max xyz): the bins' depth buckets
    const uint4* lfp;         // [T] leaf footprints (BuildArgs::lfp)
    const float* cam;         // [32] device: WVP, WV (BuildArgs::cam); the shading reads WV
    float4* color;            // output pixels (compacted band rows when nranks > 1)
    float* intensity;         // optional, same indexing as color
    unsigned long long* counters;   // [64] per trace: see flush_counts (trace.hip) and rtbvh_get_stats
    unsigned long long* overflow;   // stack overflows / guard trips, accumulated over every trace (never reset)
    int stack_limit, stack_limit4;  // stack entries the binary / 4-wide primary walks may use (<= STACK_SIZE / STACK4)
    int stack_limit4b;              // ... and the 4-wide bounce walk (<= STACK4B)
    bool limited;                   // a limit below a capacity: the kernels read the limits (else constants)
    bool acyclic;                   // built with the clz64 delta (a radix tree): the 4-wide primary walk
                                    //   needs no walk-length guard
    float* refl_rec;          // optional 14-float RayPresent records (reference reflectRay)
    float* refr_rec;          // optional refractRay records
    const QNode* qnode;       // [2T-1] quantized 4-wide nodes in slots (bounce walk mode 4)
    const QNode* qnode_walk;  // the walk-only tree's (WalkTree::qnode), or null: what a certified 4-wide bounce pass
                              //   walks in place of qnode (same slots' meaning, same leaves; nothing else reads it)
    // N > 1, the binned pass's bins: the leaves whose footprint meets the rank's rows, in PB_LISTS lists (the
    // count pass appends them, the fill pass reads only them; null at N = 1, where every leaf is read):
    // counters PB_LIST_STRIDE words apart, then the lists, pb_list_cap(T) entries each (pb_bin.h)
    uint32_t* pb_list;
};
// primary-ray walks (trace.hip k_primary): per lane in reference order / nearest-first, wave
// packets in reference order / nearest-first, 4-wide wave packets (axis-parallel box test)
enum class PrimaryKind { LANE_REFERENCE, LANE_NEAREST, PACKET_REFERENCE, PACKET_NEAREST, PACKET_WIDE, BINNED };
// bounce walks of the persistent refill kernel (k_bounce_trav)
enum class BounceWalk { REFERENCE, NEAREST, WIDE_QUANTIZED };
void launch_primary(const TraceArgs& a, RayQ* q, uint32_t* qcount, bool count, bool emit, PrimaryKind kind,
                    hipStream_t s);
// A certified trace's re-trace list: the rays of one pass whose certificate failed, and their
// count (zeroed before the pass); the pass's re-trace kernel (reference order) runs over them, REDO_BLOCKS
// workgroups striding over the count on the device
// The certified bounce walk's deferred rays (trace.hip DEFER_*): a clean list of P words per buffer set (readers
// clear what they take) and the pass's work-counter words (its claim and count); null outside bounce passes
struct Redo {
    uint32_t* list;
    uint32_t* count;
    uint32_t* defer = nullptr;
    const uint32_t* dnext = nullptr;
};
constexpr uint32_t REDO_BLOCKS = 512;
// binned primary rays (trace.hip k_primary_binned): the rank's frame in PB_TILE x PB_TILE screen
// tiles (columns x compact band rows), every leaf listed in the tiles its box covers
constexpr uint32_t PB_TILE = 32;
constexpr uint32_t PB_NZ = 16;   // depth buckets per tile: a tile's bins are listed nearest bucket first
constexpr uint32_t PB_LEAVES = 1024;   // the bin passes' leaves per workgroup (pb_bin.h)
constexpr uint32_t PB_LISTS = 16, PB_LIST_STRIDE = 32;   // TraceArgs::pb_list: lists, counter spacing (words)
// entries per list: the leaves of every PB_LISTS-th count block
inline __host__ __device__ uint32_t pb_list_cap(uint32_t T) {
    return ((T + PB_LEAVES - 1) / PB_LEAVES + PB_LISTS - 1) / PB_LISTS * PB_LEAVES;
}
inline size_t pb_list_words(uint32_t T) { return (size_t)PB_LISTS * PB_LIST_STRIDE + (size_t)PB_LISTS * pb_list_cap(T); }
struct PrimBins {
    uint32_t* off;    // [tiles * PB_NZ + 1] leaves per (tile, depth bucket), then their offsets (exclusive
                      //   scan), [tiles * PB_NZ] the total
    uint32_t* cur;    // [tiles * PB_NZ] fill cursors
    uint4* bins;      // [cap] (footprint, leaf) entries, tile by tile, nearest depth bucket first
    unsigned long long* keys;   // [W x rows] the frame's (t, leaf) keys (k_primary_binned -> k_pb_shade)
    uint32_t* sums;   // [tiles * PB_NZ / 1024 + 1] the scan's block totals
    uint32_t cap, ntx, nty;
};
inline uint32_t pb_tiles_x(uint32_t W) { return (W + PB_TILE - 1) / PB_TILE; }
inline uint32_t pb_tiles_y(uint32_t rows) { return (rows + PB_TILE - 1) / PB_TILE; }
// The binned pass (reads what launch_refit_leaves writes; rows = the rank's compact rows), then k_primary (the lane
// walk, launch_pb_gate) behind it for any tile whose bins overflowed `cap` (the whole BVH).  The pass in its two
// parts: the bins (count pass, scan, fill pass: they read the build's leaf footprints,
// the root box's depth range, the frame shape and the band deal, and write pb.off / cur / sums / bins and the rank's
// leaf list -- a product of (tree, frame shape) that api.hip keeps from trace to trace), and the kernels that only
// read them (k_primary_binned, k_primary_redo)
// redo: a certified pass (the shading checks each hit's certificate; the flagged pixels are re-traced)
// small_tiles: 512 threads a tile (a small pass one frame at a time)
void launch_pb_bins(const TraceArgs& a, const PrimBins& pb, uint32_t rows, bool zeroed, hipStream_t s,
                    const BuildArgs* tail = nullptr);
void launch_pb_raster(const TraceArgs& a, const PrimBins& pb, uint32_t rows, RayQ* q, uint32_t* qcount, bool count,
                      bool emit, hipStream_t s, const Redo* redo = nullptr, bool small_tiles = false);
// PrimBins::keys is read and written (an RTBVH_PB_FUSE=0 build: the separate shading launch)
bool pb_keys_used();
// the count pass of launch_pb_bins with the climb of the build's crossing nodes in the same launch,
// then their QNodes (build.hip: the build's launch_refit_tail, moved into the frame)
void launch_pb_count_top(const BuildArgs& b, const TraceArgs& a, uint32_t* off, uint32_t* cur, uint4* bins, uint32_t cap,
                         uint32_t ntx, uint32_t leaf_blocks, hipStream_t s);
// reference: the overflowed tiles in the reference order (a certified trace), else nearest-first
void launch_pb_gate(const TraceArgs& a, const PrimBins& pb, RayQ* q, uint32_t* qcount, bool count, bool emit,
                    hipStream_t s, bool reference);
// up to N arrays of 32-bit words zeroed by one launch (null / 0 words: unused)
struct ZeroList {
    static constexpr int N = 5;
    uint32_t* ptr[N];
    size_t words[N];
};
void launch_zero(const ZeroList& z, hipStream_t s);
// one ray per lane bounce pass (reference order or nearest-first), shading included
void launch_bounce(const TraceArgs& a, const RayQ* qin, const uint32_t* qin_count, const uint32_t* perm, RayQ* qout,
                   uint32_t* qout_count, bool count, bool emit, bool nearest, hipStream_t s);
// bounce pass as persistent refill traversal (hit records) + shading kernel; `next` holds
// NEXT_SEGS zeroed work counters NEXT_STRIDE words apart (one per queue segment);
// `blocks` persistent workgroups (0: 2048)
#ifndef RTBVH_NEXT_SEGS
#define RTBVH_NEXT_SEGS 64
#endif
constexpr uint32_t NEXT_SEGS = RTBVH_NEXT_SEGS;
constexpr uint32_t NEXT_STRIDE = 32;                          // one 128-B line per counter
constexpr uint32_t NEXT_WORDS = 16 * NEXT_SEGS * NEXT_STRIDE;  // per buffer set: bounce passes 0..15
// the certified walk's deferred rays (trace.hip): claim and count words in the pass's first counter line
constexpr uint32_t DEFER_CLAIM = 1, DEFER_COUNT = 2;
constexpr uint32_t DEFER_VALID = 0x80000000u;
// cert: the certified 4-wide walk (WIDE_QUANTIZED, no stack limit, a clz64 tree), whose hit records flag
// the rays it cannot vouch for; the shading with a Redo checks each hit's certificate and re-traces
// the flagged rays in the reference order
// a certified pass's early shading (trace.hip RTBVH_EARLY_SHADE): the outputs k_bounce_shade writes, and the pass's
// largest ray count (the shading workgroups of the walk's launch cover it)
struct BounceShade {
    RayQ* qout;
    uint32_t* qout_count;
    bool emit;
    uint32_t* redo;
    uint32_t* redo_count;
    uint32_t P;
};
void launch_bounce_traverse(const TraceArgs& a, const RayQ* qin, const uint32_t* qin_count, const uint32_t* perm,
                            bool count, BounceWalk walk, float2* hitrec, uint32_t* next, uint32_t blocks,
                            hipStream_t s, bool cert = false, uint32_t* defer = nullptr, const BounceShade* es = nullptr);
void launch_bounce_shade(const TraceArgs& a, const RayQ* qin, const uint32_t* qin_count, const float2* hitrec,
                         RayQ* qout, uint32_t* qout_count, bool count, bool emit, uint32_t P, hipStream_t s,
                         const Redo* redo = nullptr);
// *diff += the number of the n float4 pixels of a and b whose bits differ
// the context's device camera (WVP then WV, 32 floats) written by one dispatch in stream order
struct CameraWords { float w[32]; };
void launch_set_camera(const float* wvp, const float* wv, float* cam, hipStream_t s);
void launch_count_diff(const float4* a, const float4* b, size_t n, unsigned long long* diff, hipStream_t s);
// frame from per-rank compact band buffers (stride_rows rows apart), see rtbvh_assemble_bands
void launch_assemble(const float4* bands, const uint32_t* slots, uint32_t stride_rows, uint32_t W, uint32_t H,
                     uint32_t nranks,
                     float4* frame, hipStream_t s);
// presentation pass (RayTraceBVHPS.hlsl): flipped rows, UNORM8 RGBA
void launch_present(const float4* color, uint32_t W, uint32_t H, uint32_t* out, hipStream_t s);
// coherence sort keys of a bounce queue: P entries (past *count: key 0xFFFFFFFF)
void launch_bounce_keys(const RayQ* q, const uint32_t* count, const float* box, uint32_t P, uint32_t* keys,
                        uint32_t* vals, hipStream_t s);

// ---- ray queries (trace.hip k_query; rtbvh_query_async) ----------------------
// Caller rays (rtbvh_ray: two float4, {origin, t_max}, {direction, reserved}) walked in the reference order on
// the tree form the last build wrote -- the node records, or (nb) the topology and the node boxes -- and one
// rtbvh_hit (a float4: t, u, v, tri) stored per ray at the ray's own index.
struct QueryArgs {
    const Inner* inner;       // node records in slots (BuildArgs::rec), !nb
    const uint4* topo;        // nb: BuildArgs::topo, BuildArgs::nbox
    const float* nbox;
    bool nb;
    const float4* leaf;       // [4T] sorted leaf records
    uint32_t T;
    const float4* rays;       // [2n]
    float4* hits;             // [n]
    uint32_t n;
    const uint32_t* perm;     // walk order (RTBVH_QUERY_SORT: ray perm[k] is the k-th claimed), or null
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_QUERY_COUNT: [4] rays, hits, internal visits, leaf visits (zeroed)
    unsigned long long* overflow;   // the context's overflow word (TraceArgs::overflow)
    int stack_limit;          // <= STACK_SIZE
    // a certified query (RTBVH_QUERY_CERTIFIED, launch_query_certified; null / unused otherwise)
    const uint32_t* n_dev;    // k_query as the re-trace: the ray count on the device (perm: the list; n: its bound)
    const QNode* qnode;       // [2T-1] the quantized 4-wide nodes (BuildArgs::qnode)
    const float4* tclip;      // [TCS * T] the clip-space triangles (the certificate's leaf boxes)
    uint32_t* redo;           // [n] the rays for the reference-order re-trace, and their count (zeroed)
    uint32_t* redo_n;
    uint32_t* next2;          // the re-trace's work counters (as next)
    unsigned long long* walk; // RTBVH_QUERY_COUNT: [3] rays certified, redone, uncovered (zeroed)
};
constexpr uint32_t QUERY_COUNT_WORDS = 4;
// words of a query's scratch block: the work counters, then the count block and the walk counts (8-byte aligned),
// the re-trace list's length, and the re-trace's work counters
constexpr uint32_t QUERY_COUNTS_AT = NEXT_SEGS * NEXT_STRIDE, QUERY_WALK_AT = QUERY_COUNTS_AT + 2 * QUERY_COUNT_WORDS;
constexpr uint32_t QUERY_REDO_N_AT = QUERY_WALK_AT + 2 * QUERY_COUNT_WORDS;
constexpr uint32_t QUERY_NEXT2_AT = QUERY_REDO_N_AT + NEXT_STRIDE;
constexpr uint32_t QUERY_SCRATCH_WORDS = QUERY_NEXT2_AT + NEXT_SEGS * NEXT_STRIDE;
void launch_query(const QueryArgs& a, bool any, bool count, hipStream_t s);
// the certified 4-wide walk (k_query_wide) and the reference-order re-trace of the rays it lists (k_query)
void launch_query_certified(const QueryArgs& a, bool any, bool count, hipStream_t s);
// the coherence keys of caller rays (launch_bounce_keys' scheme over the root box) and vals[i] = i
void launch_query_keys(const float4* rays, uint32_t n, const float* box, uint32_t* keys, uint32_t* vals,
                       hipStream_t s);

// ---- closest-point queries (trace.hip k_nearest; rtbvh_nearest_async) --------
// Caller points (rtbvh_point: one float4, {point, max_dist2}) walked on the tree form the last build wrote, as the
// ray queries', and one rtbvh_nearest (two float4: {point, dist2}, {u, v, tri, 0}) stored per point at its own index.
struct NearestArgs {
    const Inner* inner;       // as QueryArgs
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;
    uint32_t T;
    const float4* points;     // [n]
    float4* out;              // [2n]
    uint32_t n;
    const uint32_t* perm;     // walk order (RTBVH_NEAREST_SORT), or null
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_NEAREST_COUNT: [4] points, found, internal-node steps, leaf steps (zeroed)
    unsigned long long* overflow;   // the context's overflow word
    int stack_limit;          // <= STACK_SIZE
};
// the closest-point queries' own count block, behind the ray queries' scratch words (whose memsets never reach it)
constexpr uint32_t QUERY_NEAREST_AT = QUERY_SCRATCH_WORDS;
static_assert(QUERY_NEAREST_AT % 2 == 0, "the count block's 8-byte words");
void launch_nearest(const NearestArgs& a, bool count, hipStream_t s);
// RTBVH_NEAREST_SORT's keys (the points' 30-bit Morton codes in the root box) and vals[i] = i
void launch_nearest_keys(const float4* points, uint32_t n, const float* box, uint32_t* keys, uint32_t* vals,
                         hipStream_t s);

// ---- radius queries (trace.hip k_within; rtbvh_within_async) -----------------
// The same points on the same tree forms; the output is CSR: a sizes pass stores point r's count at offsets[r + 1],
// scan_offsets turns the counts into offsets, a fill pass stores point r's (triangle, dist2) pairs at
// [offsets[r], min(offsets[r + 1], capacity)).
struct WithinArgs {
    const Inner* inner;       // as QueryArgs
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;
    uint32_t T;
    const float4* points;     // [n]
    unsigned long long* offsets;    // [n + 1]: the sizes pass writes [1, n], the fill pass reads
    uint2* pairs;             // the fill pass: [capacity] {triangle, dist2 bits}
    unsigned long long capacity;
    uint32_t n;
    const uint32_t* perm;     // walk order (RTBVH_WITHIN_SORT), or null
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_WITHIN_COUNT: [4] points, pairs, internal-node steps, leaf steps
    bool count_pairs;         // ... this pass adds the points and pairs (one pass of a call does), not only steps
    unsigned long long* overflow;   // the context's overflow word
    int stack_limit;          // <= STACK_SIZE
};
// the radius queries' own count block, behind the closest-point one
constexpr uint32_t QUERY_WITHIN_AT = QUERY_NEAREST_AT + 2 * QUERY_COUNT_WORDS;
static_assert(QUERY_WITHIN_AT % 2 == 0, "the count block's 8-byte words");
void launch_within(const WithinArgs& a, bool fill, bool count, hipStream_t s);
// sort.hip: offsets[0] = 0 and offsets[1..n] = their inclusive scan, in place, in stream order; `sums`:
// scan_sums_words(n) words of scratch
constexpr uint32_t SCAN_TILE = 2048;   // 256 threads x 8 offsets
inline size_t scan_sums_words(uint32_t n) {
    const size_t t1 = ((size_t)n + SCAN_TILE - 1) / SCAN_TILE, t2 = (t1 + SCAN_TILE - 1) / SCAN_TILE;
    return t1 + t2;
}
void scan_offsets(unsigned long long* offsets, uint32_t n, unsigned long long* sums, hipStream_t s);

// ---- all-hits ray queries (trace.hip k_allhits; rtbvh_allhits_async) ---------
// QueryArgs' rays on the same tree forms, WithinArgs' CSR output: a sizes pass stores ray r's count at
// offsets[r + 1], scan_offsets makes offsets of them, a fill pass stores ray r's hits (float4: t, u, v, tri) at
// [offsets[r], min(offsets[r + 1], capacity)) and, for RTBVH_ALLHITS_BY_T, how many it stored at written[r].
struct AllhitsArgs {
    const Inner* inner;       // as QueryArgs
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;
    uint32_t T;
    const float4* rays;       // [2n]
    unsigned long long* offsets;    // [n + 1]: the sizes pass writes [1, n], the fill pass reads
    float4* hits;             // the fill pass: [capacity]
    unsigned long long capacity;
    uint32_t n;
    const uint32_t* perm;     // walk order (RTBVH_ALLHITS_SORT), or null
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_ALLHITS_COUNT: [4] rays, hits, internal-node steps, leaf steps
    bool count_hits;          // ... this pass adds the rays and hits (one pass of a call does), not only steps
    unsigned long long* overflow;   // the context's overflow word
    int stack_limit;          // <= STACK_SIZE
    uint32_t* written;        // the fill pass of a BY_T call: [n] the hits stored of each ray; else null
};
// the all-hits queries' own count block, behind the radius queries'
constexpr uint32_t QUERY_ALLHITS_AT = QUERY_WITHIN_AT + 2 * QUERY_COUNT_WORDS;
static_assert(QUERY_ALLHITS_AT % 2 == 0, "the count block's 8-byte words");
void launch_allhits(const AllhitsArgs& a, bool fill, bool count, hipStream_t s);
// RTBVH_ALLHITS_BY_T: each ray's stored hits [offsets[r], offsets[r] + written[r]) ordered by (t, tri), in place.
// Lists of up to ALLHITS_LANE_MAX hits are sorted by their ray's lane; the rays with longer ones are listed in
// `list` ([n] words; *list_n zeroed) and sorted one workgroup a list: up to ALLHITS_LDS_MAX hits in LDS, longer
// ones chunk by chunk in LDS with the network's long-distance steps on global memory.
// (The thresholds: DESIGN.md 5f has what was measured.)
#ifndef RTBVH_ALLHITS_LANE_MAX
#define RTBVH_ALLHITS_LANE_MAX 32
#endif
#ifndef RTBVH_ALLHITS_LDS_MAX
#define RTBVH_ALLHITS_LDS_MAX 2048   // 32 KB of LDS
#endif
constexpr uint32_t ALLHITS_LANE_MAX = RTBVH_ALLHITS_LANE_MAX, ALLHITS_LDS_MAX = RTBVH_ALLHITS_LDS_MAX;
void launch_allhits_order(float4* hits, const unsigned long long* offsets, const uint32_t* written, uint32_t n,
                          uint32_t* list, uint32_t* list_n, hipStream_t s);

// ---- box-overlap queries (trace.hip k_overlap; rtbvh_overlap_async) ----------
// Query boxes (two float4 each: {lo.xyz, -}, {hi.xyz, -}) on the same tree forms, WithinArgs' CSR output with a
// triangle id per entry: a sizes pass stores box r's count at offsets[r + 1], scan_offsets makes offsets of them, a
// fill pass stores box r's ids at [offsets[r], min(offsets[r + 1], capacity)).
struct OverlapArgs {
    const Inner* inner;       // as QueryArgs
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;
    uint32_t T;
    const float4* boxes;      // [2n]
    unsigned long long* offsets;    // [n + 1]: the sizes pass writes [1, n], the fill pass reads
    uint32_t* ids;            // the fill pass: [capacity] triangle ids
    unsigned long long capacity;
    uint32_t n;
    const uint32_t* perm;     // walk order (RTBVH_OVERLAP_SORT), or null
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_OVERLAP_COUNT: [4] boxes, ids, internal-node steps, leaf steps
    bool count_ids;           // ... this pass adds the boxes and ids (one pass of a call does), not only steps
    unsigned long long* overflow;   // the context's overflow word
    int stack_limit;          // <= STACK_SIZE
};
// the box queries' own count block, behind the all-hits queries'
constexpr uint32_t QUERY_OVERLAP_AT = QUERY_ALLHITS_AT + 2 * QUERY_COUNT_WORDS;
static_assert(QUERY_OVERLAP_AT % 2 == 0, "the count block's 8-byte words");
void launch_overlap(const OverlapArgs& a, bool fill, bool count, bool tri, hipStream_t s);
// RTBVH_OVERLAP_SORT's keys (the box centres' 30-bit Morton codes in the root box) and vals[i] = i
void launch_overlap_keys(const float4* boxes, uint32_t n, const float* box, uint32_t* keys, uint32_t* vals,
                         hipStream_t s);

// ---- k-nearest queries (trace.hip k_knn; rtbvh_knn_async) --------------------
// NearestArgs' points on the same tree forms; point r's k (triangle, dist2) pairs, ascending in (dist2, triangle),
// at pairs[r * k .. r * k + k), the slots past the number found {0xFFFFFFFF, -1.0f}.
struct KnnArgs {
    const Inner* inner;       // as QueryArgs
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;
    uint32_t T;
    const float4* points;     // [n]
    uint2* pairs;             // [n * k] {triangle, dist2 bits}
    uint32_t n;
    uint32_t k;               // 1 .. KNN_MAX_K
    const uint32_t* perm;     // walk order (RTBVH_KNN_SORT), or null
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_KNN_COUNT: [4] points, pairs found, internal-node steps, leaf steps (zeroed)
    unsigned long long* overflow;   // the context's overflow word
    int stack_limit;          // <= STACK_SIZE
};
constexpr uint32_t KNN_MAX_K = 32;
// the k-nearest queries' own count block, behind the box queries'
constexpr uint32_t QUERY_KNN_AT = QUERY_OVERLAP_AT + 2 * QUERY_COUNT_WORDS;
static_assert(QUERY_KNN_AT % 2 == 0, "the count block's 8-byte words");
// the instance whose list capacity (4, 8, 16 or 32 slots a lane) is the smallest that holds k
void launch_knn(const KnnArgs& a, bool count, hipStream_t s);

// ---- signed-distance queries (trace.hip k_signed; rtbvh_signed_async) --------
// NearestArgs' points on the same tree forms; one rtbvh_signed (two float4: {point, dist2}, {u, v, tri, flags}) per
// point at its own index.  The nearest fields come from launch_nearest into the same records (an rtbvh_nearest's last
// word is 0); launch_signed is the ray pass: the crossing counts of one or three fixed rays, into `flags`.
struct SignedArgs {
    const Inner* inner;       // as QueryArgs
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;
    uint32_t T;
    const float4* points;     // [n]
    float4* out;              // [2n]
    uint32_t n;
    const uint32_t* perm;     // walk order (RTBVH_SIGNED_SORT), or null
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_SIGNED_COUNT: [4] points, points inside, internal-node steps, leaf steps (zeroed)
    unsigned long long* overflow;   // the context's overflow word
    int stack_limit;          // <= STACK_SIZE
};
// the signed-distance queries' own count blocks, behind the k-nearest queries': the ray pass's, then the
// closest-point pass's (launch_nearest's words: points, found, internal-node steps, leaf steps)
constexpr uint32_t QUERY_SIGNED_AT = QUERY_KNN_AT + 2 * QUERY_COUNT_WORDS;
constexpr uint32_t QUERY_SIGNED_NEAR_AT = QUERY_SIGNED_AT + 2 * QUERY_COUNT_WORDS;
static_assert(QUERY_SIGNED_AT % 2 == 0, "the count block's 8-byte words");
// near: launch_nearest stored the nearest fields of these records before (else this pass stores "no result");
// vote3: three rays, else ray 0 alone
void launch_signed(const SignedArgs& a, bool count, bool near, bool vote3, hipStream_t s);

// ---- first-k ray queries (trace.hip k_khits; rtbvh_khits_async) --------------
// AllhitsArgs' rays on the same tree forms; ray r's k hits (float4: t, u, v, tri), ascending in the key
// (max(t, the leaf box's slab entry), tri), at hits[r * k .. r * k + k), the slots past the number found
// {-1, 0, 0, 0xFFFFFFFF}.
struct KhitsArgs {
    const Inner* inner;       // as QueryArgs
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;
    uint32_t T;
    const float4* rays;       // [2n]
    float4* hits;             // [n * k]
    uint32_t n;
    uint32_t k;               // 1 .. KHITS_MAX_K
    const uint32_t* perm;     // walk order (RTBVH_KHITS_SORT), or null
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_KHITS_COUNT: [4] rays, hits found, internal-node steps, leaf steps (zeroed)
    unsigned long long* overflow;   // the context's overflow word
    int stack_limit;          // <= STACK_SIZE
};
constexpr uint32_t KHITS_MAX_K = 16;
// the first-k queries' own count block, behind the signed-distance queries'
constexpr uint32_t QUERY_KHITS_AT = QUERY_SIGNED_NEAR_AT + 2 * QUERY_COUNT_WORDS;
static_assert(QUERY_KHITS_AT % 2 == 0, "the count block's 8-byte words");
// the instance whose list capacity (4, 8 or 16 slots a lane) is the smallest that holds k
void launch_khits(const KhitsArgs& a, bool count, hipStream_t s);

// ---- self-collision queries (trace.hip k_collide; rtbvh_collide_async) -------
// No caller shapes: query k is the leaf at sorted position k, walked against the tree it lies in.  OverlapArgs'
// CSR output indexed by TRIANGLE id: a sizes pass stores the count of the triangle at position k at
// offsets[id + 1], scan_offsets makes offsets of them, a fill pass stores its partners' ids at
// [offsets[id], min(offsets[id + 1], capacity)).
struct CollideArgs {
    const Inner* inner;       // as QueryArgs
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;
    uint32_t T;
    const uint32_t* idx;      // [3T] BuildArgs::idx: rule (N)'s vertex indices, in triangle order
    unsigned long long* offsets;    // [T + 1]: the sizes pass writes [1, T], the fill pass reads
    uint32_t* ids;            // the fill pass: [capacity] triangle ids
    unsigned long long capacity;
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_COLLIDE_COUNT: [4] triangles, entries, internal-node steps, leaf steps
    bool count_ids;           // ... this pass adds the triangles and entries (one pass of a call does), not only steps
    unsigned long long* overflow;   // the context's overflow word
    int stack_limit;          // <= STACK_SIZE
};
// the self-collision queries' own count block, behind the first-k queries'
constexpr uint32_t QUERY_COLLIDE_AT = QUERY_KHITS_AT + 2 * QUERY_COUNT_WORDS;
static_assert(QUERY_COLLIDE_AT % 2 == 0, "the count block's 8-byte words");
// tri: rule (X), the six segment-triangle tests; sym: both triangles of a pair list it
void launch_collide(const CollideArgs& a, bool fill, bool count, bool tri, bool sym, hipStream_t s);

// ---- triangle queries (trace.hip k_cross; rtbvh_cross_async, rtbvh_cross_first_async) -------
// Query triangles (three float4 each: {v0.xyz, -}, {v1.xyz, -}, {v2.xyz, -}) on the same tree forms.  The sizes
// and fill passes are OverlapArgs' CSR output indexed by query; the first pass stores at first[r] the id of the
// first member its walk meets, or 0xFFFFFFFF, and ends the walk there.
enum CrossPass { CROSS_PASS_SIZES = 0, CROSS_PASS_FILL = 1, CROSS_PASS_FIRST = 2 };
struct CrossArgs {
    const Inner* inner;       // as QueryArgs
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;
    uint32_t T;
    const float4* tris;       // [3n]
    unsigned long long* offsets;    // [n + 1]: the sizes pass writes [1, n], the fill pass reads
    uint32_t* ids;            // the fill pass: [capacity] triangle ids
    uint32_t* first;          // the first pass: [n]
    unsigned long long capacity;
    uint32_t n;
    const uint32_t* perm;     // walk order (RTBVH_CROSS_SORT), or null
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_CROSS_COUNT: [4] queries, ids, internal-node steps, leaf steps
    bool count_ids;           // ... this pass adds the queries and ids (one pass of a call does), not only steps
    unsigned long long* overflow;   // the context's overflow word
    int stack_limit;          // <= STACK_SIZE
};
// the triangle queries' own count block, behind the self-collision queries'
constexpr uint32_t QUERY_CROSS_AT = QUERY_COLLIDE_AT + 2 * QUERY_COUNT_WORDS;
static_assert(QUERY_CROSS_AT % 2 == 0, "the count block's 8-byte words");
void launch_cross(const CrossArgs& a, CrossPass pass, bool count, hipStream_t s);
// RTBVH_CROSS_SORT's keys (the 30-bit Morton codes, in the root box, of the query boxes' centres) and vals[i] = i
void launch_cross_keys(const float4* tris, uint32_t n, const float* box, uint32_t* keys, uint32_t* vals,
                       hipStream_t s);

// ---- clearance queries (trace.hip k_clearance; rtbvh_clearance_async) -------
// CrossArgs' query triangles on the same tree forms, one bound for the call, and one rtbvh_clearance (two float4:
// {point_q, dist2}, {point_x, tri}) stored per query at its own index.
struct ClearanceArgs {
    const Inner* inner;       // as QueryArgs
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;
    uint32_t T;
    const float4* tris;       // [3n]
    float max_dist2;
    float4* out;              // [2n]
    uint32_t n;
    const uint32_t* perm;     // walk order (RTBVH_CLEARANCE_SORT), or null
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_CLEARANCE_COUNT: [4] queries, found, internal-node steps, leaf steps (zeroed)
    unsigned long long* overflow;   // the context's overflow word
    int stack_limit;          // <= STACK_SIZE
};
// the clearance queries' own count block, behind the triangle queries'
constexpr uint32_t QUERY_CLEARANCE_AT = QUERY_CROSS_AT + 2 * QUERY_COUNT_WORDS;
static_assert(QUERY_CLEARANCE_AT % 2 == 0, "the count block's 8-byte words");
void launch_clearance(const ClearanceArgs& a, bool count, hipStream_t s);

// ---- region queries (trace.hip k_region; rtbvh_region_async) -----------------
// Regions (six float4 each: plane i {n.xyz, d}) on the same tree forms, OverlapArgs' CSR output: a sizes pass
// stores region r's count at offsets[r + 1], scan_offsets makes offsets of them, a fill pass stores its ids at
// [offsets[r], min(offsets[r + 1], capacity)).  topo is read in both tree forms: an accepted subtree's leaf range.
struct RegionArgs {
    const Inner* inner;       // as QueryArgs
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;
    uint32_t T;
    const float* rootbox;     // BuildArgs::rootbox: [0..5] the root's own box
    const float4* regions;    // [6n]
    unsigned long long* offsets;    // [n + 1]: the sizes pass writes [1, n], the fill pass reads
    uint32_t* ids;            // the fill pass: [capacity] triangle ids
    unsigned long long capacity;
    uint32_t n;
    bool accept;              // take subtrees whole (not RTBVH_REGION_NO_ACCEPT) ...
    const uint32_t* leaf_nan; // ... while this word, launch_leaf_nan's for the current tree, is 0
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_REGION_COUNT: [6] regions, ids, internal-node steps, leaf steps,
                                    //   accepted subtrees, ids from accepts
    bool count_ids;           // ... this pass adds the regions, ids and ids from accepts (one pass of a call does)
    unsigned long long* overflow;   // the context's overflow word
    int stack_limit;          // <= STACK_SIZE
};
// the region queries' own count block (six words), behind the clearance queries', and the leaf-NaN word behind it
constexpr uint32_t REGION_COUNT_WORDS = 6;
constexpr uint32_t QUERY_REGION_AT = QUERY_CLEARANCE_AT + 2 * QUERY_COUNT_WORDS;
constexpr uint32_t QUERY_LEAF_NAN_AT = QUERY_REGION_AT + 2 * REGION_COUNT_WORDS;
// the split region queries' own count block (three 8-byte words: non-empty pieces, the expansion's node tests, the
// longest piece walk), behind the leaf-NaN word
constexpr uint32_t REGION_SPLIT_COUNT_WORDS = 3;
constexpr uint32_t QUERY_REGION_SPLIT_AT = QUERY_LEAF_NAN_AT + 2;
constexpr uint32_t QUERY_REGION_SPLIT_END = QUERY_REGION_SPLIT_AT + 2 * REGION_SPLIT_COUNT_WORDS;
static_assert(QUERY_REGION_AT % 2 == 0 && QUERY_REGION_SPLIT_AT % 2 == 0, "the count block's 8-byte words");
void launch_region(const RegionArgs& a, bool fill, bool count, bool tri, hipStream_t s);

// ---- split region queries (trace.hip k_region_expand, k_region_piece; the split field of rtbvh_region_async) ----
// A region is cut along the tree into at most K = 1 << kshift pieces, slots [r * K, r * K + K) of `pieces` in
// leaf-range order.  A piece {a, b}: b == 0 EMPTY; b == REGION_PIECE_NODE the subtree of walk node a (LEAF_BIT | j:
// the one leaf j), walked like a region from its own node; any other b the leaf range [a, a + b) taken whole.
// k_region_expand writes them (one wave a region); k_region_piece walks one piece a lane: its sizes pass stores
// piece p's count at poff[p + 1], scan_offsets makes offsets of them, launch_region_offsets copies every K-th into
// the caller's offsets, and its fill pass stores piece p's ids from offsets[r] + (poff[p] - poff[r * K]).
constexpr uint32_t REGION_PIECE_NODE = 0xFFFFFFFFu;
constexpr uint32_t REGION_SPLIT_MAX_SHIFT = 12;         // K <= 4096: the frontier's two lists fill 64 KB of LDS
constexpr uint32_t REGION_SPLIT_MAX_PIECES = 1u << 20;  // n * K <= this: RTBVH_REGION_SPLIT_MAX_PIECES (api.hip)
constexpr uint32_t REGION_SPLIT_ROUNDS = 64;            // the expansion's rounds: each expands one node at least
struct RegionSplitArgs {
    RegionArgs r;             // r.n regions; r.offsets the caller's
    uint2* pieces;            // [n << kshift]
    unsigned long long* poff; // [(n << kshift) + 1]
    uint32_t kshift;
    unsigned long long* split;      // RTBVH_REGION_COUNT: [3] non-empty pieces, the expansion's node tests, the
                                    //   longest piece walk (zeroed)
};
void launch_region_expand(const RegionSplitArgs& a, bool count, hipStream_t s);
void launch_region_piece(const RegionSplitArgs& a, bool fill, bool count, bool tri, hipStream_t s);
// offsets[r] = poff[r << kshift], r = 0 .. n
void launch_region_offsets(const unsigned long long* poff, unsigned long long* offsets, uint32_t n, uint32_t kshift,
                           hipStream_t s);
// *word (zeroed by the caller) = 1 if any of the T leaf records holds a NaN in its box words 10..15
void launch_leaf_nan(const float4* leaf, uint32_t T, uint32_t* word, hipStream_t s);

// ---- sphere-sweep queries (trace.hip k_sweep; rtbvh_sweep_async) -------------
// Sweeps (two float4 each: {origin, t_max}, {direction, radius}) on the same tree forms, and one rtbvh_sweep_hit
// (two float4: {t, point}, {tri, feature, 0, 0}) stored per sweep at its own index.
struct SweepArgs {
    const Inner* inner;       // as QueryArgs
    const uint4* topo;
    const float* nbox;
    bool nb;
    const float4* leaf;
    uint32_t T;
    const float4* sweeps;     // [2n]
    float4* hits;             // [2n]
    uint32_t n;
    const uint32_t* perm;     // walk order (RTBVH_SWEEP_SORT), or null
    uint32_t* next;           // NEXT_SEGS zeroed work counters NEXT_STRIDE words apart
    unsigned long long* counts;     // RTBVH_SWEEP_COUNT: [4] sweeps, hits, internal-node steps, leaf steps (zeroed)
    unsigned long long* overflow;   // the context's overflow word
    int stack_limit;          // <= STACK_SIZE
};
// the sweep queries' own count block, at the end of the scratch block (behind the split region queries')
constexpr uint32_t QUERY_SWEEP_AT = QUERY_REGION_SPLIT_END;
constexpr uint32_t QUERY_ALLOC_WORDS = QUERY_SWEEP_AT + 2 * QUERY_COUNT_WORDS;   // the whole scratch block
static_assert(QUERY_SWEEP_AT % 2 == 0, "the count block's 8-byte words");
void launch_sweep(const SweepArgs& a, bool any, bool count, hipStream_t s);

}  // namespace rtbvh
