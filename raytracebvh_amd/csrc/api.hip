// api.hip -- the C ABI of librtbvh.so (include/rtbvh.h): context, device
// buffers, stream ordering and the host sequence of Graphics::computeBVH
// (Graphics.cpp:667-831), re-done as one HIP stream of kernels with no per-frame
// queue/allocator/fence creation and no host round trip inside build or trace.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rtbvh.h"
#include "rtbvh_internal.h"

using namespace rtbvh;

#ifndef RTBVH_MAXSPLIT
#define RTBVH_MAXSPLIT 4
#endif

// Move-only owners of what the context allocates: a handle, released by Del when its owner goes.  They convert
// to the handle, so launch sites read as with raw pointers; out() is for the HIP call that creates the handle.
template <typename H, void (*Del)(H)>
struct Owner {
    H h{};
    Owner() = default;
    Owner(Owner&& o) noexcept : h(o.h) { o.h = H{}; }
    Owner& operator=(Owner&& o) noexcept {
        std::swap(h, o.h);
        return *this;
    }
    ~Owner() { reset(); }
    void reset() {
        if (h) Del(h);
        h = H{};
    }
    H* out() {
        reset();
        return &h;
    }
    operator H() const { return h; }
};
template <typename T> void del_device(T* p) { (void)hipFree((void*)p); }
template <typename T> void del_pinned(T* p) { (void)hipHostFree((void*)p); }
inline void del_event(hipEvent_t e) { (void)hipEventDestroy(e); }
inline void del_stream(hipStream_t s) {
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
}
template <typename T>
struct DevBuf : Owner<T*, del_device<T>> {   // alloc: frees first; a count of 0 allocates one element
    hipError_t alloc(size_t count) { return hipMalloc((void**)this->out(), (count ? count : 1) * sizeof(T)); }
};
template <typename T>
struct Pinned : Owner<T*, del_pinned<T>> {
    hipError_t alloc(size_t count) {
        return hipHostMalloc((void**)this->out(), count * sizeof(T), hipHostMallocDefault);
    }
};
using Event = Owner<hipEvent_t, del_event>;
using Stream = Owner<hipStream_t, del_stream>;
// A device buffer grown on demand, with the capacity it was allocated for: {null, 0} before the first reserve and
// after one that failed, so a capacity never vouches for a pointer that is not there (the next call tries again).
// What else a growth means -- a captured frame to drop, a wait for the readers of the old buffer, a memset of
// the new one -- belongs to the call site: `if (!b.has(n)) { ...; HIPC(c, b.reserve(n)); ... }`.
template <typename T>
struct Grown {
    DevBuf<T> buf;
    size_t cap = 0;   // elements
    bool has(size_t n) const { return n == 0 || (n <= cap && buf); }   // (no element needs no buffer)
    hipError_t reserve(size_t n) {   // frees first, like DevBuf::alloc
        if (has(n)) return hipSuccess;
        const hipError_t e = buf.alloc(n);
        if (e != hipSuccess) buf.h = nullptr;
        cap = e == hipSuccess ? n : 0;
        return e;
    }
    void reset() {
        buf.reset();
        cap = 0;
    }
    operator T*() const { return buf.h; }
};

// The forms of the built tree a walk or a reader may ask for (Tree::valid, ensure_form)
enum Form : uint32_t { RECORDS = 1, NBOX = 2, PSEUDO = 4, QNODES = 8 };
// The built tree.  A build assigns it whole, set_scene and build_from_codes reset it, and a replayed graph
// (compute_graph) restores the record its capture ended with: the replayed build rewrote the tree.
struct Tree {
    bool built = false;
    bool clz64 = false;      // built with the clz64 delta: a valid tree (no cycles)
    Form wrote = RECORDS;    // the node form the build wrote: records, or (a certified-only context's) node boxes;
                             //   the other is derived on first use
    uint32_t valid = 0;      // the forms that are complete now: node records (the binary and packet walks'), node
                             //   boxes (a certified trace's reference-order re-traces), the leaf pseudo-records
                             //   (the packet walks') and the QNodes (the 4-wide bounce walk's)
};

// RTBVH_FLAG_BINNED_PRIMARY: a bin set -- tile counts / offsets, fill cursors, the bins and the rank's leaf
// list (trace.hip k_pb_bin) -- is a product of the built tree and the frame shape, like the leaf footprints it
// is made from: the two bin passes and the scan read nothing else (PbKey), and every kernel behind them only
// reads the set.  So a set records the key it was filled for, and a later binned trace with the same key, on any
// stream, uses it as it is (find_bins) instead of zeroing and filling its own: one fill per build and frame
// shape, and one set in memory for all the frames in flight.  A trace that finds none fills the set of its own
// trace buffer set (prepare_walks).  RTBVH_BINS_REUSE=0: every trace fills its own set (A/B).
struct PbKey {
    uint64_t build = 0;           // bins_epoch of the fill: the tree whose footprints and depth range it read
    uint32_t W = 0, H = 0, rows = 0, rank = 0, nranks = 0, T = 0, ntx = 0, nty = 0;
    uint32_t share = 0;           // the band deal (root_share; 16 with one rank: no deal) ...
    const uint32_t* deal = nullptr;   // ... and its device table (null: round-robin, computed in the kernel)
    bool operator==(const PbKey& o) const {
        return build == o.build && W == o.W && H == o.H && rows == o.rows && rank == o.rank &&
               nranks == o.nranks && T == o.T && ntx == o.ntx && nty == o.nty && share == o.share &&
               deal == o.deal;
    }
};
struct PbBufs {
    DevBuf<uint32_t> off, cur, sums;
    DevBuf<uint4> bins;
    uint32_t cap_T = 0, cap_tiles = 0, cap_bins = 0;   // (cap_bins is what the fill clipped at: the readers' `cap`)
    Grown<uint32_t> list;       // N > 1: the rank's leaves (TraceArgs::pb_list)
    PbKey key;                  // what the set holds, when `valid`
    bool valid = false;
    Event filled;               // recorded behind the fill pass: a reader on another stream waits for it
    uint32_t readers = 0;       // trace buffer sets whose traces have read the set since its fill (bit k: set k)
};

// The walk-only tree (rtbvh_internal.h WalkTree) is a product of the built tree alone, like a bin
// set: it records the tree it was made from (`epoch`: bins_epoch, which everything that rewrites leaf records, node
// boxes or topology bumps -- a build, a replayed build, a refit, set_scene, build_from_codes; a vertex update makes
// the tree stale until one of them).  Made on the context stream before the third certified bounce trace of a
// build (`passes`): two traces on the built tree's QNodes cost nothing extra, and a tree traced a third time is
// taken as static.  `ready` is recorded behind its QNode pass: a reader on another stream waits for it.  Its
// buffers are overwritten only for a later tree, whose build has waited for every trace that read them.
// Never made or used inside a graph capture.  RTBVH_WALK_TREE=0: never; =1: before the first trace.
struct WalkTreeBufs {
    Grown<uint4> topo;
    Grown<uint32_t> pint, roots;
    Grown<float> nbox, edge;
    Grown<QNode> qnode;
    bool valid = false;
    uint64_t epoch = 0;        // when valid: the tree it is of
    uint32_t T = 0;
    Event ready;
    uint64_t seen_epoch = 0;   // the tree whose certified bounce traces `passes` counts
    uint32_t passes = 0;
    void reset() {
        topo.reset(); pint.reset(); roots.reset(); nbox.reset(); edge.reset(); qnode.reset();
        valid = false;
    }
};

// A trace buffer set: everything one primary -> bounce chain writes.  Set 0 is the context stream's; set b >= 1
// is chain b of a context-stream trace dealt over chains (the rank's bands over `nsplit` chains on their own
// streams, so one chain's kernel tail overlaps the others' work), or the set of a caller stream with frames in
// flight (rtbvh_trace_band_async on a stream other than the context's): such traces run concurrently over the
// one BVH, wait only for the last build (ev_built) and the next build waits for them (`done`).  A context does
// one or the other (slots_used).
struct TraceSet {
    // `chain` stands first: destroyed after the set's buffers and events.  Across sets and the rest of the
    // context the order does not matter: a chain is joined into the trace's stream before the trace ends, and
    // rtbvh_destroy drains the context stream and every caller stream's frame before anything goes.
    Stream chain;                   // chain b's stream (b >= 1), created on first use
    Event join;                     //   ... joined into the trace's stream
    hipStream_t caller = nullptr;   // the caller stream that owns the set (b >= 1), from its first trace on
    Event done;                     //   recorded behind its last trace
    bool busy = false;              //   ... which no build has waited for yet
    DevBuf<RayQ> q[2];              // the bounce queues, ping-pong: set 0's hold cap_P rays, the others cap_split
    DevBuf<float2> hit;             // per queued bounce ray: (t, leaf | INVALID)
    // the certified walks: the rays a pass re-traces in the reference order (their counts:
    // qcount 16..31), and the bounce walk's deferred rays (trace.hip DEFER_*), kept clean
    Grown<uint32_t> redo, defer;
    PbBufs pb;
    Grown<unsigned long long> pbkeys;   // an RTBVH_PB_FUSE=0 build's (t, leaf) keys: a result, so per set
    // its parts of the context's shared blocks (consecutive sets' parts are consecutive: one launch_zero covers
    // a trace's chains), set where the blocks are allocated
    uint32_t* qcount = nullptr;             // [32] of d_qcount: queue counts [0..15], re-trace counts [16..31]
    uint32_t* next = nullptr;               // [NEXT_WORDS] of d_next: segmented bounce work counters
    unsigned long long* counters = nullptr; // [64] of d_counters: see rtbvh_get_stats
    unsigned long long* ovf = nullptr;      // its word of h_ovf
};

// What the readbacks and rtbvh_get_stats know of the last trace.  enqueue_walks assigns it whole; a replayed
// graph (compute_graph) restores the record its capture ended with.
struct LastTrace {
    bool traced = false;
    uint32_t W = 0, H = 0, bounces = 0, rank = 0, nranks = 1;
    uint32_t nsplit = 1;             // its chains
    uint32_t slot = 0;               // its buffer set (the counters there are the stats)
    size_t rec_P = 0;                // pixels with ray records (RTBVH_FLAG_REFRACT_RECORDS), or 0
    uint32_t walk = 0;               // its walk flags
    uint32_t walk_state = 0;         // rtbvh_stats.walk_state
    bool cert = false;               // certified (its re-trace counts)
    bool frame_here = false;         // d_color holds its whole frame
    bool intensity_here = false;     // d_intensity holds its intensities
    bool walk_tree = false;          // its certified bounce passes walked the walk-only tree
};

// ---- the query chain ---------------------------------------------------------------------------------
// Every rtbvh_*_async query entry, of whatever kind and on whatever stream, is one link of one chain.  The rules:
//  - Shared: the scratch block (the walks' work counters at its head, then one count block a kind: KINDS) and
//    the buffers grown on demand -- the walk order's sort, the offset scan's block sums, the certified ray
//    query's re-trace list, RTBVH_ALLHITS_BY_T's lists, a split region query's pieces.  So a link runs alone.
//  - Waits: a link waits on its stream for `ev`, recorded behind the link before it (`busy`: since the last
//    build or host drain), and -- on a stream other than the context's -- for the last build (ev_built).  The
//    next writer of the tree waits for `ev` (wait_queries); the host drains wait for it (sync_all).
//  - Growth: a shared buffer is reallocated only after hipEventSynchronize(ev): earlier links use the old
//    one.  The first link that needs a buffer and each larger one wait on the host there (reserve_shared).
//  - Counts: a counting link zeroes and fills its kind's block only and sets counted[kind]; a link that does
//    not count leaves every block alone.  The *_counts readers wait for `ev` and read one block.
//  - Overflows: `ovf` says a link ran since the last rtbvh_synchronize, which then looks at the overflow word.
// What a caller gets when several arguments are wrong is fixed too: query_rules.
enum Kind : uint32_t {
    K_QUERY, K_NEAREST, K_WITHIN, K_ALLHITS, K_OVERLAP, K_KNN, K_SIGNED, K_KHITS, K_COLLIDE, K_CROSS, K_CLEARANCE,
    K_REGION, K_REGION_SPLIT, K_SWEEP, K_KINDS
};
struct KindRow {
    uint32_t at, words;        // its count block: QueryChain::scratch + at, 8-byte words
    const char* not_ready;     // what its reader answers before a counting query
};
constexpr KindRow KINDS[K_KINDS] = {
    {QUERY_COUNTS_AT, QUERY_COUNT_WORDS, "no RTBVH_QUERY_COUNT query yet"},
    {QUERY_NEAREST_AT, QUERY_COUNT_WORDS, "no RTBVH_NEAREST_COUNT query yet"},
    {QUERY_WITHIN_AT, QUERY_COUNT_WORDS, "no RTBVH_WITHIN_COUNT query yet"},
    {QUERY_ALLHITS_AT, QUERY_COUNT_WORDS, "no RTBVH_ALLHITS_COUNT query yet"},
    {QUERY_OVERLAP_AT, QUERY_COUNT_WORDS, "no RTBVH_OVERLAP_COUNT query yet"},
    {QUERY_KNN_AT, QUERY_COUNT_WORDS, "no RTBVH_KNN_COUNT query yet"},
    {QUERY_SIGNED_AT, 2 * QUERY_COUNT_WORDS, "no RTBVH_SIGNED_COUNT query yet"},   // the ray pass's, the closest-point pass's
    {QUERY_KHITS_AT, QUERY_COUNT_WORDS, "no RTBVH_KHITS_COUNT query yet"},
    {QUERY_COLLIDE_AT, QUERY_COUNT_WORDS, "no RTBVH_COLLIDE_COUNT query yet"},
    {QUERY_CROSS_AT, QUERY_COUNT_WORDS, "no RTBVH_CROSS_COUNT query yet"},
    {QUERY_CLEARANCE_AT, QUERY_COUNT_WORDS, "no RTBVH_CLEARANCE_COUNT query yet"},
    {QUERY_REGION_AT, REGION_COUNT_WORDS, "no RTBVH_REGION_COUNT query yet"},
    {QUERY_REGION_SPLIT_AT, REGION_SPLIT_COUNT_WORDS, "no counting region query with a split field yet"},
    {QUERY_SWEEP_AT, QUERY_COUNT_WORDS, "no RTBVH_SWEEP_COUNT query yet"},
};
static_assert(QUERY_SIGNED_NEAR_AT == QUERY_SIGNED_AT + 2 * QUERY_COUNT_WORDS, "the signed queries' two blocks are one");
struct QueryChain {
    DevBuf<uint32_t> scratch;                // [QUERY_ALLOC_WORDS]: the work counters, the ray queries' words, KINDS' blocks
    Grown<uint32_t> sort;                    // a walk order: 6 arrays of cap / 6 words (keys and values: in, A, B),
    Grown<uint32_t> sort_scratch;            //   and the sort's digit counts
    Grown<uint32_t> redo;                    // RTBVH_QUERY_CERTIFIED: the re-trace list
    Grown<unsigned long long> scan;          // the offset scan's block sums
    Grown<uint32_t> order;                   // RTBVH_ALLHITS_BY_T: 2 arrays of cap / 2 words (each ray's stored hits, the
                                             //   rays with long lists)
    Grown<uint2> pieces;                     // split region queries: the pieces, their offsets and that scan's
    Grown<unsigned long long> poff, pscan;   //   block sums
    Event ev;                                // ev_query: recorded behind the last link
    bool busy = false;                       // ... which no build or host drain has waited for yet
    bool ovf = false;                        // a link ran since the last rtbvh_synchronize (its overflows)
    bool counted[K_KINDS] = {};              // the kind's count block holds a counting query's counts
    uint64_t fallback = 0;                   // K_QUERY: its rays, when it took the present kernel for all of them; or 0
    uint64_t split_k = 0;                    // K_REGION_SPLIT: its K
    // The region queries' leaf-NaN word (scratch + QUERY_LEAF_NAN_AT) is a product of the built tree, like a bin
    // set: written on the stream of the first region query of a tree (nan_epoch: its bins_epoch), with ev_nan
    // recorded behind it for the region queries of that tree on other streams
    uint64_t nan_epoch = 0;
    Event ev_nan;
};

struct rtbvh_ctx {
    rtbvh_config cfg{};
    // Members are destroyed last to first: the streams the context created stand first, so they outlive every
    // buffer and event below (rtbvh_destroy has drained them by then).  The chains' streams: TraceSet.
    Stream own_stream, side;
    static constexpr uint32_t MAXSPLIT = RTBVH_MAXSPLIT;   // buffer sets: the context stream's + chains / caller streams
    TraceSet sets[MAXSPLIT];
    hipStream_t stream = nullptr;   // the context stream: the caller's (cfg.stream) or own_stream
    std::string err;

    // scene (set_scene)
    uint32_t V = 0, T = 0, nmat = 0;
    DevBuf<float4> d_opos;
    DevBuf<float> d_verts;
    DevBuf<uint32_t> d_idx, d_matidx;
    DevBuf<Mat> d_mats;
    float wvp[16], wv[16];
    DevBuf<float> d_cam;        // [32] the kernels' camera (BuildArgs::cam): WVP, WV, uploaded in stream order
    bool cam_dirty = false;     //   (sync_camera) when set_camera changed it
    bool have_scene = false, have_camera = false;
    Tree tree;
    // Vertex updates (rtbvh_update_vertices_async), on any stream: they write d_opos, d_verts and the mesh box.
    // The next build or refit waits for the last one (ev_update, wait_update); until then the built tree is not
    // of the geometry (stale): traces and queries are refused, the readbacks return the last build's tree.
    Event ev_update;
    bool update_pending = false;   // ev_update recorded and no build, refit or update has waited for it yet
    bool stale = false;

    // build buffers (capacity cap_T)
    uint32_t cap_T = 0;
    DevBuf<uint32_t> d_codes, d_ids, d_ka, d_va, d_kb, d_vb, d_sort_scratch;
    DevBuf<float4> d_tclip, d_leaf;
    Grown<float4> d_band;                    // rtbvh_trace_tiles: this rank's bands; rank 0: all ranks'
    DevBuf<Inner> d_inner;                   // box hand-off of refit nodes spanning workgroups
    DevBuf<uint4> d_topo;                    // Karras node: child ids + leaf range
    DevBuf<Inner> d_rec;                     // node records in slots (rtbvh_device.h), 2T-1
    DevBuf<QNode> d_qnode;                   // quantized 4-wide nodes in slots (rtbvh_device.h), 2T-1
    DevBuf<uint4> d_lfp;                     // leaf footprints on the primary pixel grid (binned primary pass)
    DevBuf<uint32_t> d_texels;               // textures (rtbvh_texture), concatenated RGBA8
    DevBuf<uint4> d_texinfo;
    DevBuf<float> d_srgb;
    uint32_t ntex = 0;
    Grown<float> d_refl_rec;                 // RTBVH_FLAG_REFRACT_RECORDS: reflectRay / refractRay
    Grown<float> d_refr_rec;                 //   RayPresent records, 14 floats per traced pixel
    DevBuf<uint32_t> d_pleaf, d_pint, d_cnt;
    DevBuf<uint32_t> d_xlist, d_xcnt;        // refit: crossing nodes per workgroup
    DevBuf<uint32_t> d_qlate;                // BuildArgs::qlate
    DevBuf<unsigned long long> d_ovf;        // stack overflows + guard trips of every trace (never reset)
    Pinned<unsigned long long> h_ovf;        // pinned: a snapshot of *d_ovf copied at the end of each trace,
                                             //   one word per buffer set (TraceSet::ovf); ovf_seen: the value last reported
    unsigned long long ovf_seen = 0;
    DevBuf<float> d_bounds, d_rootbox, d_zpart;
    // rtbvh_compute_bvh: the binned primary pass of the frame starts on `side` once the build's
    // leaves are written (ev_leaf, between k_zrange and k_refit_group) and joins the context stream
    // (ev_prim) before the walk of its overflowed tiles, which reads the whole BVH
    Event ev_leaf, ev_prim;
    DevBuf<float> d_nbox;        // [6 (T-1)] internal node boxes
    // rtbvh_compute_bvh: the build leaves its crossing nodes (launch_refit_tail) to the frame's binned
    // pass, which runs them in its bin launches (launch_pb_bin_tail); any other first use of the tree
    // runs them first (flush_tail).  The two *_pending are the build's hand-off to the trace (build_tree's
    // Handoff), reset with `tree`
    bool tail_pending = false;
    bool leaf_pending = false;   // ev_leaf recorded and nothing enqueued on the stream since
    SortResult sorted{nullptr, nullptr};

    // trace buffers (capacity cap_P pixels; with them set 0's queues and hit records)
    size_t cap_P = 0;
    DevBuf<float4> d_color;
    DevBuf<float> d_intensity;
    DevBuf<uint32_t> d_bkin, d_bvin, d_bka, d_bva, d_bkb, d_bvb, d_bscratch;   // bounce coherence sort
    // one block each for all the sets (TraceSet::qcount, next, counters)
    DevBuf<uint32_t> d_qcount;                // [32 x MAXSPLIT]
    DevBuf<uint32_t> d_next;                  // [NEXT_WORDS x MAXSPLIT]
    DevBuf<unsigned long long> d_counters;    // [64 x MAXSPLIT]
    size_t cap_split = 0;                     // rays per queue of the sets 1.. (ensure_split_capacity)
    Event ev_fork;                            // a trace dealt over chains: they start behind it
    uint64_t bins_epoch = 1;        // bumped whenever the leaf footprints are (or are about to be) rewritten
    uint64_t bin_builds = 0;        // count passes launched (rtbvh_bin_builds)
    bool knob_bins_reuse = true;    // RTBVH_BINS_REUSE
    WalkTreeBufs wt;                // the walk-only tree, freed with the build buffers
    int knob_walk_tree = -1;        // RTBVH_WALK_TREE: 0 never, 1 before the first trace, else before the third
    uint64_t walk_tree_builds = 0;
    LastTrace last;

    // hipEvent rings: per build 6 events (before bounds, after bounds/morton/sort/karras/refit),
    // per trace 3 (before primary, after primary, after bounces)
    static constexpr int RING = 32;
    Event evb[RING][6];
    Event evt[RING][5];             // trace start, primary done, end, first bounce traversal start/end
    bool evt_trav[RING] = {};
    uint32_t n_builds = 0, n_traces = 0;   // timed samples since reset
    // ev_built: the tree and every form marked valid in `tree` are complete (order_after_context): what a trace
    // or a query on a caller stream waits for
    Event ev_built;
    bool slots_used = false;  // a caller stream has a buffer set: trace chains are off
    // RTBVH_FLAG_GRAPH: the captured frame (build + trace) of rtbvh_compute_bvh and its key
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    uint64_t graph_key[5] = {};
    bool capturing = false;   // enqueueing into a capture: no event records
    uint64_t graph_captures = 0;
    // host-side state of the captured frame, restored after every replay: its trace, and the tree it leaves
    // (its build's, with the forms its trace derived)
    LastTrace graph_trace;
    Tree graph_tree;
    uint64_t cert_traces = 0;                         // certified traces so far
    // RTBVH_FLAG_AUTO_WALK at <= AUTO_WALK_MAX_TRIS: the primary kind, the reference order's lanes or its
    // wave packets (the same frame), timed on this scene and frame size (enqueue_trace)
    uint64_t small_key = 0;
    uint32_t small_flags = 0;     // the flags the small-scene primary kind was timed under
    bool small_packet = false;
    Event ev_small[2];            // its timing events (created on first use)
    // tuning knobs of A/B runs, read once by rtbvh_create (RTBVH_BOUNCE_BLOCKS, RTBVH_OVERLAP,
    // RTBVH_SIDE_PRIORITY): a shipped context does not change its launches per frame
    uint32_t knob_bounce_blocks = 0;
    bool knob_overlap = false, knob_side_priority = true, knob_keep_records = false, knob_no_early_shade = false,
         knob_no_small_tiles = false;
    // the band deal of band traces (rtbvh_set_band_deal): rank 0's weight in 1/16 of another rank's
    uint32_t root_share = 16;
    struct DealTab {   // a weighted deal's device table: every rank's bands, then slots[b] = r << 24 | pos
        uint32_t H, nranks, share;
        DevBuf<uint32_t> d;
        std::vector<uint32_t> off;   // rank r's bands at d[off[r] .. off[r + 1])
        Pinned<uint32_t> h;          // its pinned staging copy (the upload is asynchronous; freed with d)
        Event ready;                 // recorded after the upload on the context stream
    };
    std::deque<DealTab> deals;       // the MAX_DEALS most recently used (H, nranks, share), most recent first
    static constexpr size_t MAX_DEALS = 8;
    QueryChain q;                    // the queries' shared state (above): last, so gone before every stream
};

namespace {

std::string g_create_error;

rtbvh_status fail(rtbvh_ctx* c, rtbvh_status st, const std::string& msg) {
    if (c) c->err = msg;
    else g_create_error = msg;
    return st;
}

#define HIPC(ctx, expr)                                                                          \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail(ctx, _e == hipErrorOutOfMemory ? RTBVH_ERR_OOM : RTBVH_ERR_HIP,          \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                      \
    } while (0)
// ... and of a step that has recorded its own failure
#define TRY(expr)                                      \
    do {                                               \
        if (rtbvh_status _st = (expr)) return _st;     \
    } while (0)

// A captured frame (RTBVH_FLAG_GRAPH) holds the device pointers of capture time: every
// reallocation below drops it, so a replay never writes to a freed buffer.
void drop_graph(rtbvh_ctx* c) {
    if (c->graph_exec) (void)hipGraphExecDestroy(c->graph_exec);
    if (c->graph) (void)hipGraphDestroy(c->graph);
    c->graph_exec = nullptr;
    c->graph = nullptr;
}

// No tree: the buffers of the built one are about to be rewritten (set_scene, build_from_codes)
void reset_tree(rtbvh_ctx* c) {
    c->tree = Tree{};
    c->stale = false;
    c->bins_epoch++;   // (no bin set is of the next tree)
    c->tail_pending = c->leaf_pending = false;
}

rtbvh_status check_launch(rtbvh_ctx* c, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, RTBVH_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return RTBVH_OK;
}

// ---- stream ordering ---------------------------------------------------------------------------------
// The frames in flight on caller streams, drained on the host
rtbvh_status drain_slots(rtbvh_ctx* c) {
    for (TraceSet& t : c->sets)
        if (t.busy) HIPC(c, hipEventSynchronize(t.done));
    return RTBVH_OK;
}
// ... with the context stream and the ray queries: the one host drain
rtbvh_status sync_all(rtbvh_ctx* c) {
    HIPC(c, hipStreamSynchronize(c->stream));
    TRY(drain_slots(c));
    if (c->q.busy) HIPC(c, hipEventSynchronize(c->q.ev));
    if (c->update_pending) HIPC(c, hipEventSynchronize(c->ev_update));   // (a vertex update on a caller stream)
    return RTBVH_OK;
}

// The next writer of what the frames in flight read (a build: the BVH; a camera upload) on stream s waits for them
rtbvh_status wait_slots(rtbvh_ctx* c, hipStream_t s) {
    for (TraceSet& t : c->sets)
        if (t.busy) {
            HIPC(c, hipStreamWaitEvent(s, t.done, 0));
            t.busy = false;
        }
    return RTBVH_OK;
}

// The next writer of the BVH on stream s (a build) waits for the outstanding ray queries, which read it.  (Never
// inside a capture: rtbvh_compute_bvh's plain frame before it has cleared q.busy.)
rtbvh_status wait_queries(rtbvh_ctx* c, hipStream_t s) {
    if (c->q.busy) {
        HIPC(c, hipStreamWaitEvent(s, c->q.ev, 0));
        c->q.busy = false;
    }
    return RTBVH_OK;
}

// The next reader or writer of the vertices and the mesh box on stream s (a build, a refit, another update) waits
// for the last vertex update.  (Never inside a capture: rtbvh_compute_bvh's plain frame before it has waited.)
rtbvh_status wait_update(rtbvh_ctx* c, hipStream_t s) {
    if (c->update_pending) {
        HIPC(c, hipStreamWaitEvent(s, c->ev_update, 0));
        c->update_pending = false;
    }
    return RTBVH_OK;
}
// What a trace or a query answers between a vertex update and the next build or refit
rtbvh_status fail_stale(rtbvh_ctx* c, const char* what) {
    return fail(c, RTBVH_ERR_NOT_READY,
                std::string(what) + ": the vertices were updated after the last build -- the tree is not of this "
                                    "geometry until rtbvh_build, rtbvh_refit or rtbvh_compute_bvh");
}

// Stream s is ordered after what the context stream holds now.  ev_built is recorded again every time (not inside
// a capture, whose nodes are ordered by the capture), so it keeps meaning "the tree and every form marked valid
// are complete" for every later caller stream, which waits for it alone (rtbvh_trace_band_async).
rtbvh_status order_after_context(rtbvh_ctx* c, hipStream_t s) {
    if (!c->capturing) HIPC(c, hipEventRecord(c->ev_built, c->stream));
    if (s != c->stream) HIPC(c, hipStreamWaitEvent(s, c->ev_built, 0));
    return RTBVH_OK;
}

rtbvh_status ensure_build_capacity(rtbvh_ctx* c, uint32_t T) {
    if (T <= c->cap_T && c->d_codes) return RTBVH_OK;
    drop_graph(c);
    reset_tree(c);   // (its buffers go)
    c->wt.reset();
    const size_t n = T, ni = T > 1 ? T - 1 : 1;
    HIPC(c, c->d_codes.alloc(n));
    HIPC(c, c->d_ids.alloc(n));
    HIPC(c, c->d_ka.alloc(n));
    HIPC(c, c->d_va.alloc(n));
    HIPC(c, c->d_kb.alloc(n));
    HIPC(c, c->d_vb.alloc(n));
    HIPC(c, c->d_sort_scratch.alloc(sort_scratch_words(T)));
    HIPC(c, c->d_tclip.alloc(TCS * n));
    HIPC(c, c->d_leaf.alloc(4 * n));
    HIPC(c, c->d_inner.alloc(ni));
    HIPC(c, c->d_topo.alloc(ni));
    HIPC(c, c->d_rec.alloc(2 * (size_t)n - 1));
    HIPC(c, c->d_nbox.alloc(6 * (size_t)ni));
    HIPC(c, c->d_qnode.alloc(2 * (size_t)n - 1));
    HIPC(c, c->d_lfp.alloc(n));
    HIPC(c, c->d_pleaf.alloc(n));
    HIPC(c, c->d_pint.alloc(ni));
    HIPC(c, c->d_cnt.alloc(ni));
    HIPC(c, c->d_xlist.alloc(n));
    HIPC(c, c->d_qlate.alloc(n + 1));
    HIPC(c, c->d_xcnt.alloc(refit_blocks(T)));
    HIPC(c, c->d_zpart.alloc(ZPART * (size_t)refit_blocks(T)));
    HIPC(c, c->d_bounds.alloc(BOUNDS_WORDS));
    HIPC(c, c->d_rootbox.alloc(ROOTBOX_WORDS));
    c->cap_T = T;
    return RTBVH_OK;
}

rtbvh_status ensure_trace_capacity(rtbvh_ctx* c, size_t P) {
    if (P <= c->cap_P && c->d_color) return RTBVH_OK;
    drop_graph(c);
    HIPC(c, c->d_color.alloc(P));
    HIPC(c, c->d_intensity.alloc(P));
    HIPC(c, c->sets[0].q[0].alloc(P));
    HIPC(c, c->sets[0].q[1].alloc(P));
    HIPC(c, c->d_bkin.alloc(P));
    HIPC(c, c->d_bvin.alloc(P));
    HIPC(c, c->d_bka.alloc(P));
    HIPC(c, c->d_bva.alloc(P));
    HIPC(c, c->d_bkb.alloc(P));
    HIPC(c, c->d_bvb.alloc(P));
    HIPC(c, c->d_bscratch.alloc(sort_scratch_words((uint32_t)P)));
    HIPC(c, c->sets[0].hit.alloc(P));
    if (!c->d_qcount) HIPC(c, c->d_qcount.alloc(32 * rtbvh_ctx::MAXSPLIT));
    if (!c->d_next) HIPC(c, c->d_next.alloc((size_t)NEXT_WORDS * rtbvh_ctx::MAXSPLIT));
    if (!c->d_counters) HIPC(c, c->d_counters.alloc(64 * rtbvh_ctx::MAXSPLIT));
    for (uint32_t b = 0; b < rtbvh_ctx::MAXSPLIT; b++) {   // (the blocks stay where they are from here on)
        c->sets[b].qcount = c->d_qcount + 32 * b;
        c->sets[b].next = c->d_next + (size_t)NEXT_WORDS * b;
        c->sets[b].counters = c->d_counters + 64 * b;
    }
    c->cap_P = P;
    return RTBVH_OK;
}

// chains of a trace (enqueue_trace): RTBVH_FLAG_SPLIT_SHIFT bits, 0 = automatic
uint32_t trace_split(const rtbvh_ctx* c) {
    const uint32_t v = (c->cfg.flags >> RTBVH_FLAG_SPLIT_SHIFT) & 7u;
    if (v) return v < rtbvh_ctx::MAXSPLIT ? v : rtbvh_ctx::MAXSPLIT;
    return 1;
}

// The sets 1 .. nsets - 1 (a trace's chains, or the caller streams' sets up to this trace's) with queues of `rays`
// rays, and the chains' streams and events
rtbvh_status ensure_split_capacity(rtbvh_ctx* c, uint32_t nsets, size_t rays) {
    if (nsets < 2) return RTBVH_OK;
    const bool grow = rays > c->cap_split;
    if (grow) {
        drop_graph(c);   // every set's queues hold cap_split rays: drop the smaller ones
        TRY(drain_slots(c));   // (after any frame in flight on them)
        c->cap_split = rays;
        for (uint32_t g = nsets; g < rtbvh_ctx::MAXSPLIT; g++) {
            TraceSet& t = c->sets[g];
            t.q[0].reset(); t.q[1].reset(); t.hit.reset();
        }
    }
    for (uint32_t g = 1; g < nsets; g++) {
        TraceSet& t = c->sets[g];
        if (!t.chain) HIPC(c, hipStreamCreateWithFlags(t.chain.out(), hipStreamNonBlocking));
        if (!t.join) HIPC(c, hipEventCreateWithFlags(t.join.out(), hipEventDisableTiming));
        if (!c->ev_fork) HIPC(c, hipEventCreateWithFlags(c->ev_fork.out(), hipEventDisableTiming));
        if (t.q[0] && !grow) continue;
        HIPC(c, t.q[0].alloc(c->cap_split));
        HIPC(c, t.q[1].alloc(c->cap_split));
        HIPC(c, t.hit.alloc(c->cap_split));
    }
    return RTBVH_OK;
}

// Binned primary buffers of a buffer set for T leaves and `tiles` screen tiles.  The bins hold
// BINS_PER_LEAF entries per leaf (C5: 1.37 tiles per leaf); a tile whose bins would pass the end is
// traced by the 4-wide packet walk instead (trace.hip pb_gate), so the capacity is a speed knob only.
constexpr uint32_t BINS_PER_LEAF = 3;
rtbvh_status ensure_pb_capacity(rtbvh_ctx* c, PbBufs& p, uint32_t T, uint32_t tiles) {
    const uint32_t bins = BINS_PER_LEAF * T + 16 * tiles;
    if (T <= p.cap_T && tiles <= p.cap_tiles && bins <= p.cap_bins && p.off) return RTBVH_OK;
    drop_graph(c);
    p.valid = false;   // (its buffers go; the free waits for the device, so for every reader)
    const uint32_t nT = std::max(T, p.cap_T), nt = std::max(tiles, p.cap_tiles);
    const uint32_t nb = std::max(BINS_PER_LEAF * nT + 16 * nt, p.cap_bins);
    HIPC(c, p.off.alloc((size_t)nt * PB_NZ + 1));
    HIPC(c, p.cur.alloc((size_t)nt * PB_NZ));
    HIPC(c, p.sums.alloc((size_t)nt * PB_NZ / 1024 + 1));
    HIPC(c, p.bins.alloc(nb));
    p.cap_T = nT;
    p.cap_tiles = nt;
    p.cap_bins = nb;
    return RTBVH_OK;
}

// The buffer set whose bin set is filled for `key`, if the context has one, or -1.  The key holds everything the bin
// passes and the scan read: the tree (bins_epoch: the leaf footprints and the root box's depth range, both written
// by the build alone), T, the frame shape, the rank's rows and the band deal.  Not the camera: the passes read it only
// through the footprints, which a camera upload without a build leaves as they are (the frame then still shows the
// tree of the last build, whose clip-space triangles the walks read).  Not the walk flags, the counters or the
// overflow word: no bin kernel reads them.  Never inside a capture: a captured frame holds its own bin passes, so
// that its replay depends on no host state.
int find_bins(const rtbvh_ctx* c, const PbKey& key) {
    if (!c->knob_bins_reuse || c->capturing) return -1;
    for (uint32_t k = 0; k < rtbvh_ctx::MAXSPLIT; k++) {
        const PbBufs& p = c->sets[k].pb;
        if (p.valid && p.off && p.key == key) return (int)k;
    }
    return -1;
}

BuildArgs build_args(rtbvh_ctx* c) {
    BuildArgs a{};
    a.opos = c->d_opos;
    a.idx = c->d_idx;
    a.matidx = c->d_matidx;
    a.V = c->V;
    a.T = c->T;
    a.morton_mode = (int)c->cfg.morton_mode;
    a.delta_mode = (int)c->cfg.delta_mode;
    a.cam = c->d_cam;
    memcpy(a.smin, c->cfg.scene_bb_min, 12);
    memcpy(a.smax, c->cfg.scene_bb_max, 12);
    a.bounds = c->d_bounds;
    a.keys = c->d_codes;
    a.vals = c->d_ids;
    a.tclip = c->d_tclip;
    a.sorted_keys = c->sorted.keys;
    a.sorted_vals = c->sorted.vals;
    a.leaf = c->d_leaf;
    a.inner = c->d_inner;
    a.topo = c->d_topo;
    a.rec = c->d_rec;
    a.pleaf = c->d_pleaf;
    a.pint = c->d_pint;
    a.refit_cnt = c->d_cnt;
    a.xlist = c->d_xlist;
    a.qlate = c->d_qlate;
    a.xcnt = c->d_xcnt;
    a.rootbox = c->d_rootbox;
    a.qnode = c->d_qnode;
    a.lfp = c->d_lfp;
    a.zpart = c->d_zpart;
    // the leaf pseudo-records cost the build 0.64 GB of writes at 10M triangles: written when the
    // context's walks include a packet primary walk (AUTO and the binned pass take none)
    // (choose_walks: a packet primary walk iff PACKET_PRIMARY without BINNED_PRIMARY)
    const uint32_t f = c->cfg.flags;
    a.pseudo = (f & RTBVH_FLAG_PACKET_PRIMARY) &&
               !(f & (RTBVH_FLAG_BINNED_PRIMARY | RTBVH_FLAG_AUTO_WALK | RTBVH_FLAG_CERTIFIED));
    // the last build's outputs: node records, or (a certified-only context's) node boxes instead
    const bool boxes = c->tree.wrote == NBOX;
    a.rec_on = boxes ? 0u : 1u;
    a.nbox = boxes ? c->d_nbox.h : nullptr;
    return a;
}

// ---- the band deal ----------------------------------------------
// The frame's 8-row bands b = 0 .. ceil(H / 8) - 1 go to the ranks by smooth weighted round-robin:
// rank 0 has weight `share`, every other rank 16; for each band every rank's credit grows by its
// weight, and the rank with the most credit (the lowest on a tie) takes the band and pays the
// total weight.  share 16 deals b -> b % nranks exactly; below 16, rank 0 -- which also receives
// and assembles the other ranks' bands -- traces share / 16 of another rank's bands, spread evenly
// over the frame (the centre-heavy hit distribution stays balanced).
void deal_owners(uint32_t H, uint32_t nranks, uint32_t share, std::vector<uint32_t>& owner) {
    const uint32_t nb = (H + 7) / 8;
    owner.assign(nb, 0);
    if (nranks <= 1) return;
    std::vector<int64_t> credit(nranks, 0);
    const int64_t total = (int64_t)share + 16 * (int64_t)(nranks - 1);
    for (uint32_t b = 0; b < nb; b++) {
        uint32_t best = 0;
        for (uint32_t r = 0; r < nranks; r++) {
            credit[r] += r == 0 ? share : 16;
            if (credit[r] > credit[best]) best = r;
        }
        credit[best] -= total;
        owner[b] = best;
    }
}
uint32_t band_height(uint32_t H, uint32_t b) { return (H - b * 8) < 8 ? (H - b * 8) : 8; }
uint32_t deal_rows(uint32_t H, uint32_t rank, uint32_t nranks, uint32_t share) {
    if (nranks == 0 || rank >= nranks) return 0;
    if (share == 16 || nranks == 1) {
        uint32_t rows = 0;
        for (uint32_t b = rank; b * 8 < H; b += nranks) rows += band_height(H, b);
        return rows;
    }
    std::vector<uint32_t> owner;
    deal_owners(H, nranks, share, owner);
    uint32_t rows = 0;
    for (uint32_t b = 0; b < owner.size(); b++)
        if (owner[b] == rank) rows += band_height(H, b);
    return rows;
}
uint32_t deal_max_rows(uint32_t H, uint32_t nranks, uint32_t share) {
    uint32_t m = 0;
    for (uint32_t r = 0; r < nranks; r++) m = std::max(m, deal_rows(H, r, nranks, share));
    return m;
}
// The device table of a weighted deal (null for round-robin: the kernels compute it).  Uploaded on
// first use (a few KB, once per frame size and deal), so not from inside a graph capture (whose frames
// have one rank): an asynchronous copy from pinned staging on the context stream, and an event the
// caller's stream `s` waits for (a trace on a caller stream, an assembly on another).  The MAX_DEALS
// most recently used tables are kept; evicting one first waits for the context's work (traces in
// flight may read it).
rtbvh_status get_deal(rtbvh_ctx* c, uint32_t H, uint32_t nranks, const rtbvh_ctx::DealTab** out, hipStream_t s) {
    *out = nullptr;
    if (c->root_share == 16 || nranks <= 1) return RTBVH_OK;
    for (auto it = c->deals.begin(); it != c->deals.end(); ++it)
        if (it->H == H && it->nranks == nranks && it->share == c->root_share) {
            if (it != c->deals.begin()) {   // most recent first
                rtbvh_ctx::DealTab t = std::move(*it);
                c->deals.erase(it);
                c->deals.push_front(std::move(t));
            }
            *out = &c->deals.front();
            if (s != c->stream && !c->capturing) HIPC(c, hipStreamWaitEvent(s, c->deals.front().ready, 0));
            return RTBVH_OK;
        }
    if (c->capturing) return fail(c, RTBVH_ERR_INVALID_ARG, "a new band deal inside a graph capture");
    if (c->deals.size() >= rtbvh_ctx::MAX_DEALS) {
        TRY(sync_all(c));
        c->deals.pop_back();
    }
    std::vector<uint32_t> owner;
    deal_owners(H, nranks, c->root_share, owner);
    const uint32_t nb = (uint32_t)owner.size();
    rtbvh_ctx::DealTab t{H, nranks, c->root_share, {}, std::vector<uint32_t>(nranks + 1, 0), {}, {}};
    const size_t words = 2 * (size_t)nb + 1;
    std::vector<uint32_t> cnt(nranks, 0);
    if (t.h.alloc(words) != hipSuccess || t.d.alloc(words) != hipSuccess ||
        hipEventCreateWithFlags(t.ready.out(), hipEventDisableTiming) != hipSuccess)
        return fail(c, RTBVH_ERR_OOM, "band deal table");
    for (uint32_t b = 0; b < nb; b++) t.off[owner[b] + 1]++;
    for (uint32_t r = 0; r < nranks; r++) t.off[r + 1] += t.off[r];
    t.h[2 * nb] = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t r = owner[b], pos = cnt[r]++;
        t.h[t.off[r] + pos] = b;           // rank r's pos-th band
        t.h[nb + b] = r << 24 | pos;       // where band b sits (k_assemble)
    }
    c->deals.push_front(std::move(t));
    rtbvh_ctx::DealTab& f = c->deals.front();
    HIPC(c, hipMemcpyAsync(f.d, f.h, words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipEventRecord(f.ready, c->stream));
    if (s != c->stream) HIPC(c, hipStreamWaitEvent(s, f.ready, 0));
    *out = &f;
    return RTBVH_OK;
}

TraceArgs trace_args(rtbvh_ctx* c, uint32_t W, uint32_t H, uint32_t rank, uint32_t nranks, float4* color, float* inten) {
    TraceArgs a{};
    a.inner = c->d_rec;
    a.topo = c->d_topo;
    a.nbox = c->d_nbox;
    a.nb = false;
    a.leaf = c->d_leaf;
    a.qnode = c->d_qnode;
    a.rootbox = c->d_rootbox;
    a.lfp = c->d_lfp;
    a.tclip = c->d_tclip;
    a.verts = c->d_verts;
    a.idx = c->d_idx;
    a.matidx = c->d_matidx;
    a.texels = c->d_texels;
    a.texinfo = c->d_texinfo;
    a.srgb = c->d_srgb;
    a.ntex = c->ntex;
    a.mats = c->d_mats;
    a.T = c->T;
    a.W = W;
    a.H = H;
    a.rank = rank;
    a.nranks = nranks;
    a.band0 = 0;
    a.bstep = 1;
    const uint32_t nb = (H + 7) / 8;
    a.my_bands = rank < nb ? (nb - rank + nranks - 1) / nranks : 0;   // round-robin; enqueue_walks sets a deal's
    a.band_list = nullptr;
    a.cam = c->d_cam;
    a.color = color;
    a.intensity = inten;
    a.counters = c->d_counters;
    a.overflow = c->d_ovf;
    const uint32_t lim = c->cfg.stack_limit;
    a.stack_limit = lim && lim < (uint32_t)STACK_SIZE ? (int)lim : STACK_SIZE;
    a.stack_limit4 = lim && lim < (uint32_t)STACK4 ? (int)lim : STACK4;
    a.stack_limit4b = lim && lim < (uint32_t)STACK4B ? (int)lim : STACK4B;
    a.limited = lim != 0 && lim < (uint32_t)STACK4B;
    a.acyclic = c->tree.clz64;
    return a;
}

// The walks of a trace (include/rtbvh.h RTBVH_FLAG_*).  RTBVH_FLAG_AUTO_WALK: the
// reference-order kernels (the exact findCollision DFS) up to AUTO_WALK_MAX_TRIS triangles,
// where they are the fastest (C2/C3: Image_Test.obj, Test.obj); above, the 4-wide
// nearest-first walks (C5: 3.4x the reference order) for a frame key once a frame of that key
// traced both ways compared equal on the device (enqueue_trace), the reference order otherwise.
constexpr uint32_t AUTO_WALK_MAX_TRIS = 1u << 16;
constexpr uint32_t WALK_FLAGS = RTBVH_FLAG_NEAREST_FIRST | RTBVH_FLAG_PACKET_PRIMARY | RTBVH_FLAG_REFILL_BOUNCE |
                                RTBVH_FLAG_WIDE_BVH | RTBVH_FLAG_BINNED_PRIMARY;
bool auto_checked(const rtbvh_ctx* c) {
    return (c->cfg.flags & RTBVH_FLAG_AUTO_WALK) && c->T > AUTO_WALK_MAX_TRIS;
}
// A certified-only context -- RTBVH_FLAG_CERTIFIED, or AUTO_WALK on a scene past AUTO_WALK_MAX_TRIS, on a clz64
// tree with no stack limit (plan_trace) -- traces with walks that read no node record: the binned primary pass
// (leaf footprints and records), the certified 4-wide bounce walk (QNodes; a node without a grid flags the ray),
// and reference-order re-traces of the few flagged rays on the topology and node boxes (trace.hip traverse_nb).
// Its multi-kernel build writes the 24-B node boxes instead of the 64-B node records (C4
// refit stage 0.94 -> 0.81 ms without them); records are derived if another walk needs them (ensure_form).
// RTBVH_KEEP_RECORDS=1 (A/B): write the records anyway.
bool records_skipped(const rtbvh_ctx* c) {
    const uint32_t f = c->cfg.flags;
    const bool limited = c->cfg.stack_limit != 0 && c->cfg.stack_limit < (uint32_t)STACK_SIZE;
    const bool small = c->T <= small_build_max() && !(f & RTBVH_FLAG_MULTI_KERNEL_BUILD);   // (k_build_small: records)
    return !small && !c->knob_keep_records && ((f & RTBVH_FLAG_CERTIFIED) || auto_checked(c)) &&
           c->cfg.delta_mode == RTBVH_DELTA_CLZ64 && !limited;
}
// A form of the built tree that the build did not write, derived on first use from the complete tree: on the
// context stream (no walk of a slot stream reads what the kernels write), with stream s ordered behind it.
// The node records come from the topology and node boxes, the boxes from the records (a build writes one of the
// two); the leaf pseudo-records and the QNodes only when the context's walks at the build read none.
rtbvh_status ensure_form(rtbvh_ctx* c, Form form, hipStream_t s) {
    if ((c->tree.valid & form) || !c->tree.built) return RTBVH_OK;
    BuildArgs a = build_args(c);
    if (form == RECORDS || form == NBOX) a.nbox = c->d_nbox;   // (the kernel reads, or writes, the node boxes)
    if (form == RECORDS) launch_records(a, c->stream);
    if (form == NBOX) {
        a.rec_on = 1;
        launch_nbox(a, c->stream);
    }
    if (form == PSEUDO) launch_pseudo(a, c->stream);
    if (form == QNODES) launch_qnodes(a, c->stream);
    HIPC(c, hipGetLastError());
    c->tree.valid |= form;
    return order_after_context(c, s);
}
struct Walks {
    PrimaryKind primary;
    bool refill;        // bounce passes as persistent refill traversal + shading kernel
    BounceWalk bounce;  // refill walk
    bool nearest;       // one-ray-per-lane bounce kernel: nearest-first
    bool sort;          // coherence sort of the bounce queue
};
Walks choose_walks(uint32_t f) {
    Walks w{};
    const bool nearest = (f & RTBVH_FLAG_NEAREST_FIRST) != 0, wide = (f & RTBVH_FLAG_WIDE_BVH) != 0;
    const bool packet = (f & RTBVH_FLAG_PACKET_PRIMARY) != 0;
    w.primary = packet ? (wide ? PrimaryKind::PACKET_WIDE : nearest ? PrimaryKind::PACKET_NEAREST
                                                                    : PrimaryKind::PACKET_REFERENCE)
                       : (nearest ? PrimaryKind::LANE_NEAREST : PrimaryKind::LANE_REFERENCE);
    if (f & RTBVH_FLAG_BINNED_PRIMARY) w.primary = PrimaryKind::BINNED;
    // the ray records are written by k_primary and k_bounce_shade: the split bounce path
    w.refill = (f & (RTBVH_FLAG_REFILL_BOUNCE | RTBVH_FLAG_WIDE_BVH | RTBVH_FLAG_REFRACT_RECORDS)) != 0;
    w.bounce = wide ? BounceWalk::WIDE_QUANTIZED : nearest ? BounceWalk::NEAREST : BounceWalk::REFERENCE;
    w.nearest = nearest;
    w.sort = (f & RTBVH_FLAG_SORT_BOUNCE) != 0;
    return w;
}

// RCCL, resolved at run time: the process's librccl.so.1 if one is already loaded (e.g.
// PyTorch's; dlopen by SONAME returns it), else the system's.  No link-time dependency.
struct Rccl {
    bool ok = false;
    std::string err;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
const Rccl& rccl() {
    static const Rccl lib = [] {
        Rccl r;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) {
            const char* e = dlerror();
            r.err = std::string("RCCL not available: ") + (e ? e : "dlopen(librccl.so.1) failed");
            return r;
        }
        bool all = true;
        auto sym = [&](auto& f, const char* name) {
            f = reinterpret_cast<std::remove_reference_t<decltype(f)>>(dlsym(h, name));
            if (!f) all = false;
        };
        sym(r.GetUniqueId, "ncclGetUniqueId");
        sym(r.CommInitRank, "ncclCommInitRank");
        sym(r.CommDestroy, "ncclCommDestroy");
        sym(r.Send, "ncclSend");
        sym(r.Recv, "ncclRecv");
        sym(r.GroupStart, "ncclGroupStart");
        sym(r.GroupEnd, "ncclGroupEnd");
        sym(r.GetErrorString, "ncclGetErrorString");
        r.ok = all;
        if (!all) r.err = "RCCL: librccl.so.1 lacks a required symbol";
        return r;
    }();
    return lib;
}

// The camera the kernels read (BuildArgs::cam), uploaded in stream order on the context stream when
// rtbvh_set_camera changed it -- after the frames in flight, which read the old one -- and ordered
// before stream s.  A captured frame (RTBVH_FLAG_GRAPH) reads the buffer, so it survives a camera change
// (Graphics::onUpdate writes the camera every frame and the arrow keys orbit it, Graphics.cpp:40-56,
// 937-960).  The matrices travel as a kernel argument (launch_set_camera): captured at the call, one
// dispatch, no pageable host copy (staged through the driver at the call).  Never inside a capture:
// compute_graph's plain frame before it has cleared cam_dirty, and the captured frame must not bake a
// camera in.
rtbvh_status sync_camera(rtbvh_ctx* c, hipStream_t s) {
    if (!c->cam_dirty) return RTBVH_OK;
    TRY(wait_slots(c, c->stream));
    launch_set_camera(c->wvp, c->wv, c->d_cam, c->stream);
    HIPC(c, hipGetLastError());
    c->cam_dirty = false;
    return order_after_context(c, s);
}

// Stream s is about to rewrite the tree (a build, a refit, the replayed build of a captured frame): it waits for
// the tree's readers -- the frames in flight, the outstanding ray queries -- for the last vertex update, whose
// vertices and mesh box it reads, and for this frame's camera; from here on no bin set is of the tree (new
// leaf footprints and depth range).
rtbvh_status before_tree_write(rtbvh_ctx* c, hipStream_t s) {
    TRY(wait_slots(c, s));
    TRY(wait_queries(c, s));
    TRY(wait_update(c, s));
    TRY(sync_camera(c, s));
    c->bins_epoch++;
    return RTBVH_OK;
}

// The build's crossing nodes, if left to a trace (rtbvh_ctx::tail_pending): run in the trace's bin launches
// (WalkPlan::fuse_tail), or before any walk reads the tree and on every early return by the guard
struct TailGuard {
    rtbvh_ctx* c;
    bool pending;
    void run() {
        if (pending) launch_refit_tail(build_args(c), c->stream);
        pending = false;
    }
    ~TailGuard() { run(); }
};

// What a trace launches and where: decided before anything is enqueued (plan_walks), read by prepare_walks
// and launch_walks
struct WalkPlan {
    hipStream_t s;          // as asked: the trace's stream and buffer set,
    uint32_t slot, bounces;
    bool cert;
    bool leaf_pending;      //   the first trace behind a build that recorded ev_leaf
    bool count, timing, records;
    Walks wk;
    PrimaryKind pkind;
    Form nodes;             // the node data its walks read
    uint32_t P, rows;       // max live rays of this shard; its rows
    uint32_t nsplit, Pg;    // chains; max live rays per chain
    uint32_t tblocks;       // the bounce walk's persistent grid
    uint32_t ntx, nty;      // the binned pass's tiles
    bool inflight, fuse_tail, overlap, small_tiles, early_shade;
    uint32_t bset;          // prepare_walks: the buffer set whose bin set the binned pass reads ...
    bool fill_bins;         //   ... and fills first (its own)
    bool walk_tree;         // prepare_walks: the certified bounce passes walk the walk-only tree
};

// The walk-only tree for this trace's certified 4-wide bounce passes: 0 none (the built tree's QNodes), 1 the one the
// context holds for the current build, 2 made first.  Counts the trace (WalkTreeBufs::passes).
int plan_walk_tree(rtbvh_ctx* c, const WalkPlan& p) {
    if (c->capturing || c->knob_walk_tree == 0 || c->T < 2) return 0;
    if (!(p.cert && p.bounces > 0 && p.wk.refill && p.wk.bounce == BounceWalk::WIDE_QUANTIZED)) return 0;
    WalkTreeBufs& w = c->wt;
    if (w.seen_epoch != c->bins_epoch) {
        w.seen_epoch = c->bins_epoch;
        w.passes = 0;
    }
    w.passes++;
    if (w.valid && w.epoch == c->bins_epoch && w.T == c->T) return 1;
    return c->knob_walk_tree == 1 || w.passes >= 3 ? 2 : 0;
}
// ... made: on the context stream, behind the complete built tree (its crossing nodes and node boxes included)
rtbvh_status make_walk_tree(rtbvh_ctx* c) {
    WalkTreeBufs& w = c->wt;
    const size_t T = c->T, ni = T - 1;
    w.valid = false;
    HIPC(c, w.topo.reserve(ni));
    HIPC(c, w.pint.reserve(ni));
    HIPC(c, w.nbox.reserve(6 * ni));
    HIPC(c, w.edge.reserve(ni));
    HIPC(c, w.qnode.reserve(2 * T - 1));
    HIPC(c, w.roots.reserve(2 + T / 2));
    if (!w.ready) HIPC(c, hipEventCreateWithFlags(w.ready.out(), hipEventDisableTiming));
    BuildArgs a = build_args(c);
    a.nbox = c->d_nbox;
    launch_walk_tree(a, WalkTree{w.topo, w.pint, w.nbox, w.edge, w.qnode, w.roots}, c->stream);
    HIPC(c, hipGetLastError());
    HIPC(c, hipEventRecord(w.ready, c->stream));
    w.valid = true;
    w.epoch = c->bins_epoch;
    w.T = c->T;
    c->walk_tree_builds++;
    return RTBVH_OK;
}

WalkPlan plan_walks(const rtbvh_ctx* c, const TraceArgs& a, uint32_t bounces, hipStream_t s, uint32_t slot,
                    uint32_t flags, bool cert, bool timed, bool tail_pending, bool leaf_pending) {
    WalkPlan p{s, slot, bounces, cert, leaf_pending};
    p.bset = slot;
    p.count = (c->cfg.flags & RTBVH_FLAG_COUNT_VISITS) != 0;
    p.timing = timed && (c->cfg.flags & RTBVH_FLAG_TIMING) != 0 && s == c->stream && !c->capturing;
    p.wk = choose_walks(flags);
    p.records = (flags & RTBVH_FLAG_REFRACT_RECORDS) != 0;
    p.P = a.W * deal_rows(a.H, a.rank, a.nranks, c->root_share);
    p.rows = p.P / a.W;
    // persistent grid of the bounce walk: 2048 blocks (8 waves/SIMD), 1024 for a shard of
    // < 4M pixels -- with frames in flight the next frame's primary blocks then share the CUs
    // (C5, rank of N=8, three frames in flight: 0.85 -> 0.78 ms per frame) -- and 512 below 3M pixels once
    // frames are in flight on caller streams (round 5, four in flight, `r05_hh`: the N = 8 rank 0.62 -> 0.60
    // ms per frame, N = 4 1.03 -> 1.00; one frame at a time 512 is slower, 1.13 -> 1.37 ms at N = 8); one frame at
    // a time, 1536 (round 6, with early shading, `r06_bb`: the N = 8 rank 1.198 -> 1.169 ms, N = 4 1.602 -> 1.535;
    // 768 / 2048 / 3072: 1.29 / 1.23 / 1.36 at N = 8)
#ifndef RTBVH_BOUNCE_GRID
#define RTBVH_BOUNCE_GRID (256 * BOUNCE_WAVES)
#endif
    // ("in flight": this trace is on a caller stream's slot, or another slot's frame is still running --
    // not a flag that stays set once any caller stream has traced: ADVICE r5)
    p.inflight = slot != 0;
    for (uint32_t k = 1; k < rtbvh_ctx::MAXSPLIT && !p.inflight && !c->capturing; k++)
        p.inflight = c->sets[k].busy && hipEventQuery(c->sets[k].done) == hipErrorNotReady;
    p.tblocks = p.P < (1u << 22) ? (!p.inflight ? 1536 : p.P < (3u << 20) ? 512 : 1024) : RTBVH_BOUNCE_GRID;
    if (c->knob_bounce_blocks) p.tblocks = c->knob_bounce_blocks;   // tuning override (A/B runs)
    // chains: the rank's bands dealt round-robin over nsplit primary -> bounce chains (band k of this rank goes
    // to chain k % nsplit), each with its own buffer set, chain 0 on the trace's stream, chain g on set g's;
    // joined before the end event.  One chain where the buffers are not per set (the coherence sort's), where
    // the sets are the caller streams', and for the binned primary pass, which covers the rank's whole frame.
    // The build's leaf footprints are exact for frames of up to 32768 pixels a side (rtbvh_device.h
    // leaf_footprint); a certified trace past that size: the reference-order lane walk, exact by construction
    const bool binned = p.wk.primary == PrimaryKind::BINNED;
    p.pkind = binned && (a.W > 32768u || a.H > 32768u)
                  ? (cert ? PrimaryKind::LANE_REFERENCE : PrimaryKind::PACKET_WIDE)
                  : p.wk.primary;
    p.nsplit = trace_split(c);
    if (p.wk.sort || a.my_bands < p.nsplit || slot || c->slots_used || binned) p.nsplit = 1;
    p.Pg = p.nsplit == 1 ? p.P : a.W * 8 * ((a.my_bands + p.nsplit - 1) / p.nsplit);
    // the walks' node data: a certified trace's re-traces walk the node boxes (TraceArgs::nb), every other walk
    // the node records; a build writes one of the two, the other is derived from the complete tree (after the
    // tail: prepare_walks), so only a trace that finds its form runs the build's crossing nodes in its bin launches
    p.nodes = cert ? NBOX : RECORDS;
    p.fuse_tail = tail_pending && p.pkind == PrimaryKind::BINNED && s == c->stream && slot == 0 && p.rows > 0 &&
                  (c->tree.valid & p.nodes);
    // rtbvh_compute_bvh: the binned pass (and the zeroing before it) on the side stream, concurrent
    // with the build's crossing nodes (launch_refit_tail)
    p.overlap = p.pkind == PrimaryKind::BINNED && leaf_pending && s == c->stream && slot == 0 && p.nsplit == 1;
    p.ntx = pb_tiles_x(a.W);
    p.nty = pb_tiles_y(p.rows);
    // a rank's small pass one frame at a time: 512 threads a tile (its ~1,000 tiles all run at once;
    // with frames in flight 256 is faster, round 5 r05_jj). Round 6 (r06_stl): the N = 8 rank's frame
    // 1.13-1.15 -> 1.11 ms; N = 4 (2.1M pixels) the same, N = 2 (4.1M) +0.05 ms: below 1.5M pixels only
    p.small_tiles = !p.inflight && !c->knob_no_small_tiles && (size_t)a.W * p.rows < (3u << 19);
    // a frame one at a time shades its rays in the walk's tail (trace.hip RTBVH_EARLY_SHADE: one C5 frame
    // 3.44-3.46 -> 3.37-3.40 ms); with frames in flight other frames' kernels fill that tail, and the
    // shading workgroups cost the in-flight rate 1-3% (r06_x): not then
    p.early_shade = cert && !p.inflight && !c->knob_no_early_shade;
    return p;
}

// What the launches need before the first of them: capacities, the tree forms the walks read (behind the
// build's crossing nodes), and the binned pass's bin set -- found, or the trace's own to be filled, ordered
// behind the other sets' traces that still read it
rtbvh_status prepare_walks(rtbvh_ctx* c, WalkPlan& p, TraceArgs& a, const rtbvh_ctx::DealTab* deal, TailGuard& tail) {
    hipStream_t s = p.s;
    TraceSet& mine = c->sets[p.slot];
    const size_t P = p.P;
    if (p.records) {
        if (!(c->d_refl_rec.has(14 * P) && c->d_refr_rec.has(14 * P))) {
            drop_graph(c);
            HIPC(c, c->d_refl_rec.reserve(14 * P));
            HIPC(c, c->d_refr_rec.reserve(14 * P));
        }
        a.refl_rec = c->d_refl_rec;
        a.refr_rec = c->d_refr_rec;
    }
    const int wt = plan_walk_tree(c, p);
    if (wt == 2) p.fuse_tail = false;   // (it reads the crossing nodes: they run first, not in this trace's bin launches)
    if (!p.fuse_tail && tail.pending) {   // before any walk reads the tree
        tail.run();
        TRY(order_after_context(c, s));   // (a caller stream: ordered after it like after the build)
    }
    TRY(ensure_form(c, p.nodes, s));
    a.nb = p.cert;
    TRY(ensure_split_capacity(c, p.slot ? p.slot + 1 : p.nsplit, p.Pg));
    // a 4-wide bounce walk over a one-workgroup build that quantized no nodes (the context's walks took none)
    if (p.bounces > 0 && p.wk.refill && p.wk.bounce == BounceWalk::WIDE_QUANTIZED) TRY(ensure_form(c, QNODES, s));
    // the walk-only tree of the certified bounce passes: made here (the node boxes are there: p.nodes), or the
    // context's; a trace on another stream waits for its QNode pass
    if (wt) {
        if (wt == 2) TRY(make_walk_tree(c));
        if (s != c->stream) HIPC(c, hipStreamWaitEvent(s, c->wt.ready, 0));
        a.qnode_walk = c->wt.qnode;
        p.walk_tree = true;
    }
    // a packet walk over a tree built without the leaf pseudo-records (the context's walks took none;
    // set_flags since, or a frame past the binned pass's 32768 pixels a side)
    if (p.pkind == PrimaryKind::PACKET_REFERENCE || p.pkind == PrimaryKind::PACKET_NEAREST ||
        p.pkind == PrimaryKind::PACKET_WIDE)
        TRY(ensure_form(c, PSEUDO, s));
    // a certified trace's lists (one chain: the trace's own set)
    if (p.cert && p.bounces > 0 && !mine.defer.has(P)) {   // (zeroed once: its readers clear what they take)
        drop_graph(c);
        HIPC(c, mine.defer.reserve(P));
        if (hipMemsetAsync(mine.defer, 0, sizeof(uint32_t) * P, c->stream) != hipSuccess) {
            mine.defer.reset();   // (not clean: not kept)
            return fail(c, RTBVH_ERR_HIP, "clearing the deferred-ray list failed");
        }
        TRY(order_after_context(c, s));
    }
    if (p.cert && !mine.redo.has(P)) {
        drop_graph(c);
        HIPC(c, mine.redo.reserve(P));
    }
    if (p.pkind != PrimaryKind::BINNED || p.rows == 0) return RTBVH_OK;
    // the binned pass's bin set (one chain): a set already filled for this tree and frame shape, or the trace's
    // own, filled by this trace (fill_bins)
    const size_t px = (size_t)a.W * p.rows;
    if (pb_keys_used() && !mine.pbkeys.has(px)) {   // (the trace's own, whichever the bin set)
        drop_graph(c);
        HIPC(c, mine.pbkeys.reserve(px));
    }
    const PbKey key{c->bins_epoch, a.W, a.H, p.rows, a.rank, a.nranks, c->T, p.ntx, p.nty,
                    a.nranks > 1 ? c->root_share : 16u, deal ? deal->d.h : nullptr};
    // (a trace that runs the build's crossing nodes in its count pass, or its pass beside them, is the first
    // of its tree: it finds none)
    const int found = p.fuse_tail || p.leaf_pending ? -1 : find_bins(c, key);
    if (found >= 0) {
        p.bset = (uint32_t)found;
        PbBufs& pb = c->sets[p.bset].pb;
        if (p.bset != p.slot) HIPC(c, hipStreamWaitEvent(s, pb.filled, 0));   // (its own set's: stream order)
        pb.readers |= 1u << p.slot;
        return RTBVH_OK;
    }
    p.fill_bins = true;
    PbBufs& pb = mine.pb;
    TRY(ensure_pb_capacity(c, pb, c->T, p.ntx * p.nty));
    if (a.nranks > 1 && !pb.list.has(pb_list_words(c->T))) {
        drop_graph(c);
        HIPC(c, pb.list.reserve(pb_list_words(c->T)));
    }
    // the traces of other buffer sets that read what the bin set held (the same tree at another frame shape,
    // rank or deal -- a new tree's build has waited for them all) end before this one overwrites it:
    // stream-side, on their sets' events, or the context stream's work so far for set 0's.  Not inside a
    // capture (no frame in flight outlives the wait_slots before every replay)
    for (uint32_t k = 0; k < rtbvh_ctx::MAXSPLIT && !c->capturing; k++) {
        if (k == p.slot || !(pb.readers & 1u << k)) continue;
        if (k == 0) TRY(order_after_context(c, s));
        else if (c->sets[k].done) HIPC(c, hipStreamWaitEvent(s, c->sets[k].done, 0));
    }
    pb.readers = 1u << p.slot;
    pb.valid = false;   // (until the fill is enqueued: launch_walks)
    pb.key = key;
    return RTBVH_OK;
}

// The launches: one zeroing of the trace's counters, queue counts, bounce work counters and bin counts, then
// per chain the primary pass and the bounce passes
rtbvh_status launch_walks(rtbvh_ctx* c, const WalkPlan& p, const TraceArgs& a, TailGuard& tail) {
    hipStream_t s = p.s;
    TraceSet& mine = c->sets[p.slot];   // the trace's set: chain 0's, and all that a one-chain trace uses
    const uint32_t bounces = p.bounces, nsplit = p.nsplit;
    const bool count = p.count, cert = p.cert, refill = p.wk.refill;
    Event* ev = c->evt[c->n_traces % rtbvh_ctx::RING];
    ZeroList z{};   // (a trace's chains use consecutive sets: their parts of the shared blocks are consecutive)
    z.ptr[0] = reinterpret_cast<uint32_t*>(mine.counters);
    z.words[0] = 64 * 2;
    z.ptr[1] = mine.qcount;
    z.words[1] = 32 * nsplit;
    if (refill && bounces) {
        z.ptr[2] = mine.next;
        z.words[2] = (size_t)NEXT_WORDS * nsplit;
    }
    if (p.fill_bins) {
        z.ptr[3] = mine.pb.off;
        z.words[3] = (size_t)p.ntx * p.nty * PB_NZ + 1;
        if (a.nranks > 1) {   // the list counters
            z.ptr[4] = mine.pb.list;
            z.words[4] = (size_t)PB_LISTS * PB_LIST_STRIDE;
        }
    }
    hipStream_t sp = s;   // the binned pass's stream
    if (p.overlap) {
        sp = c->side;
        HIPC(c, hipStreamWaitEvent(sp, c->ev_leaf, 0));
    }
    launch_zero(z, sp);
    if (p.timing) HIPC(c, hipEventRecord(ev[0], sp));
    if (nsplit > 1) HIPC(c, hipEventRecord(c->ev_fork, s));
    for (uint32_t g = 0; g < nsplit; g++) {
        TraceSet& set = c->sets[p.slot + g];   // chain g's set
        hipStream_t sg = g ? set.chain : s;
        if (g) HIPC(c, hipStreamWaitEvent(sg, c->ev_fork, 0));
        TraceArgs ag = a;
        ag.band0 = g;
        ag.bstep = nsplit;
        ag.pb_list = p.fill_bins && a.nranks > 1 ? mine.pb.list : nullptr;   // (the bin passes': one chain)
        RayQ* q[2] = {set.q[0], set.q[1]};
        uint32_t* qc = set.qcount;
        const bool tg = p.timing && g == 0;   // stage events: chain 0's kernels
        if (p.pkind == PrimaryKind::BINNED) {   // (one chain: `mine`)
            PbBufs& pbb = c->sets[p.bset].pb;
            const PrimBins pb{pbb.off, pbb.cur, pbb.bins, mine.pbkeys, pbb.sums, pbb.cap_bins, p.ntx, p.nty};
            if (p.rows) {
                const BuildArgs ba = build_args(c);
                const Redo rd{mine.redo, &qc[16]};
                if (p.fill_bins) {
                    launch_pb_bins(ag, pb, p.rows, true, sp, p.fuse_tail ? &ba : nullptr);
                    c->bin_builds++;
                    // the set is this key's from here on, for every later trace (they wait for `filled`); a
                    // captured fill is the graph's own, rewritten by every replay
                    if (c->knob_bins_reuse && !c->capturing) {
                        if (!pbb.filled) HIPC(c, hipEventCreateWithFlags(pbb.filled.out(), hipEventDisableTiming));
                        HIPC(c, hipEventRecord(pbb.filled, sp));
                        pbb.valid = true;
                    }
                }
                launch_pb_raster(ag, pb, p.rows, q[0], &qc[0], count, bounces > 0, sp, cert ? &rd : nullptr,
                                 p.small_tiles);
                if (p.fuse_tail) tail.pending = false;
            }
            if (p.overlap) {   // (with nothing traced, the zeroing still joins)
                HIPC(c, hipEventRecord(c->ev_prim, sp));
                HIPC(c, hipStreamWaitEvent(sg, c->ev_prim, 0));
            }
            if (p.rows) launch_pb_gate(ag, pb, q[0], &qc[0], count, bounces > 0, sg, cert);
        } else
            launch_primary(ag, q[0], &qc[0], count, bounces > 0, p.pkind, sg);
        if (tg) HIPC(c, hipEventRecord(ev[1], sg));
        for (uint32_t b = 0; b < bounces; b++) {
            const uint32_t* perm = nullptr;
            if (p.wk.sort) {
                launch_bounce_keys(q[b & 1], &qc[b], c->d_rootbox, p.P, c->d_bkin, c->d_bvin, sg);
                perm = radix_sort_pairs(c->d_bkin, c->d_bvin, c->d_bka, c->d_bva, c->d_bkb, c->d_bvb, p.P, 30,
                                        c->d_bscratch, sg).vals;
            }
            if (refill) {
                if (tg && b == 0) HIPC(c, hipEventRecord(ev[3], sg));
                uint32_t* nxb = set.next + (size_t)NEXT_SEGS * NEXT_STRIDE * b;
                const BounceShade es{q[(b + 1) & 1], &qc[b + 1], b + 1 < bounces, mine.redo, &qc[17 + b], p.Pg};
                launch_bounce_traverse(ag, q[b & 1], &qc[b], perm, count, p.wk.bounce, set.hit, nxb, p.tblocks, sg, cert,
                                       mine.defer, p.early_shade ? &es : nullptr);
                if (tg && b == 0) HIPC(c, hipEventRecord(ev[4], sg));
                const Redo rd{mine.redo, &qc[17 + b], mine.defer, nxb};
                launch_bounce_shade(ag, q[b & 1], &qc[b], set.hit, q[(b + 1) & 1], &qc[b + 1], count, b + 1 < bounces,
                                    p.Pg, sg, cert ? &rd : nullptr);
            } else
                launch_bounce(ag, q[b & 1], &qc[b], perm, q[(b + 1) & 1], &qc[b + 1], count, b + 1 < bounces,
                              p.wk.nearest, sg);
        }
        if (g) {
            HIPC(c, hipEventRecord(set.join, sg));
            HIPC(c, hipStreamWaitEvent(s, set.join, 0));
        }
    }
    // a snapshot of the overflow word for this trace's set (rtbvh_synchronize reports a change)
    HIPC(c, hipMemcpyAsync(mine.ovf, c->d_ovf, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (p.timing) {
        HIPC(c, hipEventRecord(ev[2], s));
        c->evt_trav[c->n_traces % rtbvh_ctx::RING] = refill && bounces > 0;
        c->n_traces++;
    }
    return RTBVH_OK;
}

// The kernels of one trace with the walks of `flags` (timed: record the stage events when
// RTBVH_FLAG_TIMING asks for them); walk_state: what rtbvh_stats.walk_state reports of it.
// cert: the certified walks (flags = the fast walks: binned primary pass, 4-wide bounce walk):
// every pass checks each ray's certificate and re-traces the rays that fail it in the reference order.
rtbvh_status enqueue_walks(rtbvh_ctx* c, uint32_t W, uint32_t H, uint32_t bounces, uint32_t rank, uint32_t nranks,
                           float4* color, float* inten, hipStream_t s, uint32_t slot, uint32_t flags, bool timed,
                           uint32_t walk_state, bool cert = false) {
    const bool leaf_pending = c->leaf_pending;   // (this trace is the first after the build or none is)
    c->leaf_pending = false;
    TailGuard tail{c, c->tail_pending};
    c->tail_pending = false;
    if (!c->tree.built) return fail(c, RTBVH_ERR_NOT_READY, "trace before build");
    if (c->stale) return fail_stale(c, "trace");
    if (W == 0 || H == 0 || nranks == 0 || rank >= nranks || bounces > 14)
        return fail(c, RTBVH_ERR_INVALID_ARG, "bad trace dimensions");
    TRY(ensure_trace_capacity(c, (size_t)W * H));
    if (!color) color = c->d_color;
    TraceArgs a = trace_args(c, W, H, rank, nranks, color, inten);
    const rtbvh_ctx::DealTab* deal = nullptr;
    TRY(get_deal(c, H, nranks, &deal, s));
    if (deal) {
        a.my_bands = deal->off[rank + 1] - deal->off[rank];
        a.band_list = deal->d + deal->off[rank];
        a.band_slots = deal->d + (H + 7) / 8;
    }
    a.counters = c->sets[slot].counters;
    if ((flags & RTBVH_FLAG_REFRACT_RECORDS) && slot)
        return fail(c, RTBVH_ERR_INVALID_ARG, "ray records are traced on the context stream only");
    WalkPlan p = plan_walks(c, a, bounces, s, slot, flags, cert, timed, tail.pending, leaf_pending);
    TRY(prepare_walks(c, p, a, deal, tail));
    TRY(launch_walks(c, p, a, tail));
    const bool frame_here = color == c->d_color && nranks == 1;
    c->last = LastTrace{true, W, H, bounces, rank, nranks, p.nsplit, slot, p.records ? p.P : 0, flags & WALK_FLAGS,
                        walk_state, cert, frame_here, frame_here && inten != nullptr, p.walk_tree};
    return check_launch(c, "trace kernels");
}

// ---- RTBVH_FLAG_AUTO_WALK: the certified fast walks ---------------------------------
// The fast walks return the lexicographic (t, leaf) minimum over the leaves they reach, findCollision
// (RayTraceTraversal.hlsl:106-193) the first strict minimum over the leaves IT reaches; they agree
// whenever every hit lies inside the boxes on its root path under the same rounding ("containment").
// Where containment fails they can differ (tests/containment.py).  The certified walks make each ray
// carry its own proof: they prune on boxes grown by the rounding margin of the triangle test
// (margin.h), so they see every triangle that could be accepted below their bound -- the minimum they
// return is the minimum over every triangle the reference could test -- and a ray's answer is the
// reference's when its winning leaf's own box passes the reference slab test at that t (the
// certificate).  Rays without one are re-traced in the reference order.  No per-frame check, no frame
// key: a moving camera costs nothing extra, and a captured frame replays as it is.
// The walks of a trace: (flags, certified)
struct TracePlan {
    uint32_t flags;
    bool cert;
    uint32_t state;   // rtbvh_stats.walk_state
};
TracePlan plan_trace(const rtbvh_ctx* c, uint32_t f) {
    if (!(f & (RTBVH_FLAG_AUTO_WALK | RTBVH_FLAG_CERTIFIED))) return TracePlan{f, false, 0};
    const uint32_t ref = f & ~WALK_FLAGS;
    // the certificate speaks for the reference order on a clz64 tree with the full stack (a run-time
    // stack limit makes the reference order end rays early, which no fast walk reproduces)
    const bool limited = c->cfg.stack_limit != 0 && c->cfg.stack_limit < (uint32_t)STACK_SIZE;
    const bool want = (f & RTBVH_FLAG_CERTIFIED) || auto_checked(c);
    if (!want || !c->tree.clz64 || limited) return TracePlan{ref, false, 0};
    return TracePlan{ref | RTBVH_FLAG_NEAREST_FIRST | RTBVH_FLAG_REFILL_BOUNCE | RTBVH_FLAG_WIDE_BVH |
                         RTBVH_FLAG_BINNED_PRIMARY,
                     true, 2};
}

rtbvh_status enqueue_trace(rtbvh_ctx* c, uint32_t W, uint32_t H, uint32_t bounces, uint32_t rank, uint32_t nranks,
                           float4* color, float* inten, hipStream_t s, uint32_t slot = 0) {
    if (!c->tree.built) return fail(c, RTBVH_ERR_NOT_READY, "trace before build");
    if (c->stale) return fail_stale(c, "trace");
    TRY(sync_camera(c, s));
    TracePlan p = plan_trace(c, c->cfg.flags);
    if (p.cert && !c->capturing) c->cert_traces++;
    // AUTO_WALK on a small scene: the reference order, as one-ray-per-lane walks or as wave packets (the
    // same frame: both are the exact findCollision DFS per ray).  Which is faster depends on the scene
    // (C3, Test.obj: packets 0.089 against lanes 0.108 ms; C2, Image_Test.obj: 0.175 against 0.073), so
    // the first full-frame trace of a scene and frame size on the context stream times both primary
    // passes, twice each, and keeps the packets only when they are 5% faster.  Not while capturing: a
    // captured frame keeps the choice made before it (rtbvh_compute_bvh with RTBVH_FLAG_GRAPH traces a
    // frame uncaptured first).  Not with a stack limit (a wave packet shares one stack: its overflows
    // differ from a lane's) nor the CPUTests delta.
    const uint32_t f = c->cfg.flags;
    const bool limited = c->cfg.stack_limit != 0 && c->cfg.stack_limit < (uint32_t)STACK_SIZE;
    if ((f & RTBVH_FLAG_AUTO_WALK) && !p.cert && c->tree.clz64 && !limited) {
        const uint64_t key = (uint64_t)W << 48 | (uint64_t)H << 32 | c->T;
        // (the first frame of a key is synchronous: it waits for its own timed passes; the key includes the
        // walk flags, so a set_flags that changes the walks times them again)
        const uint32_t fw = f & (WALK_FLAGS | RTBVH_FLAG_AUTO_WALK | RTBVH_FLAG_CERTIFIED | RTBVH_FLAG_SORT_BOUNCE);
        if ((c->small_key != key || c->small_flags != fw) && !c->capturing && s == c->stream && slot == 0 &&
            nranks == 1) {
            Event* ev = c->ev_small;
            for (int k = 0; k < 2; k++)
                if (!ev[k]) HIPC(c, hipEventCreate(ev[k].out()));
            float best[2] = {INFINITY, INFINITY};
            for (int round = 0; round < 2; round++)
                for (int k = 0; k < 2; k++) {
                    HIPC(c, hipEventRecord(ev[0], s));
                    TRY(enqueue_walks(c, W, H, 0, 0, 1, color, inten, s, 0,
                                      p.flags | (k ? RTBVH_FLAG_PACKET_PRIMARY : 0u), false, p.state));
                    HIPC(c, hipEventRecord(ev[1], s));
                    HIPC(c, hipEventSynchronize(ev[1]));
                    float ms = 0.f;
                    HIPC(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
                    best[k] = std::min(best[k], ms);
                }
            c->small_packet = best[1] < 0.95f * best[0];
            c->small_key = key;
            c->small_flags = fw;
        }
        if (c->small_key == key && c->small_flags == fw && c->small_packet) p.flags |= RTBVH_FLAG_PACKET_PRIMARY;
    }
    return enqueue_walks(c, W, H, bounces, rank, nranks, color, inten, s, slot, p.flags, true, p.state, p.cert);
}

}  // namespace

extern "C" {

int rtbvh_abi_version(void) { return RTBVH_ABI_VERSION; }
uint32_t rtbvh_stats_size(void) { return (uint32_t)sizeof(rtbvh_stats); }

void rtbvh_config_default(rtbvh_config* cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->device = 0;
    cfg->morton_mode = RTBVH_MORTON_CPUTESTS;
    cfg->delta_mode = RTBVH_DELTA_CLZ64;
    for (int k = 0; k < 3; k++) {   // Graphics.cpp:528-529
        cfg->scene_bb_min[k] = -700.f;
        cfg->scene_bb_max[k] = 700.f;
    }
}

rtbvh_status rtbvh_create(const rtbvh_config* cfg, rtbvh_ctx** out) {
    if (!out) return fail(nullptr, RTBVH_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    rtbvh_ctx* c = new (std::nothrow) rtbvh_ctx();
    if (!c) return fail(nullptr, RTBVH_ERR_OOM, "host allocation failed");
    if (cfg) c->cfg = *cfg;
    else rtbvh_config_default(&c->cfg);
    if (c->cfg.morton_mode > 1 || c->cfg.delta_mode > 1 || c->cfg.reserved != 0) {
        delete c;
        return fail(nullptr, RTBVH_ERR_INVALID_ARG, "bad morton/delta mode");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        delete c;
        return fail(nullptr, RTBVH_ERR_NO_DEVICE, "no HIP device");
    }
    if (c->cfg.device < 0 || c->cfg.device >= ndev || hipSetDevice(c->cfg.device) != hipSuccess) {
        delete c;
        return fail(nullptr, RTBVH_ERR_NO_DEVICE, "bad device ordinal");
    }
    if (c->cfg.stream) {
        c->stream = (hipStream_t)c->cfg.stream;
    } else {
        if (hipStreamCreateWithFlags(c->own_stream.out(), hipStreamNonBlocking) != hipSuccess) {
            delete c;
            return fail(nullptr, RTBVH_ERR_HIP, "hipStreamCreate failed");
        }
        c->stream = c->own_stream;
    }
    bool ev_ok = true;
    for (auto& row : c->evb)
        for (auto& e : row) ev_ok = ev_ok && hipEventCreate(e.out()) == hipSuccess;
    for (auto& row : c->evt)
        for (auto& e : row) ev_ok = ev_ok && hipEventCreate(e.out()) == hipSuccess;
    if (!ev_ok) {
        rtbvh_destroy(c);
        return fail(nullptr, RTBVH_ERR_HIP, "hipEventCreate failed");
    }
    if (hipEventCreateWithFlags(c->ev_built.out(), hipEventDisableTiming) != hipSuccess) {
        rtbvh_destroy(c);
        return fail(nullptr, RTBVH_ERR_HIP, "hipEventCreate failed");
    }
    if (c->d_ovf.alloc(1) != hipSuccess || hipMemset(c->d_ovf, 0, sizeof(unsigned long long)) != hipSuccess ||
        c->h_ovf.alloc(rtbvh_ctx::MAXSPLIT) != hipSuccess) {
        rtbvh_destroy(c);
        return fail(nullptr, RTBVH_ERR_OOM, "overflow counter allocation failed");
    }
    memset(c->h_ovf, 0, sizeof(unsigned long long) * rtbvh_ctx::MAXSPLIT);
    for (uint32_t b = 0; b < rtbvh_ctx::MAXSPLIT; b++) c->sets[b].ovf = c->h_ovf + b;
    if (c->d_cam.alloc(32) != hipSuccess ||
        hipMemset(c->d_cam, 0, 32 * sizeof(float)) != hipSuccess) {
        rtbvh_destroy(c);
        return fail(nullptr, RTBVH_ERR_OOM, "camera buffer allocation failed");
    }
    // A/B tuning knobs, read once here (not per frame)
    if (const char* e = getenv("RTBVH_BOUNCE_BLOCKS")) c->knob_bounce_blocks = (uint32_t)std::max(0, atoi(e));
    if (const char* e = getenv("RTBVH_OVERLAP")) c->knob_overlap = atoi(e) != 0;
    if (const char* e = getenv("RTBVH_SIDE_PRIORITY")) c->knob_side_priority = atoi(e) != 0;
    if (const char* e = getenv("RTBVH_KEEP_RECORDS")) c->knob_keep_records = atoi(e) != 0;
    if (const char* e = getenv("RTBVH_EARLY_SHADE")) c->knob_no_early_shade = atoi(e) == 0;   // (A/B: 0 = off)
    if (const char* e = getenv("RTBVH_PB_SMALL_TILES")) c->knob_no_small_tiles = atoi(e) == 0;   // (A/B: 0 = off)
    if (const char* e = getenv("RTBVH_BINS_REUSE")) c->knob_bins_reuse = atoi(e) != 0;   // (A/B: 0 = a fill per trace)
    if (const char* e = getenv("RTBVH_WALK_TREE")) c->knob_walk_tree = atoi(e) != 0 ? 1 : 0;   // (tests, A/B)
    *out = c;
    return RTBVH_OK;
}

void rtbvh_destroy(rtbvh_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    (void)sync_all(c);   // the context stream, then the frames in flight and the ray queries on caller streams
    drop_graph(c);
    delete c;
}

const char* rtbvh_last_error(const rtbvh_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

rtbvh_status rtbvh_set_scene(rtbvh_ctx* c, const rtbvh_vertex* verts, uint32_t nverts, const uint32_t* indices,
                             uint32_t nidx, const uint32_t* mat_idx, const rtbvh_material* mats, uint32_t nmats,
                             const rtbvh_texture* textures, uint32_t ntex) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    drop_graph(c);   // a captured frame holds the old buffers
    if (ntex && !textures) return fail(c, RTBVH_ERR_INVALID_ARG, "set_scene: ntex > 0 without textures");
    for (uint32_t k = 0; k < ntex; k++)
        if (textures[k].width == 0 || textures[k].height == 0 || !textures[k].rgba8)
            return fail(c, RTBVH_ERR_INVALID_ARG, "set_scene: empty texture");
    if (!verts || !indices || !mat_idx || !mats || nverts == 0 || nidx == 0 || nidx % 3 != 0 || nmats == 0)
        return fail(c, RTBVH_ERR_INVALID_ARG, "set_scene: empty or ragged input");
    const uint32_t T = nidx / 3;
    if (T >= (1u << 30)) return fail(c, RTBVH_ERR_INVALID_ARG, "set_scene: too many triangles");
    for (uint32_t i = 0; i < nidx; i++)
        if (indices[i] >= nverts) return fail(c, RTBVH_ERR_INVALID_ARG, "set_scene: index out of range");
    for (uint32_t t = 0; t < T; t++)
        if (mat_idx[t] >= nmats) return fail(c, RTBVH_ERR_INVALID_ARG, "set_scene: material index out of range");
    HIPC(c, hipSetDevice(c->cfg.device));
    TRY(sync_all(c));   // frames in flight and ray queries on caller streams read the old scene and BVH
    c->q.busy = false;
    reset_tree(c);
    try {
        std::vector<float4> opos(nverts);
        for (uint32_t i = 0; i < nverts; i++)
            opos[i] = make_float4(verts[i].position[0], verts[i].position[1], verts[i].position[2], 0.f);
        HIPC(c, c->d_opos.alloc(nverts));
        HIPC(c, c->d_verts.alloc((size_t)nverts * 8));
        HIPC(c, c->d_idx.alloc(nidx));
        HIPC(c, c->d_matidx.alloc(T));
        HIPC(c, c->d_mats.alloc(nmats));
        HIPC(c, hipMemcpy(c->d_opos, opos.data(), sizeof(float4) * nverts, hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(c->d_verts, verts, sizeof(rtbvh_vertex) * nverts, hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(c->d_idx, indices, sizeof(uint32_t) * nidx, hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(c->d_matidx, mat_idx, sizeof(uint32_t) * T, hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(c->d_mats, mats, sizeof(rtbvh_material) * nmats, hipMemcpyHostToDevice));
        // textures: one texel array + a {first texel, width, height} table (t4-t5 of
        // RayTraceGlobal.hlsl:114-115, any count here)
        std::vector<uint4> info(ntex ? ntex : 1);
        size_t total = 0;
        for (uint32_t k = 0; k < ntex; k++) {
            info[k] = make_uint4((uint32_t)total, textures[k].width, textures[k].height, 0u);
            total += (size_t)textures[k].width * textures[k].height;
        }
        if (total >= (1ull << 32)) return fail(c, RTBVH_ERR_INVALID_ARG, "set_scene: textures too large");
        HIPC(c, c->d_texels.alloc(total ? total : 1));
        HIPC(c, c->d_texinfo.alloc(info.size()));
        for (uint32_t k = 0; k < ntex; k++)
            HIPC(c, hipMemcpy(c->d_texels + info[k].x, textures[k].rgba8,
                              (size_t)textures[k].width * textures[k].height * 4, hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(c->d_texinfo, info.data(), sizeof(uint4) * info.size(), hipMemcpyHostToDevice));
        if (!c->d_srgb) {
            float tab[256];
            rtbvh_srgb_table(tab);
            HIPC(c, c->d_srgb.alloc(256));
            HIPC(c, hipMemcpy(c->d_srgb, tab, sizeof(tab), hipMemcpyHostToDevice));
        }
        c->ntex = ntex;
    } catch (const std::bad_alloc&) {
        return fail(c, RTBVH_ERR_OOM, "set_scene: host allocation failed");
    }
    static_assert(sizeof(rtbvh_material) == sizeof(Mat), "material layout");
    c->V = nverts;
    c->T = T;
    c->nmat = nmats;
    TRY(ensure_build_capacity(c, T));
    if (c->cfg.morton_mode == RTBVH_MORTON_CPUTESTS) {
        // the object-space mesh box the CPUTests Morton codes are normalised by: a property of
        // the scene, computed once after loading as ShaderSim does (ShaderSim/main.cpp:277-285),
        // not per build (it does not depend on the camera)
        BuildArgs a = build_args(c);
        launch_bounds(a, c->stream);
        TRY(check_launch(c, "mesh bounds"));
        HIPC(c, hipStreamSynchronize(c->stream));
    }
    c->have_scene = true;
    c->small_key = 0;   // (the primary kind of a small scene is timed again)
    return RTBVH_OK;
}

rtbvh_status rtbvh_set_camera(rtbvh_ctx* c, const float wvp[16], const float wv[16]) {
    if (!c || !wvp || !wv) return RTBVH_ERR_INVALID_ARG;
    // Graphics::onUpdate writes the matrices every frame (Graphics.cpp:44-53); the kernels read them
    // from a device buffer (sync_camera), so a captured frame (RTBVH_FLAG_GRAPH) replays with the new
    // camera as it is
    if (c->have_camera && memcmp(c->wvp, wvp, sizeof(c->wvp)) == 0 && memcmp(c->wv, wv, sizeof(c->wv)) == 0)
        return RTBVH_OK;
    memcpy(c->wvp, wvp, sizeof(c->wvp));
    memcpy(c->wv, wv, sizeof(c->wv));
    c->have_camera = true;
    c->cam_dirty = true;
    return RTBVH_OK;
}

// What a build leaves to the trace behind it (rtbvh_compute_bvh's frame): LEAF_EVENT: it records ev_leaf once the
// leaves are written (rtbvh_ctx::leaf_pending); TAIL_TO_TRACE: it leaves its crossing nodes to the trace's bin
// launches (tail_pending; flush_tail if no trace takes them)
enum Handoff : uint32_t { LEAF_EVENT = 1, TAIL_TO_TRACE = 2 };
static rtbvh_status build_tree(rtbvh_ctx* c, uint32_t handoff) {
    if (!c->have_scene || !c->have_camera) return fail(c, RTBVH_ERR_NOT_READY, "build before set_scene/set_camera");
    HIPC(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    const bool timing = (c->cfg.flags & RTBVH_FLAG_TIMING) != 0 && !c->capturing;
    BuildArgs a = build_args(c);
    TRY(before_tree_write(c, s));
    const bool clz64 = c->cfg.delta_mode == RTBVH_DELTA_CLZ64;
    Event* ev = c->evb[c->n_builds % rtbvh_ctx::RING];
    if (timing) HIPC(c, hipEventRecord(ev[0], s));
    if (c->T <= small_build_max() && !(c->cfg.flags & RTBVH_FLAG_MULTI_KERNEL_BUILD)) {
        // one workgroup (build.hip k_build_small); its time is reported as stage 0
        c->sorted = SortResult{c->d_ka, c->d_va};
        a.sorted_keys = c->d_ka;
        a.sorted_vals = c->d_va;
        a.pseudo = 1;   // (the one-workgroup build writes them anyway)
        a.rec_on = 1;   // (and the node records)
        a.nbox = nullptr;
        launch_build_small(a, s);
        // the QNodes only for walks that read them (the 4-wide bounce walk; enqueue_walks otherwise)
        const bool qnodes = (c->cfg.flags & (RTBVH_FLAG_WIDE_BVH | RTBVH_FLAG_CERTIFIED)) != 0 || auto_checked(c);
        if (qnodes) launch_qnodes(a, s);
        c->leaf_pending = false;
        c->tail_pending = false;
        if (timing) for (int k = 1; k <= 5; k++) HIPC(c, hipEventRecord(ev[k], s));
        if (timing) c->n_builds++;
        if (!c->capturing) HIPC(c, hipEventRecord(c->ev_built, s));
        c->tree = Tree{true, clz64, RECORDS, RECORDS | PSEUDO | (qnodes ? QNODES : 0u)};
        c->stale = false;
        return check_launch(c, "build kernel");
    }
    if (timing) HIPC(c, hipEventRecord(ev[1], s));   // (the mesh box is the scene's: rtbvh_set_scene)
    // a certified-only context's build: node boxes instead of node records (records_skipped)
    const Form nodes = records_skipped(c) ? NBOX : RECORDS;
    a.rec_on = nodes == RECORDS ? 1u : 0u;
    a.nbox = nodes == NBOX ? c->d_nbox.h : nullptr;
    if (c->T <= small_sort_max() && !(c->cfg.flags & RTBVH_FLAG_MULTI_KERNEL_BUILD)) {
        // the Morton pass and the sort in one workgroup (build.hip k_morton_sort_small; stage "morton")
        c->sorted = SortResult{c->d_ka, c->d_va};
        a.sorted_keys = c->d_ka;
        a.sorted_vals = c->d_va;
        launch_morton_sort_small(a, s);
        if (timing) HIPC(c, hipEventRecord(ev[2], s));
    } else {
        launch_morton(a, s);
        if (timing) HIPC(c, hipEventRecord(ev[2], s));
        c->sorted = radix_sort_pairs(c->d_codes, c->d_ids, c->d_ka, c->d_va, c->d_kb, c->d_vb, c->T, 30,
                                     c->d_sort_scratch, s);
    }
    if (timing) HIPC(c, hipEventRecord(ev[3], s));
    a.sorted_keys = c->sorted.keys;
    a.sorted_vals = c->sorted.vals;
    launch_karras(a, s);
    if (timing) HIPC(c, hipEventRecord(ev[4], s));
    // leaf records, boxes, node records and QNodes; rtbvh_compute_bvh's primary pass may start
    // after the leaves (ev_leaf)
    launch_refit_leaves(a, s);
    c->leaf_pending = false;
    if (handoff & LEAF_EVENT) {
        if (!c->side) {   // high priority: its workgroups go first while the crossing nodes' fill the CUs
            int lo = 0, hi = 0;
            HIPC(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
            if (!c->knob_side_priority) hi = lo;   // (A/B runs: RTBVH_SIDE_PRIORITY=0)
            HIPC(c, hipStreamCreateWithPriority(c->side.out(), hipStreamNonBlocking, hi));
        }
        if (!c->ev_leaf) HIPC(c, hipEventCreateWithFlags(c->ev_leaf.out(), hipEventDisableTiming));
        if (!c->ev_prim) HIPC(c, hipEventCreateWithFlags(c->ev_prim.out(), hipEventDisableTiming));
        HIPC(c, hipEventRecord(c->ev_leaf, s));
        c->leaf_pending = true;
    }
    if ((handoff & TAIL_TO_TRACE) && !c->leaf_pending) c->tail_pending = true;   // (the trace runs it: launch_pb_bin_tail)
    else launch_refit_tail(a, s);
    if (timing) HIPC(c, hipEventRecord(ev[5], s));
    if (timing) c->n_builds++;
    if (!c->capturing) HIPC(c, hipEventRecord(c->ev_built, s));
    // (the refit kernels quantize the QNodes)
    c->tree = Tree{true, clz64, nodes, (uint32_t)nodes | (a.pseudo ? PSEUDO : 0u) | QNODES};
    c->stale = false;
    return check_launch(c, "build kernels");
}

rtbvh_status rtbvh_build_async(rtbvh_ctx* c) { return c ? build_tree(c, 0) : RTBVH_ERR_INVALID_ARG; }

rtbvh_status rtbvh_build(rtbvh_ctx* c) {
    TRY(rtbvh_build_async(c));
    return rtbvh_synchronize(c);
}

rtbvh_status rtbvh_trace_async(rtbvh_ctx* c, uint32_t W, uint32_t H, uint32_t bounces) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    HIPC(c, hipSetDevice(c->cfg.device));
    TRY(ensure_trace_capacity(c, (size_t)W * H));
    return enqueue_trace(c, W, H, bounces, 0, 1, c->d_color, c->d_intensity, c->stream);
}

rtbvh_status rtbvh_trace(rtbvh_ctx* c, uint32_t W, uint32_t H, uint32_t bounces) {
    TRY(rtbvh_trace_async(c, W, H, bounces));
    return rtbvh_synchronize(c);
}

// The binned primary pass of rtbvh_compute_bvh on a side stream beside the build's crossing nodes
// (ev_leaf / ev_prim): opt-in (RTBVH_OVERLAP=1).  A/B at C5: the rocprof frame span 5.07 -> ~4.95
// ms in a process with the context's own stream, but bench.py's context (a torch stream, the slot
// streams of frames in flight) ran every build kernel of the frame up to 10x slower while the side
// queue held its wait (6.28 ms per frame against 5.14 without; 5.81 at normal priority), and as a
// hipGraph it was +-0 (4.98 / 4.99 / 5.00 ms).
// the crossing nodes a build left to the trace, when the trace did not run (an error on the way)
static rtbvh_status flush_tail(rtbvh_ctx* c, rtbvh_status st) {
    if (c->tail_pending) {
        launch_refit_tail(build_args(c), c->stream);
        c->tail_pending = false;
    }
    return st;
}

// rtbvh_compute_bvh's frame: the build hands its crossing nodes (and with RTBVH_OVERLAP its leaf event) to the trace
static rtbvh_status enqueue_frame(rtbvh_ctx* c, uint32_t W, uint32_t H, uint32_t bounces) {
    rtbvh_status st = build_tree(c, TAIL_TO_TRACE | (c->knob_overlap ? LEAF_EVENT : 0u));
    if (!st) st = rtbvh_trace_async(c, W, H, bounces);
    return flush_tail(c, st);
}

// RTBVH_FLAG_GRAPH: Graphics.cpp:56 rebuilds and traces every frame, ~20 launches and memsets
// of little work each on the reference's own meshes; the frame is captured once into a
// hipGraph and replayed.  A plain frame runs first so that every buffer exists before the
// capture; kernel arguments (sizes, buffers) are baked into the graph, hence the key and the
// drop on set_scene and reallocations.  The camera is not: the kernels read it from the
// context's camera buffer, updated before each replay (sync_camera), so a moving camera
// (Graphics::onKeyDown, Graphics.cpp:937-960) replays the same graph; and the certified walks
// (plan_trace) need no per-camera decision.
static rtbvh_status compute_graph(rtbvh_ctx* c, uint32_t W, uint32_t H, uint32_t bounces) {
    const uint64_t key[5] = {W, H, bounces, (uint64_t)c->cfg.flags | (uint64_t)c->T << 32,
                             (uint64_t)c->slots_used | (uint64_t)c->cfg.stack_limit << 1};
    if (!c->graph_exec || memcmp(key, c->graph_key, sizeof(key)) != 0) {
        drop_graph(c);
        rtbvh_status st = enqueue_frame(c, W, H, bounces);
        if (!st) st = rtbvh_synchronize(c);
        if (st && st != RTBVH_ERR_STACK_OVERFLOW) return st;
        HIPC(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        c->capturing = true;
        st = enqueue_frame(c, W, H, bounces);
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(c->stream, &g);
        c->capturing = false;
        if (st || e != hipSuccess) {
            if (g) (void)hipGraphDestroy(g);
            return st ? st : fail(c, RTBVH_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        }
        c->graph = g;
        HIPC(c, hipGraphInstantiate(&c->graph_exec, g, nullptr, nullptr, 0));
        memcpy(c->graph_key, key, sizeof(key));
        // (a whole frame into the framebuffer on the context stream: rank 0 of 1, set 0, frame and intensities here)
        c->graph_trace = c->last;
        c->graph_tree = c->tree;   // (the forms the captured trace derived are in the graph too)
        c->graph_captures++;
    }
    // the replayed build rewrites the BVH and the bin set of the context stream's buffer set (the replayed
    // trace fills it), with this frame's camera: as build_tree
    TRY(before_tree_write(c, c->stream));
    HIPC(c, hipGraphLaunch(c->graph_exec, c->stream));
    HIPC(c, hipEventRecord(c->ev_built, c->stream));
    // the host-side state of the captured frame: its tree (the replayed build rewrote it for this camera, so
    // whatever was derived since belongs to the old one) and its trace (one in between may have changed it)
    c->tree = c->graph_tree;
    c->stale = false;
    c->last = c->graph_trace;
    if (c->last.cert) c->cert_traces++;
    return rtbvh_synchronize(c);
}

rtbvh_status rtbvh_compute_bvh(rtbvh_ctx* c, uint32_t W, uint32_t H, uint32_t bounces) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    if (c->cfg.flags & RTBVH_FLAG_GRAPH) return compute_graph(c, W, H, bounces);
    TRY(enqueue_frame(c, W, H, bounces));
    return rtbvh_synchronize(c);
}

// ---- animated geometry: vertex updates and the topology-keeping refit -----------------------
static rtbvh_status check_update(rtbvh_ctx* c, const float* positions, uint32_t pos_stride, const float* normals,
                                 uint32_t nrm_stride, uint32_t first, uint32_t count) {
    if (!positions) return fail(c, RTBVH_ERR_INVALID_ARG, "update_vertices: NULL positions");
    if (pos_stride < 3 || (normals && nrm_stride < 3))
        return fail(c, RTBVH_ERR_INVALID_ARG, "update_vertices: a stride below 3 floats");
    if (!c->have_scene) return fail(c, RTBVH_ERR_NOT_READY, "update_vertices before set_scene");
    if (first > c->V || count > c->V - first)
        return fail(c, RTBVH_ERR_INVALID_ARG, "update_vertices: first + count exceeds the scene's vertices");
    return RTBVH_OK;
}

// One kernel (two with the mesh box's final reduction) on the caller's stream, behind the frames in flight -- they
// read the normals -- and the context stream's work so far (a build reads the positions and the box, a trace the
// normals); nothing is reallocated, nothing waits on the host, and a captured frame stays: its kernels read the
// same buffers.
rtbvh_status rtbvh_update_vertices_async(rtbvh_ctx* c, const float* dev_positions, uint32_t pos_stride,
                                         const float* dev_normals, uint32_t nrm_stride, uint32_t first,
                                         uint32_t count, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    if (count == 0) return RTBVH_OK;
    TRY(check_update(c, dev_positions, pos_stride, dev_normals, nrm_stride, first, count));
    HIPC(c, hipSetDevice(c->cfg.device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (!c->ev_update) HIPC(c, hipEventCreateWithFlags(c->ev_update.out(), hipEventDisableTiming));
    TRY(wait_slots(c, s));
    TRY(order_after_context(c, s));
    TRY(wait_update(c, s));   // (an earlier update on another stream wrote the same buffers)
    VertexUpdate u{};
    u.pos = dev_positions;
    u.pos_stride = pos_stride;
    u.nrm = dev_normals;
    u.nrm_stride = nrm_stride;
    u.first = first;
    u.count = count;
    u.opos = c->d_opos;
    u.verts = c->d_verts;
    u.bounds = c->cfg.morton_mode == RTBVH_MORTON_CPUTESTS ? c->d_bounds.h : nullptr;
    u.V = c->V;
    launch_update_vertices(u, s);
    const rtbvh_status st = check_launch(c, "vertex update");
    HIPC(c, hipEventRecord(c->ev_update, s));
    c->update_pending = true;
    c->stale = c->tree.built;
    return st;
}

rtbvh_status rtbvh_update_vertices_host(rtbvh_ctx* c, const float* positions, uint32_t pos_stride,
                                        const float* normals, uint32_t nrm_stride, uint32_t first, uint32_t count) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    if (count == 0) return RTBVH_OK;
    TRY(check_update(c, positions, pos_stride, normals, nrm_stride, first, count));
    HIPC(c, hipSetDevice(c->cfg.device));
    // the arrays as they are, strides included: the last vertex's three floats end each
    const size_t np = (size_t)(count - 1) * pos_stride + 3, nn = normals ? (size_t)(count - 1) * nrm_stride + 3 : 0;
    DevBuf<float> d;
    HIPC(c, d.alloc(np + nn));
    HIPC(c, hipMemcpy(d, positions, np * sizeof(float), hipMemcpyHostToDevice));
    if (normals) HIPC(c, hipMemcpy(d + np, normals, nn * sizeof(float), hipMemcpyHostToDevice));
    TRY(rtbvh_update_vertices_async(c, d, pos_stride, normals ? d + np : nullptr, nrm_stride, first, count, nullptr));
    HIPC(c, hipStreamSynchronize(c->stream));   // (the staging buffer goes with this scope)
    return RTBVH_OK;
}

// New boxes over the last build's sort order and topology (sorted, topo, pleaf, pint stay): the clip-space
// triangles of the current positions and camera (k_morton<false>), then the build's own refit stages, which write
// everything downstream -- leaf records and footprints, node records or node boxes in the form the build wrote
// (and the leaf pseudo-records if the tree had them), the QNodes with their margin codes, the root box with
// its depth range and edge bound.  A one-workgroup build (k_build_small) leaves the same arrays, so its tree
// is refitted by the same kernels.  Forms derived since the build (ensure_form) are of the old boxes: dropped.
rtbvh_status rtbvh_refit_async(rtbvh_ctx* c) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    if (!c->have_scene || !c->tree.built) return fail(c, RTBVH_ERR_NOT_READY, "refit before build");
    HIPC(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    TRY(before_tree_write(c, s));   // (frames in flight and ray queries read the old boxes)
    BuildArgs a = build_args(c);
    a.pseudo = a.rec_on && (c->tree.valid & PSEUDO) ? 1u : 0u;
    launch_clip(a, s);
    launch_refit_leaves(a, s);
    launch_refit_tail(a, s);
    c->leaf_pending = c->tail_pending = false;
    HIPC(c, hipEventRecord(c->ev_built, s));
    c->tree.valid = (uint32_t)c->tree.wrote | (a.pseudo ? PSEUDO : 0u) | QNODES;
    c->stale = false;
    return check_launch(c, "refit kernels");
}

rtbvh_status rtbvh_refit(rtbvh_ctx* c) {
    TRY(rtbvh_refit_async(c));
    return rtbvh_synchronize(c);
}

// The identity check of a fast walk (DESIGN.md "Traversal orders"): the frame in the
// reference order (the exact findCollision DFS, RayTraceTraversal.hlsl:106-193) into a
// scratch buffer, then the frame with the context's walks into the framebuffer, compared
// on the device.  Leaves the context as rtbvh_trace with its own flags does.
rtbvh_status rtbvh_verify_walk(rtbvh_ctx* c, uint32_t W, uint32_t H, uint32_t bounces, uint64_t* differing) {
    if (!c || !differing) return RTBVH_ERR_INVALID_ARG;
    if (!c->tree.built) return fail(c, RTBVH_ERR_NOT_READY, "verify_walk before build");
    if (c->stale) return fail_stale(c, "verify_walk");
    if (W == 0 || H == 0 || bounces > 14) return fail(c, RTBVH_ERR_INVALID_ARG, "bad trace dimensions");
    HIPC(c, hipSetDevice(c->cfg.device));
    TRY(ensure_trace_capacity(c, (size_t)W * H));
    const size_t n = (size_t)W * H;
    float4* ref = nullptr;
    unsigned long long* d_diff = nullptr;
    HIPC(c, hipMallocAsync((void**)&ref, n * sizeof(float4) + 256, c->stream));
    d_diff = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ref) + n * sizeof(float4));
    // the reference order, then the walks the context takes (AUTO: the certified fast walks above
    // AUTO_WALK_MAX_TRIS), without the ray records
    const uint32_t f = c->cfg.flags & ~RTBVH_FLAG_REFRACT_RECORDS;
    const uint32_t refw = f & ~(WALK_FLAGS | RTBVH_FLAG_AUTO_WALK);
    const TracePlan mine = plan_trace(c, f);
    rtbvh_status st = sync_camera(c, c->stream);
    if (!st) st = enqueue_walks(c, W, H, bounces, 0, 1, ref, nullptr, c->stream, 0, refw, true, mine.state);
    if (!st)
        st = enqueue_walks(c, W, H, bounces, 0, 1, c->d_color, c->d_intensity, c->stream, 0, mine.flags, true,
                           mine.state, mine.cert);
    unsigned long long diff = 0;
    if (!st) {
        hipError_t e = hipMemsetAsync(d_diff, 0, sizeof(unsigned long long), c->stream);
        if (e == hipSuccess) {
            launch_count_diff(ref, c->d_color, n, d_diff, c->stream);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&diff, d_diff, sizeof(diff), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) st = fail(c, RTBVH_ERR_HIP, std::string("verify_walk: ") + hipGetErrorString(e));
    }
    (void)hipFreeAsync(ref, c->stream);
    if (st) return st;
    *differing = diff;
    return rtbvh_synchronize(c);
}

uint32_t rtbvh_band_rows(uint32_t H, uint32_t rank, uint32_t nranks) { return deal_rows(H, rank, nranks, 16); }

uint32_t rtbvh_deal_rows(uint32_t H, uint32_t rank, uint32_t nranks, uint32_t root_share) {
    return root_share > 16 ? 0 : deal_rows(H, rank, nranks, root_share);
}

uint32_t rtbvh_deal_bands(uint32_t H, uint32_t rank, uint32_t nranks, uint32_t root_share, uint32_t* bands,
                          uint32_t capacity) {
    if (nranks == 0 || rank >= nranks || root_share > 16) return 0;
    std::vector<uint32_t> owner;
    if (root_share == 16 || nranks == 1) {
        owner.resize((H + 7) / 8);
        for (uint32_t b = 0; b < owner.size(); b++) owner[b] = b % nranks;
    } else {
        deal_owners(H, nranks, root_share, owner);
    }
    uint32_t n = 0;
    for (uint32_t b = 0; b < owner.size(); b++)
        if (owner[b] == rank) {
            if (bands && n < capacity) bands[n] = b;
            n++;
        }
    return n;
}

rtbvh_status rtbvh_set_band_deal(rtbvh_ctx* c, uint32_t root_share) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    if (root_share > 16) return fail(c, RTBVH_ERR_INVALID_ARG, "set_band_deal: root_share > 16");
    c->root_share = root_share;
    return RTBVH_OK;
}

rtbvh_status rtbvh_trace_band_async(rtbvh_ctx* c, uint32_t W, uint32_t H, uint32_t bounces, uint32_t rank,
                                    uint32_t nranks, float* dev_out, void* stream) {
    if (!c || !dev_out) return RTBVH_ERR_INVALID_ARG;
    HIPC(c, hipSetDevice(c->cfg.device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    uint32_t slot = 0;
    if (s != c->stream) {   // a frame in flight: this stream's buffer set, after the last build
        for (uint32_t k = 1; k < rtbvh_ctx::MAXSPLIT && !slot; k++)
            if (c->sets[k].caller == s) slot = k;
        for (uint32_t k = 1; k < rtbvh_ctx::MAXSPLIT && !slot; k++)
            if (!c->sets[k].caller) {
                c->sets[k].caller = s;
                slot = k;
            }
        if (!slot) return fail(c, RTBVH_ERR_INVALID_ARG, "more caller streams trace one context than it has slots");
        Event& done = c->sets[slot].done;
        if (!done) HIPC(c, hipEventCreateWithFlags(done.out(), hipEventDisableTiming));
        c->slots_used = true;
        HIPC(c, hipStreamWaitEvent(s, c->ev_built, 0));
    }
    TRY(enqueue_trace(c, W, H, bounces, rank, nranks, (float4*)dev_out, nullptr, s, slot));
    if (slot) {   // the next build (context stream) waits for this trace
        HIPC(c, hipEventRecord(c->sets[slot].done, s));
        c->sets[slot].busy = true;
    }
    return RTBVH_OK;
}

rtbvh_status rtbvh_assemble_bands(rtbvh_ctx* c, uint32_t W, uint32_t H, uint32_t nranks, const float* dev_bands,
                                  uint32_t stride_rows, float* dev_frame, void* stream) {
    if (!c || !dev_bands || !dev_frame || W == 0 || H == 0 || nranks == 0 ||
        stride_rows < deal_max_rows(H, nranks, c->root_share))
        return RTBVH_ERR_INVALID_ARG;
    HIPC(c, hipSetDevice(c->cfg.device));
    const rtbvh_ctx::DealTab* deal = nullptr;
    const hipStream_t as = stream ? (hipStream_t)stream : c->stream;
    TRY(get_deal(c, H, nranks, &deal, as));
    launch_assemble((const float4*)dev_bands, deal ? deal->d + (H + 7) / 8 : nullptr, stride_rows, W, H, nranks,
                    (float4*)dev_frame, as);
    return check_launch(c, "assemble bands");
}

rtbvh_status rtbvh_comm_unique_id(uint8_t id[RTBVH_COMM_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == RTBVH_COMM_ID_BYTES, "ncclUniqueId is 128 B");
    if (!id) return RTBVH_ERR_INVALID_ARG;
    const Rccl& r = rccl();
    if (!r.ok) return fail(nullptr, RTBVH_ERR_COMM, r.err);
    ncclUniqueId u;
    const ncclResult_t e = r.GetUniqueId(&u);
    if (e != ncclSuccess) return fail(nullptr, RTBVH_ERR_COMM, std::string("ncclGetUniqueId: ") + r.GetErrorString(e));
    memcpy(id, &u, sizeof(u));
    return RTBVH_OK;
}

rtbvh_status rtbvh_comm_init(rtbvh_ctx* c, uint32_t nranks, uint32_t rank, const uint8_t id[RTBVH_COMM_ID_BYTES],
                             void** comm) {
    if (!c || !id || !comm || nranks == 0 || rank >= nranks) return RTBVH_ERR_INVALID_ARG;
    const Rccl& r = rccl();
    if (!r.ok) return fail(c, RTBVH_ERR_COMM, r.err);
    HIPC(c, hipSetDevice(c->cfg.device));
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t cm = nullptr;
    const ncclResult_t e = r.CommInitRank(&cm, (int)nranks, u, (int)rank);
    if (e != ncclSuccess) return fail(c, RTBVH_ERR_COMM, std::string("ncclCommInitRank: ") + r.GetErrorString(e));
    *comm = cm;
    return RTBVH_OK;
}

rtbvh_status rtbvh_comm_destroy(void* comm) {
    if (!comm) return RTBVH_ERR_INVALID_ARG;
    const Rccl& r = rccl();
    if (!r.ok) return fail(nullptr, RTBVH_ERR_COMM, r.err);
    const ncclResult_t e = r.CommDestroy((ncclComm_t)comm);
    if (e != ncclSuccess) return fail(nullptr, RTBVH_ERR_COMM, std::string("ncclCommDestroy: ") + r.GetErrorString(e));
    return RTBVH_OK;
}

// bands of 8 rows dealt by the context's deal (rtbvh_set_band_deal); one RCCL
// group of point-to-point transfers into rank 0 (xGMI is point to point: each rank's shard
// travels its own link), then the row scatter on rank 0.  Rank 0's buffer holds every rank's
// bands, rank r at r * rows0 rows (rows0 = the most band rows any rank has).
rtbvh_status rtbvh_trace_tiles(rtbvh_ctx* c, uint32_t W, uint32_t H, uint32_t bounces, uint32_t rank,
                               uint32_t nranks, void* comm) {
    if (!c || !comm || W == 0 || H == 0 || nranks == 0 || rank >= nranks) return RTBVH_ERR_INVALID_ARG;
    const Rccl& r = rccl();
    if (!r.ok) return fail(c, RTBVH_ERR_COMM, r.err);
    HIPC(c, hipSetDevice(c->cfg.device));
    const uint32_t rows0 = deal_max_rows(H, nranks, c->root_share);
    const size_t need = (size_t)(rank == 0 ? nranks : 1) * rows0 * W;
    HIPC(c, c->d_band.reserve(need));
    TRY(enqueue_trace(c, W, H, bounces, rank, nranks, c->d_band, nullptr, c->stream));
    const ncclComm_t cm = (ncclComm_t)comm;
    ncclResult_t e = r.GroupStart();
    if (rank != 0) {
        if (e == ncclSuccess)
            e = r.Send(c->d_band, (size_t)deal_rows(H, rank, nranks, c->root_share) * W * 4, ncclFloat32, 0, cm,
                       c->stream);
    } else {
        for (uint32_t q = 1; q < nranks && e == ncclSuccess; q++)
            e = r.Recv(c->d_band + (size_t)q * rows0 * W, (size_t)deal_rows(H, q, nranks, c->root_share) * W * 4,
                       ncclFloat32,
                       (int)q, cm, c->stream);
    }
    const ncclResult_t e2 = r.GroupEnd();
    if (e == ncclSuccess) e = e2;
    if (e != ncclSuccess) return fail(c, RTBVH_ERR_COMM, std::string("band gather: ") + r.GetErrorString(e));
    if (rank == 0) {
        const rtbvh_ctx::DealTab* deal = nullptr;
        TRY(get_deal(c, H, nranks, &deal, c->stream));
        launch_assemble(c->d_band, deal ? deal->d + (H + 7) / 8 : nullptr, rows0, W, H, nranks, c->d_color,
                        c->stream);
        TRY(check_launch(c, "assemble bands"));
    }
    c->last.frame_here = rank == 0;   // (assembled)
    return rtbvh_synchronize(c);
}

rtbvh_status rtbvh_synchronize(rtbvh_ctx* c) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    TRY(sync_all(c));
    c->q.busy = false;
    // each trace ends by copying the never-reset overflow word into its slot's pinned word
    unsigned long long ovf = c->ovf_seen;
    for (uint32_t k = 0; k < rtbvh_ctx::MAXSPLIT; k++)
        if (c->h_ovf[k] > ovf) ovf = c->h_ovf[k];
    if (c->q.ovf) {   // queries run on any stream: the word itself, once they are all done
        unsigned long long v = 0;
        HIPC(c, hipMemcpy(&v, c->d_ovf, sizeof(v), hipMemcpyDeviceToHost));
        c->q.ovf = false;
        if (v > ovf) ovf = v;
    }
    if (ovf > c->ovf_seen) {
        const unsigned long long n = ovf - c->ovf_seen;
        c->ovf_seen = ovf;
        return fail(c, RTBVH_ERR_STACK_OVERFLOW,
                    "traversal stack overflow: " + std::to_string(n) +
                        " event(s) -- a per-lane walk's ray ended early, or a packet walk skipped a subtree "
                        "for the rays that hit it; each keeps the best hit found so far (stack limit " +
                        std::to_string(c->cfg.stack_limit ? c->cfg.stack_limit : (uint32_t)STACK_SIZE) +
                        " entries; the reference's 32-entry stack is unchecked, RayTraceTraversal.hlsl:9,115)");
    }
    return RTBVH_OK;
}

rtbvh_status rtbvh_read_framebuffer(rtbvh_ctx* c, float* rgba) {
    if (!c || !rgba) return RTBVH_ERR_INVALID_ARG;
    if (!c->last.traced) return fail(c, RTBVH_ERR_NOT_READY, "no trace yet");
    if (!c->last.frame_here)
        return fail(c, RTBVH_ERR_NOT_READY, "the last trace was a band trace: the frame is elsewhere");
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(rgba, c->d_color, sizeof(float4) * (size_t)c->last.W * c->last.H, hipMemcpyDeviceToHost));
    return RTBVH_OK;
}

rtbvh_status rtbvh_read_intensity(rtbvh_ctx* c, float* inten) {
    if (!c || !inten) return RTBVH_ERR_INVALID_ARG;
    if (!c->last.traced || !c->last.intensity_here) return fail(c, RTBVH_ERR_NOT_READY, "no full-frame trace yet");
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(inten, c->d_intensity, sizeof(float) * (size_t)c->last.W * c->last.H, hipMemcpyDeviceToHost));
    return RTBVH_OK;
}

const float* rtbvh_framebuffer_device(rtbvh_ctx* c) { return c ? (const float*)c->d_color.h : nullptr; }

rtbvh_status rtbvh_read_bvh(rtbvh_ctx* c, rtbvh_node* out, uint32_t capacity) {
    if (!c || !out) return RTBVH_ERR_INVALID_ARG;
    if (!c->tree.built) return fail(c, RTBVH_ERR_NOT_READY, "no build yet");
    const size_t total = 2 * (size_t)c->T - 1;
    if (capacity < total) return fail(c, RTBVH_ERR_INVALID_ARG, "read_bvh: capacity < 2n-1");
    HIPC(c, hipSetDevice(c->cfg.device));
    void* tmp = nullptr;
    HIPC(c, hipMalloc(&tmp, total * sizeof(rtbvh_node)));
    BuildArgs a = build_args(c);
    launch_export(a, tmp, c->stream);
    hipError_t e1 = hipGetLastError();
    hipError_t e2 = hipStreamSynchronize(c->stream);
    hipError_t e3 = hipMemcpy(out, tmp, total * sizeof(rtbvh_node), hipMemcpyDeviceToHost);
    (void)hipFree(tmp);
    HIPC(c, e1);
    HIPC(c, e2);
    HIPC(c, e3);
    return RTBVH_OK;
}

rtbvh_status rtbvh_present(rtbvh_ctx* c, uint8_t* rgba8) {
    if (!c || !rgba8) return RTBVH_ERR_INVALID_ARG;
    if (!c->last.traced || !c->last.frame_here)
        return fail(c, RTBVH_ERR_NOT_READY, "present: no full frame on this context");
    HIPC(c, hipSetDevice(c->cfg.device));
    const size_t n = (size_t)c->last.W * c->last.H;
    uint32_t* d = nullptr;
    HIPC(c, hipMallocAsync((void**)&d, n * 4, c->stream));
    launch_present(c->d_color, c->last.W, c->last.H, d, c->stream);
    hipError_t e1 = hipGetLastError();
    hipError_t e2 = hipMemcpyAsync(rgba8, d, n * 4, hipMemcpyDeviceToHost, c->stream);
    hipError_t e3 = hipFreeAsync(d, c->stream);
    hipError_t e4 = hipStreamSynchronize(c->stream);
    HIPC(c, e1);
    HIPC(c, e2);
    HIPC(c, e3);
    HIPC(c, e4);
    return RTBVH_OK;
}

rtbvh_status rtbvh_read_wide(rtbvh_ctx* c, uint32_t* out, uint64_t capacity) {
    if (!c || !out) return RTBVH_ERR_INVALID_ARG;
    if (!c->tree.built) return fail(c, RTBVH_ERR_NOT_READY, "no build yet");
    const size_t total = c->T > 1 ? 2 * (size_t)(c->T - 1) : 0;
    if (capacity < total) return fail(c, RTBVH_ERR_INVALID_ARG, "read_wide: capacity < 2(n-1)");
    HIPC(c, hipSetDevice(c->cfg.device));
    TRY(ensure_form(c, RECORDS, c->stream));   // (a certified-only build wrote node boxes instead)
    TRY(ensure_form(c, PSEUDO, c->stream));    // (binned / AUTO walks: a build without them)
    HIPC(c, hipStreamSynchronize(c->stream));
    if (total) HIPC(c, hipMemcpy(out, c->d_rec, total * sizeof(Inner), hipMemcpyDeviceToHost));
    return RTBVH_OK;
}

rtbvh_status rtbvh_read_qnodes(rtbvh_ctx* c, uint32_t* out, uint64_t capacity) {
    if (!c || !out) return RTBVH_ERR_INVALID_ARG;
    if (!c->tree.built) return fail(c, RTBVH_ERR_NOT_READY, "no build yet");
    const size_t total = c->T > 1 ? 2 * (size_t)c->T - 1 : 0;
    if (capacity < total) return fail(c, RTBVH_ERR_INVALID_ARG, "read_qnodes: capacity < 2n-1");
    HIPC(c, hipSetDevice(c->cfg.device));
    TRY(ensure_form(c, QNODES, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (total) HIPC(c, hipMemcpy(out, c->d_qnode, total * sizeof(QNode), hipMemcpyDeviceToHost));
    return RTBVH_OK;
}

rtbvh_status rtbvh_read_walk_qnodes(rtbvh_ctx* c, uint32_t* out, uint64_t capacity) {
    if (!c || !out) return RTBVH_ERR_INVALID_ARG;
    const WalkTreeBufs& w = c->wt;
    if (!c->tree.built || !(w.valid && w.epoch == c->bins_epoch && w.T == c->T))
        return fail(c, RTBVH_ERR_NOT_READY, "read_walk_qnodes: no walk-only tree of the current build");
    const uint64_t total = 2 * (uint64_t)c->T - 1;
    if (capacity < total) return fail(c, RTBVH_ERR_INVALID_ARG, "read_walk_qnodes: capacity < 2n-1");
    HIPC(c, hipSetDevice(c->cfg.device));
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(out, w.qnode, total * sizeof(QNode), hipMemcpyDeviceToHost));
    return RTBVH_OK;
}

rtbvh_status rtbvh_read_morton(rtbvh_ctx* c, uint32_t* codes) {
    if (!c || !codes) return RTBVH_ERR_INVALID_ARG;
    if (!c->tree.built) return fail(c, RTBVH_ERR_NOT_READY, "no build yet");
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(codes, c->d_codes, sizeof(uint32_t) * c->T, hipMemcpyDeviceToHost));
    return RTBVH_OK;
}

rtbvh_status rtbvh_read_sorted(rtbvh_ctx* c, uint32_t* keys, uint32_t* ids) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    if (!c->tree.built) return fail(c, RTBVH_ERR_NOT_READY, "no build yet");
    HIPC(c, hipStreamSynchronize(c->stream));
    if (keys) HIPC(c, hipMemcpy(keys, c->sorted.keys, sizeof(uint32_t) * c->T, hipMemcpyDeviceToHost));
    if (ids) HIPC(c, hipMemcpy(ids, c->sorted.vals, sizeof(uint32_t) * c->T, hipMemcpyDeviceToHost));
    return RTBVH_OK;
}

rtbvh_status rtbvh_read_rays(rtbvh_ctx* c, rtbvh_ray_present* reflect_out, rtbvh_ray_present* refract_out) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    if (!c->last.traced || c->last.rec_P == 0)
        return fail(c, RTBVH_ERR_NOT_READY, "read_rays: the last trace ran without RTBVH_FLAG_REFRACT_RECORDS");
    HIPC(c, hipSetDevice(c->cfg.device));
    HIPC(c, hipStreamSynchronize(c->stream));
    const size_t bytes = c->last.rec_P * sizeof(rtbvh_ray_present);
    if (reflect_out) HIPC(c, hipMemcpy(reflect_out, c->d_refl_rec, bytes, hipMemcpyDeviceToHost));
    if (refract_out) HIPC(c, hipMemcpy(refract_out, c->d_refr_rec, bytes, hipMemcpyDeviceToHost));
    return RTBVH_OK;
}

rtbvh_status rtbvh_get_stats(rtbvh_ctx* c, rtbvh_stats* out) {
    if (!c || !out) return RTBVH_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    if (rtbvh_status st = sync_all(c)) return st;
    out->num_tris = c->T;
    out->num_nodes = c->T ? 2 * c->T - 1 : 0;
    const LastTrace& t = c->last;
    const TraceSet& set = c->sets[t.slot];   // the last trace's (chain 0's) set
    out->width = t.W;
    out->height = t.H;
    const uint32_t nb = c->n_builds < (uint32_t)rtbvh_ctx::RING ? c->n_builds : rtbvh_ctx::RING;
    for (uint32_t k = 0; k < nb; k++) {
        float ms;
        HIPC(c, hipEventElapsedTime(&ms, c->evb[k][0], c->evb[k][5]));
        out->ms_build += ms / nb;
        for (int st = 0; st < 5; st++) {
            HIPC(c, hipEventElapsedTime(&ms, c->evb[k][st], c->evb[k][st + 1]));
            out->ms_stage[st] += ms / nb;
        }
    }
    out->timed_builds = nb;
    const uint32_t nt = c->n_traces < (uint32_t)rtbvh_ctx::RING ? c->n_traces : rtbvh_ctx::RING;
    for (uint32_t k = 0; k < nt; k++) {
        float ms;
        HIPC(c, hipEventElapsedTime(&ms, c->evt[k][0], c->evt[k][2]));
        out->ms_trace += ms / nt;
        HIPC(c, hipEventElapsedTime(&ms, c->evt[k][0], c->evt[k][1]));
        out->ms_stage[5] += ms / nt;
        HIPC(c, hipEventElapsedTime(&ms, c->evt[k][1], c->evt[k][2]));
        out->ms_stage[6] += ms / nt;
        if (c->evt_trav[k]) {
            HIPC(c, hipEventElapsedTime(&ms, c->evt[k][3], c->evt[k][4]));
            out->ms_stage[7] += ms / nt;
        }
    }
    out->timed_traces = nt;
    if (t.traced && set.counters) {
        unsigned long long cnt[64];
        uint32_t q[32 * rtbvh_ctx::MAXSPLIT];   // (its chains' sets follow it)
        HIPC(c, hipMemcpy(cnt, set.counters, sizeof(cnt), hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(q, set.qcount, sizeof(uint32_t) * 32 * t.nsplit, hipMemcpyDeviceToHost));
        out->primary_rays = (uint64_t)t.W * deal_rows(t.H, t.rank, t.nranks, c->root_share);
        uint64_t b = 0;
        for (uint32_t g = 0; g < t.nsplit; g++)
            for (uint32_t k = 0; k < t.bounces; k++) b += q[32 * g + k];
        out->bounce_rays = b;
        for (int p = 0; p < 2; p++) {
            out->internal_visits[p] = cnt[2 + 3 * p];
            out->leaf_visits[p] = cnt[3 + 3 * p];
            out->hits[p] = cnt[4 + 3 * p];
        }
        out->stack_overflows = cnt[8];
        out->textured_hits = cnt[9];
        out->trav_wave_steps = cnt[10];
        out->trav_max_steps = cnt[13];
        out->trav_longest = cnt[20];
        for (int k = 0; k < 32; k++) out->trav_steps_log2[k] = cnt[32 + k];
        out->trav_mixed_steps = cnt[11];
        out->trav_active_lanes = cnt[12];
        for (int p = 0; p < 2; p++) {
            out->packet_steps[p] = cnt[14 + p];
            out->bin_entries[p] = cnt[16 + p];
        }
    }
    out->graph_captures = c->graph_captures;
    out->walk_flags = t.walk;
    out->walk_state = t.walk_state;
    out->cert_traces = c->cert_traces;
    if (t.traced && t.cert && set.qcount) {   // the last trace's re-trace counts (qcount 16..)
        uint32_t q[32];
        HIPC(c, hipMemcpy(q, set.qcount, sizeof(q), hipMemcpyDeviceToHost));
        out->redo_rays[0] = q[16];
        for (uint32_t k = 0; k < t.bounces && k < 15; k++) out->redo_rays[1] += q[17 + k];
        // ... and the bounce walks' deferred rays (walked in the reference order by the walk or k_bounce_redo)
        for (uint32_t k = 0; k < t.bounces && k < 15; k++) {
            uint32_t nd = 0;
            HIPC(c, hipMemcpy(&nd, set.next + (size_t)NEXT_SEGS * NEXT_STRIDE * k + DEFER_COUNT, sizeof(nd),
                              hipMemcpyDeviceToHost));
            out->redo_rays[1] += nd;
            out->redo_deferred += nd;
        }
    }
    out->redo_total = out->redo_rays[0] + out->redo_rays[1];
    out->walk_tree_builds = c->walk_tree_builds;
    out->walk_tree_used = t.traced && t.walk_tree ? 1u : 0u;
    return RTBVH_OK;
}

uint64_t rtbvh_bin_builds(rtbvh_ctx* c) { return c ? c->bin_builds : 0; }

uint32_t rtbvh_bin_sets(rtbvh_ctx* c) {
    uint32_t n = 0;
    for (uint32_t k = 0; c && k < rtbvh_ctx::MAXSPLIT; k++) n += c->sets[k].pb.bins ? 1u : 0u;
    return n;
}

rtbvh_status rtbvh_set_flags(rtbvh_ctx* c, uint32_t flags) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    c->cfg.flags = flags;
    return RTBVH_OK;
}

rtbvh_status rtbvh_reset_stats(rtbvh_ctx* c) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    HIPC(c, hipStreamSynchronize(c->stream));
    c->n_builds = 0;
    c->n_traces = 0;
    return RTBVH_OK;
}

rtbvh_status rtbvh_sort_pairs_async(rtbvh_ctx* c, uint32_t* kin, uint32_t* vin, uint32_t* kout, uint32_t* vout,
                                    uint32_t n, uint32_t key_bits) {
    if (!c || (n && (!kin || !vin || !kout || !vout)) || key_bits == 0 || key_bits > 32)
        return RTBVH_ERR_INVALID_ARG;
    if (n == 0) return RTBVH_OK;
    HIPC(c, hipSetDevice(c->cfg.device));
    const uint32_t passes = (key_bits + RADIX_BITS - 1) / RADIX_BITS;
    uint32_t *tk = nullptr, *tv = nullptr, *scratch = nullptr;
    HIPC(c, hipMallocAsync((void**)&scratch, sort_scratch_words(n) * 4, c->stream));
    if (passes > 1) {
        HIPC(c, hipMallocAsync((void**)&tk, (size_t)n * 4, c->stream));
        HIPC(c, hipMallocAsync((void**)&tv, (size_t)n * 4, c->stream));
    }
    // odd pass count ends in A, even in B: arrange for the result to land in (kout, vout)
    if (passes & 1) radix_sort_pairs(kin, vin, kout, vout, tk, tv, n, key_bits, scratch, c->stream);
    else radix_sort_pairs(kin, vin, tk, tv, kout, vout, n, key_bits, scratch, c->stream);
    rtbvh_status st = check_launch(c, "sort kernels");
    (void)hipFreeAsync(scratch, c->stream);
    if (tk) (void)hipFreeAsync(tk, c->stream);
    if (tv) (void)hipFreeAsync(tv, c->stream);
    return st;
}

rtbvh_status rtbvh_sort_pairs_host(rtbvh_ctx* c, const uint32_t* keys, const uint32_t* vals, uint32_t* kout,
                                   uint32_t* vout, uint32_t n, uint32_t key_bits) {
    if (!c || (n && (!keys || !vals || !kout || !vout))) return RTBVH_ERR_INVALID_ARG;
    if (n == 0) return RTBVH_OK;
    HIPC(c, hipSetDevice(c->cfg.device));
    uint32_t* d = nullptr;
    HIPC(c, hipMalloc((void**)&d, (size_t)n * 16));
    uint32_t *dk = d, *dv = d + n, *ok = d + 2 * (size_t)n, *ov = d + 3 * (size_t)n;
    rtbvh_status st = RTBVH_OK;
    if (hipMemcpy(dk, keys, (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dv, vals, (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess)
        st = fail(c, RTBVH_ERR_HIP, "sort_pairs_host: upload failed");
    if (!st) st = rtbvh_sort_pairs_async(c, dk, dv, ok, ov, n, key_bits);
    if (!st && hipStreamSynchronize(c->stream) != hipSuccess) st = fail(c, RTBVH_ERR_HIP, "sort_pairs_host: sync");
    if (!st && (hipMemcpy(kout, ok, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(vout, ov, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess))
        st = fail(c, RTBVH_ERR_HIP, "sort_pairs_host: download failed");
    (void)hipFree(d);
    return st;
}

rtbvh_status rtbvh_build_from_codes(rtbvh_ctx* c, const uint32_t* sorted_codes, const float* leaf_boxes, uint32_t n,
                                    rtbvh_node* out) {
    if (!c || !sorted_codes || !leaf_boxes || !out || n == 0 || n >= (1u << 30)) return RTBVH_ERR_INVALID_ARG;
    HIPC(c, hipSetDevice(c->cfg.device));
    if (c->q.ev) HIPC(c, hipEventSynchronize(c->q.ev));   // (the scene's BVH buffers are reused)
    c->q.busy = false;
    TRY(ensure_build_capacity(c, n));
    DevBuf<float> d_boxes;
    DevBuf<rtbvh_node> d_out;
    HIPC(c, d_boxes.alloc((size_t)n * 6));
    HIPC(c, d_out.alloc(2 * (size_t)n - 1));
    reset_tree(c);   // the scene's BVH buffers are reused from here on
    HIPC(c, hipMemcpy(c->d_ka, sorted_codes, (size_t)n * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_boxes, leaf_boxes, (size_t)n * 24, hipMemcpyHostToDevice));
    BuildArgs a = build_args(c);
    a.T = n;
    a.sorted_keys = c->d_ka;
    a.sorted_vals = nullptr;
    a.leaf = nullptr;
    a.rec_on = 1;   // (its QNodes and export read the records)
    a.nbox = nullptr;
    launch_from_codes(a, d_boxes, c->stream);
    launch_export(a, d_out, c->stream);
    const rtbvh_status st = check_launch(c, "build_from_codes kernels");
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (st) return st;
    HIPC(c, e);
    HIPC(c, hipMemcpy(out, d_out, (2 * (size_t)n - 1) * sizeof(rtbvh_node), hipMemcpyDeviceToHost));
    return RTBVH_OK;
}

}  // extern "C"

// ---- queries: the frame every kind shares ------------------------------------------------------------
// The chain's rules stand at QueryChain.  A rtbvh_<kind>_async entry is: its rules (a *_rules call: the same for
// its _host entry), enter_chain, the kind's words zeroed, fill_tree and the Args fields of its own,
// [walk_order], its launches ([two_passes] for lists), leave_chain.  The walks read the tree form the last build
// wrote (Tree::wrote NBOX: the topology and node boxes, else the node records), never a derived one.
namespace {

// What is wrong with a query call, in the order every kind keeps.  Ahead of this the kind has looked at its mode
// bits, then at its own scalars (k; the region split field).  Then: 2^31 queries or more; no queries -- nothing
// to do, *run stays false, whatever the pointers and the tree; a NULL array (null_msg: the kind's words for it);
// no tree; a tree that is not of the geometry.
rtbvh_status query_rules(rtbvh_ctx* c, const char* kind, const char* nouns, uint64_t n, const char* null_msg,
                         bool* run) {
    *run = false;
    if (n >= (1ull << 31))
        return fail(c, RTBVH_ERR_INVALID_ARG, std::string(kind) + ": 2^31 " + nouns + " or more");
    if (n == 0) return RTBVH_OK;
    if (null_msg) return fail(c, RTBVH_ERR_INVALID_ARG, null_msg);
    if (!c->tree.built) return fail(c, RTBVH_ERR_NOT_READY, std::string(kind) + " before build");
    if (c->stale) return fail_stale(c, kind);
    *run = true;
    return RTBVH_OK;
}

// The kinds that answer one record (or k) a query
struct RecordKind {
    const char *name, *nouns, *bad_mode, *nulls;
    uint32_t modes;
};
constexpr RecordKind QUERY{"query", "rays", "query: unknown mode bits", "query: NULL rays or hits",
                           RTBVH_QUERY_ANY | RTBVH_QUERY_SORT | RTBVH_QUERY_COUNT | RTBVH_QUERY_CERTIFIED};
constexpr RecordKind NEAREST{"nearest", "points", "nearest: unknown mode bits", "nearest: NULL points or results",
                             RTBVH_NEAREST_SORT | RTBVH_NEAREST_COUNT};
constexpr RecordKind KNN{"knn", "points", "knn: unknown mode bits", "knn: NULL points or pairs",
                         RTBVH_KNN_SORT | RTBVH_KNN_COUNT};
constexpr RecordKind KHITS{"khits", "rays", "khits: unknown mode bits", "khits: NULL rays or hits",
                           RTBVH_KHITS_SORT | RTBVH_KHITS_COUNT};
constexpr RecordKind SWEEP{"sweep", "sweeps", "sweep: unknown mode bits", "sweep: NULL sweeps or hits",
                           RTBVH_SWEEP_ANY | RTBVH_SWEEP_SORT | RTBVH_SWEEP_COUNT};
constexpr RecordKind SIGNED{"signed", "points", "signed: unknown mode bits", "signed: NULL points or results",
                            RTBVH_SIGNED_SORT | RTBVH_SIGNED_COUNT | RTBVH_SIGNED_VOTE3 | RTBVH_SIGNED_INSIDE_ONLY};
constexpr RecordKind CROSS_FIRST{"cross_first", "triangles", "cross_first: bad mode bits",
                                 "cross_first: NULL triangles or output", RTBVH_CROSS_SORT | RTBVH_CROSS_COUNT};
constexpr RecordKind CLEARANCE{"clearance", "triangles", "clearance: bad mode bits",
                               "clearance: NULL triangles or results", RTBVH_CLEARANCE_SORT | RTBVH_CLEARANCE_COUNT};
// bad_scalar: what is wrong with the kind's own scalar (k), or null
rtbvh_status record_rules(rtbvh_ctx* c, const RecordKind& k, uint32_t mode, const char* bad_scalar, const void* in,
                          uint64_t n, const void* out, bool* run) {
    if (mode & ~k.modes) return fail(c, RTBVH_ERR_INVALID_ARG, k.bad_mode);
    if (bad_scalar) return fail(c, RTBVH_ERR_INVALID_ARG, bad_scalar);
    return query_rules(c, k.name, k.nouns, n, !in || !out ? k.nulls : nullptr, run);
}

// The kinds that answer offsets and lists (CSR): one call, or a SIZES call and a FILL call
struct ListKind {
    const char *name, *nouns, *items;
    uint32_t modes, sizes, fill;   // every mode bit; the two of which a call takes one at the most
    bool own_queries = false;      // the tree's triangles are the queries: no array and no n of the caller's
};
constexpr ListKind WITHIN{"within", "points", "pairs",
                          RTBVH_WITHIN_SORT | RTBVH_WITHIN_COUNT | RTBVH_WITHIN_SIZES | RTBVH_WITHIN_FILL,
                          RTBVH_WITHIN_SIZES, RTBVH_WITHIN_FILL};
constexpr ListKind ALLHITS{"allhits", "rays", "hits",
                           RTBVH_ALLHITS_SORT | RTBVH_ALLHITS_COUNT | RTBVH_ALLHITS_BY_T | RTBVH_ALLHITS_SIZES |
                               RTBVH_ALLHITS_FILL,
                           RTBVH_ALLHITS_SIZES, RTBVH_ALLHITS_FILL};
constexpr ListKind OVERLAP{"overlap", "boxes", "ids",
                           RTBVH_OVERLAP_SORT | RTBVH_OVERLAP_COUNT | RTBVH_OVERLAP_TRIANGLE | RTBVH_OVERLAP_SIZES |
                               RTBVH_OVERLAP_FILL,
                           RTBVH_OVERLAP_SIZES, RTBVH_OVERLAP_FILL};
constexpr ListKind CROSS{"cross", "triangles", "ids",
                         RTBVH_CROSS_SORT | RTBVH_CROSS_COUNT | RTBVH_CROSS_SIZES | RTBVH_CROSS_FILL, RTBVH_CROSS_SIZES,
                         RTBVH_CROSS_FILL};
constexpr ListKind REGION{"region", "regions", "ids",
                          RTBVH_REGION_COUNT | RTBVH_REGION_TRIANGLE | RTBVH_REGION_SIZES | RTBVH_REGION_FILL |
                              RTBVH_REGION_NO_ACCEPT | RTBVH_REGION_SPLIT_AUTO,
                          RTBVH_REGION_SIZES, RTBVH_REGION_FILL};
constexpr ListKind COLLIDE{"collide", "", "ids",
                           RTBVH_COLLIDE_COUNT | RTBVH_COLLIDE_TRIANGLE | RTBVH_COLLIDE_SIZES | RTBVH_COLLIDE_FILL |
                               RTBVH_COLLIDE_SYMMETRIC,
                           RTBVH_COLLIDE_SIZES, RTBVH_COLLIDE_FILL, true};
// bad_scalar: as record_rules'.  A kind with own_queries has neither `in` nor `n` to check: what is left of the
// order is mode, NULL offsets, NULL items, the tree.
rtbvh_status list_rules(rtbvh_ctx* c, const ListKind& k, uint32_t mode, const char* bad_scalar, const void* in,
                        uint64_t n, const void* offsets, const void* items, uint64_t capacity, bool* run) {
    const std::string name = k.name;
    if ((mode & ~k.modes) || (mode & k.sizes && mode & k.fill))
        return fail(c, RTBVH_ERR_INVALID_ARG, name + ": bad mode bits");
    if (bad_scalar) return fail(c, RTBVH_ERR_INVALID_ARG, bad_scalar);
    const bool own = k.own_queries;
    std::string nulls;
    if (own ? !offsets : !in || !offsets)
        nulls = own ? name + ": NULL offsets" : name + ": NULL " + k.nouns + " or offsets";
    else if (!(mode & k.sizes) && capacity > 0 && !items) nulls = name + ": NULL " + k.items;
    // (own queries: any count that passes the rules on n)
    return query_rules(c, k.name, k.nouns, own ? 1 : n, nulls.empty() ? nullptr : nulls.c_str(), run);
}
// ... whose call without queries stores offsets[0] = 0, unless the offsets are input
rtbvh_status store_no_lists(rtbvh_ctx* c, uint64_t* dev_offsets, bool fill_only, void* stream) {
    if (!dev_offsets || fill_only) return RTBVH_OK;
    HIPC(c, hipSetDevice(c->cfg.device));
    HIPC(c, hipMemsetAsync(dev_offsets, 0, sizeof(uint64_t), stream ? (hipStream_t)stream : c->stream));
    return RTBVH_OK;
}

// What a link needs of the buffers grown on demand: counts of queries, 0 for none
struct Need {
    uint32_t sort = 0;     // a walk order over this many ([keys + sort])
    uint32_t scan = 0;     // an offset scan over this many
    uint32_t redo = 0;     // a certified ray query's re-trace list
    uint32_t order = 0;    // RTBVH_ALLHITS_BY_T over this many rays
    uint32_t pieces = 0;   // a split region query's piece slots
};
// The growth rule: the first link that needs a buffer and each larger one wait on the host for the links before
// them, which use the old buffers (and hipMalloc blocks too), as include/rtbvh.h says
rtbvh_status reserve_shared(rtbvh_ctx* c, const Need& n) {
    QueryChain& q = c->q;
    const size_t sort = n.sort ? 6 * (size_t)n.sort : 0, digits = n.sort ? sort_scratch_words(n.sort) : 0;
    const size_t scan = scan_sums_words(n.scan), order = 2 * (size_t)n.order;
    const size_t poff = n.pieces ? (size_t)n.pieces + 1 : 0, pscan = scan_sums_words(n.pieces);
    if (q.sort.has(sort) && q.sort_scratch.has(digits) && q.scan.has(scan) && q.redo.has(n.redo) && q.order.has(order) &&
        q.pieces.has(n.pieces) && q.poff.has(poff) && q.pscan.has(pscan))
        return RTBVH_OK;
    HIPC(c, hipEventSynchronize(q.ev));
    HIPC(c, q.sort.reserve(sort));
    HIPC(c, q.sort_scratch.reserve(digits));
    HIPC(c, q.scan.reserve(scan));
    HIPC(c, q.redo.reserve(n.redo));
    HIPC(c, q.order.reserve(order));
    HIPC(c, q.pieces.reserve(n.pieces));
    HIPC(c, q.poff.reserve(poff));
    HIPC(c, q.pscan.reserve(pscan));
    return RTBVH_OK;
}

// A link enters the chain on *s, the caller's stream or the context's: the shared buffers, then the waits for the
// last build and for the link before.  `derive`: a tree form to derive between the two (the QNodes of a build
// that wrote none, once: behind the earlier links, none of which reads them).
rtbvh_status enter_chain(rtbvh_ctx* c, void* stream, const Need& need, hipStream_t* s, uint32_t derive = 0) {
    QueryChain& q = c->q;
    HIPC(c, hipSetDevice(c->cfg.device));
    *s = stream ? (hipStream_t)stream : c->stream;
    if (!q.scratch) HIPC(c, q.scratch.alloc(QUERY_ALLOC_WORDS));
    if (!q.ev) HIPC(c, hipEventCreateWithFlags(q.ev.out(), hipEventDisableTiming));
    TRY(reserve_shared(c, need));
    if (*s != c->stream) HIPC(c, hipStreamWaitEvent(*s, c->ev_built, 0));
    if (derive) TRY(ensure_form(c, (Form)derive, *s));
    if (q.busy) HIPC(c, hipStreamWaitEvent(*s, q.ev, 0));
    return RTBVH_OK;
}
// ... and leaves it: the next link waits for what was enqueued up to here
rtbvh_status leave_chain(rtbvh_ctx* c, Kind k, bool count, const char* what, hipStream_t s) {
    const rtbvh_status st = check_launch(c, what);
    HIPC(c, hipEventRecord(c->q.ev, s));
    c->q.busy = true;
    c->q.ovf = true;
    if (count && !st) c->q.counted[k] = true;
    return st;
}

// Every walk launch needs the work counters zeroed again
rtbvh_status zero_work(rtbvh_ctx* c, hipStream_t s) {
    HIPC(c, hipMemsetAsync(c->q.scratch, 0, sizeof(uint32_t) * QUERY_COUNTS_AT, s));
    return RTBVH_OK;
}
// A counting link zeroes its kind's block (a link that does not count leaves the last counting one's words alone)
rtbvh_status zero_counts(rtbvh_ctx* c, Kind k, bool count, hipStream_t s) {
    if (count) HIPC(c, hipMemsetAsync(c->q.scratch + KINDS[k].at, 0, sizeof(uint64_t) * KINDS[k].words, s));
    return RTBVH_OK;
}

// The fields every kind's Args has: the tree, the work counters, a count block, the stack
template <typename Args>
void fill_tree(const rtbvh_ctx* c, Args& a, uint32_t counts_at) {
    a.inner = c->d_rec;
    a.topo = c->d_topo;
    a.nbox = c->d_nbox;
    a.nb = c->tree.wrote == NBOX;
    a.leaf = c->d_leaf;
    a.T = c->T;
    a.next = c->q.scratch;
    a.counts = reinterpret_cast<unsigned long long*>(c->q.scratch + counts_at);
    a.overflow = c->d_ovf;
    const uint32_t lim = c->cfg.stack_limit;
    a.stack_limit = lim && lim < (uint32_t)STACK_SIZE ? (int)lim : STACK_SIZE;
}

// [keys + sort]: the walk order of N queries by their kind's 30-bit keys, one permutation for every pass of the call
using KeysFn = void (*)(const float4*, uint32_t, const float*, uint32_t*, uint32_t*, hipStream_t);
const uint32_t* walk_order(rtbvh_ctx* c, KeysFn keys, const float4* queries, uint32_t N, hipStream_t s) {
    uint32_t* q = c->q.sort;
    const size_t m = c->q.sort.cap / 6;
    keys(queries, N, c->d_rootbox, q, q + m, s);
    return radix_sort_pairs(q, q + m, q + 2 * m, q + 3 * m, q + 4 * m, q + 5 * m, N, 30, c->q.sort_scratch, s).vals;
}

// [sizes + scan], then [fill]: pass(fill, count_items) sets the Args field that says whether the pass counts its
// items -- the sizes pass does; the fill pass of a FILL call does -- and launches
template <typename Pass>
rtbvh_status two_passes(rtbvh_ctx* c, bool sizes, bool fill, unsigned long long* offsets, uint32_t N, hipStream_t s,
                        Pass pass) {
    if (sizes) {
        TRY(zero_work(c, s));
        pass(false, true);
        scan_offsets(offsets, N, c->q.scan, s);
    }
    if (fill) {
        TRY(zero_work(c, s));
        pass(true, !sizes);
    }
    return RTBVH_OK;
}

// A host entry of a record kind: the inputs and behind them the outputs in one allocation (an input record is a
// multiple of 16 bytes), call(inputs, outputs) -- the kind's async entry on the context stream -- and the records
// back.  They are complete (knn, khits: the best found) when rtbvh_synchronize reports RTBVH_ERR_STACK_OVERFLOW.
template <typename Call>
rtbvh_status host_records(rtbvh_ctx* c, const std::string& name, const void* in, size_t in_bytes, void* out,
                          size_t out_bytes, Call call) {
    HIPC(c, hipSetDevice(c->cfg.device));
    DevBuf<char> d;
    HIPC(c, d.alloc(in_bytes + out_bytes));
    if (hipMemcpy(d, in, in_bytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(c, RTBVH_ERR_HIP, name + "_host: upload failed");
    TRY(call(d.h, d.h + in_bytes));
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, RTBVH_ERR_HIP, name + "_host: sync");
    if (hipMemcpy(out, d + in_bytes, out_bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(c, RTBVH_ERR_HIP, name + "_host: download failed");
    return rtbvh_synchronize(c);
}
// A host entry of a list kind: n + 1 offsets and behind them the inputs (8- and 16-byte aligned), the items apart;
// call(inputs, offsets, items, capacity).  FILL takes the offsets up, every other call brings them back; SIZES has
// no items; min(offsets[n], capacity) items come back.
template <typename Call>
rtbvh_status host_lists(rtbvh_ctx* c, const ListKind& k, uint32_t mode, const void* in, size_t in_bytes, uint64_t n,
                        uint64_t* offsets, void* items, size_t item_bytes, uint64_t capacity, Call call) {
    const std::string name = k.name;
    const bool fill_only = (mode & k.fill) != 0;
    HIPC(c, hipSetDevice(c->cfg.device));
    const size_t off_bytes = (size_t)(n + 1) * sizeof(uint64_t), in_at = (off_bytes + 15) & ~(size_t)15;
    DevBuf<char> d, ditems;
    HIPC(c, d.alloc(in_at + in_bytes));
    uint64_t* doff = reinterpret_cast<uint64_t*>(d.h);
    if (in_bytes && hipMemcpy(d + in_at, in, in_bytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(c, RTBVH_ERR_HIP, name + "_host: upload failed");
    if (fill_only && hipMemcpy(doff, offsets, off_bytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(c, RTBVH_ERR_HIP, name + "_host: upload failed");
    if (mode & k.sizes) capacity = 0;
    if (capacity) HIPC(c, ditems.alloc((size_t)capacity * item_bytes));
    if (capacity && fill_only)   // (offsets of another tree, mode or input leave gaps: zeros, not what the allocation held)
        HIPC(c, hipMemsetAsync(ditems, 0, (size_t)capacity * item_bytes, c->stream));
    TRY(call(d.h + in_at, doff, ditems.h, capacity));
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, RTBVH_ERR_HIP, name + "_host: sync");
    if (!fill_only && hipMemcpy(offsets, doff, off_bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(c, RTBVH_ERR_HIP, name + "_host: download failed");
    const uint64_t m = offsets[n] < capacity ? offsets[n] : capacity;
    if (m && hipMemcpy(items, ditems, (size_t)m * item_bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(c, RTBVH_ERR_HIP, name + "_host: download failed");
    return rtbvh_synchronize(c);   // (the results are complete when it reports RTBVH_ERR_STACK_OVERFLOW)
}

// A *_counts reader: `words` of the scratch block at `at`, behind the chain
rtbvh_status read_counts(rtbvh_ctx* c, Kind k, uint64_t* out, uint32_t at, uint32_t words) {
    if (!c || !out) return RTBVH_ERR_INVALID_ARG;
    if (!c->q.counted[k]) return fail(c, RTBVH_ERR_NOT_READY, KINDS[k].not_ready);
    HIPC(c, hipSetDevice(c->cfg.device));
    HIPC(c, hipEventSynchronize(c->q.ev));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "count block words");
    HIPC(c, hipMemcpy(out, c->q.scratch + at, sizeof(uint64_t) * words, hipMemcpyDeviceToHost));
    return RTBVH_OK;
}
rtbvh_status kind_counts(rtbvh_ctx* c, Kind k, uint64_t* out) { return read_counts(c, k, out, KINDS[k].at, KINDS[k].words); }

}  // namespace

extern "C" {

// ---- ray queries -------------------------------------------------------------------------------------
rtbvh_status rtbvh_query_async(rtbvh_ctx* c, const rtbvh_ray* dev_rays, uint64_t n, rtbvh_hit* dev_hits,
                               uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, QUERY, mode, nullptr, dev_rays, n, dev_hits, &run));
    if (!run) return RTBVH_OK;
    static_assert(sizeof(rtbvh_ray) == 32 && sizeof(rtbvh_hit) == 16, "query record layouts");
    const bool any = (mode & RTBVH_QUERY_ANY) != 0, sort = (mode & RTBVH_QUERY_SORT) != 0;
    const bool count = (mode & RTBVH_QUERY_COUNT) != 0;
    const uint32_t N = (uint32_t)n;
    // RTBVH_QUERY_CERTIFIED: the certified 4-wide walk under a certified trace's conditions (plan_trace: a clz64
    // tree, the full stack); otherwise the present kernel for every ray -- the same hits either way
    const bool limited = c->cfg.stack_limit != 0 && c->cfg.stack_limit < (uint32_t)STACK_SIZE;
    const bool cert = (mode & RTBVH_QUERY_CERTIFIED) != 0 && c->tree.clz64 && !limited;
    Need need;
    need.sort = sort ? N : 0;
    need.redo = cert ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s, cert ? QNODES : 0));
    uint32_t* scratch = c->q.scratch;
    // the work counters; behind them a counting query's count block and walk counts, a certified query's list
    // length and its re-trace's work counters
    HIPC(c, hipMemsetAsync(scratch, 0, sizeof(uint32_t) * (count ? QUERY_REDO_N_AT : QUERY_COUNTS_AT), s));
    if (cert)
        HIPC(c, hipMemsetAsync(scratch + QUERY_REDO_N_AT, 0, sizeof(uint32_t) * (QUERY_SCRATCH_WORDS - QUERY_REDO_N_AT), s));
    QueryArgs a{};
    fill_tree(c, a, QUERY_COUNTS_AT);
    a.rays = reinterpret_cast<const float4*>(dev_rays);
    a.hits = reinterpret_cast<float4*>(dev_hits);
    a.n = N;
    a.walk = reinterpret_cast<unsigned long long*>(scratch + QUERY_WALK_AT);
    a.qnode = c->d_qnode;
    a.tclip = c->d_tclip;
    a.redo = c->q.redo;
    a.redo_n = scratch + QUERY_REDO_N_AT;
    a.next2 = scratch + QUERY_NEXT2_AT;
    if (sort) a.perm = walk_order(c, launch_query_keys, a.rays, N, s);
    if (cert) launch_query_certified(a, any, count, s);
    else launch_query(a, any, count, s);
    const rtbvh_status st = leave_chain(c, K_QUERY, count, "query kernels", s);
    if (count && !st) c->q.fallback = cert ? 0 : n;
    return st;
}

rtbvh_status rtbvh_query_host(rtbvh_ctx* c, const rtbvh_ray* rays, uint64_t n, rtbvh_hit* hits, uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, QUERY, mode, nullptr, rays, n, hits, &run));
    if (!run) return RTBVH_OK;
    return host_records(c, QUERY.name, rays, (size_t)n * sizeof(rtbvh_ray), hits, (size_t)n * sizeof(rtbvh_hit),
                        [&](char* in, char* out) {
                            return rtbvh_query_async(c, reinterpret_cast<const rtbvh_ray*>(in), n,
                                                     reinterpret_cast<rtbvh_hit*>(out), mode, nullptr);
                        });
}

rtbvh_status rtbvh_query_counts(rtbvh_ctx* c, uint64_t out[4]) { return kind_counts(c, K_QUERY, out); }

rtbvh_status rtbvh_query_walk_counts(rtbvh_ctx* c, uint64_t out[4]) {
    // certified, redone, uncovered from the walk; a query that took the present kernel wrote none (zeroed)
    TRY(read_counts(c, K_QUERY, out, QUERY_WALK_AT, 3));
    out[3] = c->q.fallback;
    return RTBVH_OK;
}

// ---- closest-point queries ---------------------------------------------------------------------------
// Never the quantized nodes, whose boxes are grown.
rtbvh_status rtbvh_nearest_async(rtbvh_ctx* c, const rtbvh_point* dev_points, uint64_t n, rtbvh_nearest* dev_out,
                                 uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, NEAREST, mode, nullptr, dev_points, n, dev_out, &run));
    if (!run) return RTBVH_OK;
    static_assert(sizeof(rtbvh_point) == 16 && sizeof(rtbvh_nearest) == 32, "closest-point record layouts");
    const bool sort = (mode & RTBVH_NEAREST_SORT) != 0, count = (mode & RTBVH_NEAREST_COUNT) != 0;
    const uint32_t N = (uint32_t)n;
    Need need;
    need.sort = sort ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    TRY(zero_work(c, s));
    TRY(zero_counts(c, K_NEAREST, count, s));
    NearestArgs a{};
    fill_tree(c, a, QUERY_NEAREST_AT);
    a.points = reinterpret_cast<const float4*>(dev_points);
    a.out = reinterpret_cast<float4*>(dev_out);
    a.n = N;
    if (sort) a.perm = walk_order(c, launch_nearest_keys, a.points, N, s);
    launch_nearest(a, count, s);
    return leave_chain(c, K_NEAREST, count, "nearest kernels", s);
}

rtbvh_status rtbvh_nearest_host(rtbvh_ctx* c, const rtbvh_point* points, uint64_t n, rtbvh_nearest* out, uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, NEAREST, mode, nullptr, points, n, out, &run));
    if (!run) return RTBVH_OK;
    return host_records(c, NEAREST.name, points, (size_t)n * sizeof(rtbvh_point), out, (size_t)n * sizeof(rtbvh_nearest),
                        [&](char* in, char* res) {
                            return rtbvh_nearest_async(c, reinterpret_cast<const rtbvh_point*>(in), n,
                                                       reinterpret_cast<rtbvh_nearest*>(res), mode, nullptr);
                        });
}

rtbvh_status rtbvh_nearest_counts(rtbvh_ctx* c, uint64_t out[4]) { return kind_counts(c, K_NEAREST, out); }

// ---- radius queries ------------------------------------------------------------------------------------
rtbvh_status rtbvh_within_async(rtbvh_ctx* c, const rtbvh_point* dev_points, uint64_t n, uint64_t* dev_offsets,
                                rtbvh_pair* dev_pairs, uint64_t capacity, uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(list_rules(c, WITHIN, mode, nullptr, dev_points, n, dev_offsets, dev_pairs, capacity, &run));
    const bool sizes = !(mode & RTBVH_WITHIN_FILL), fill = !(mode & RTBVH_WITHIN_SIZES);
    if (!run) return store_no_lists(c, dev_offsets, !sizes, stream);
    static_assert(sizeof(rtbvh_pair) == 8 && sizeof(uint64_t) == sizeof(unsigned long long), "radius query layouts");
    const bool sort = (mode & RTBVH_WITHIN_SORT) != 0, count = (mode & RTBVH_WITHIN_COUNT) != 0;
    const uint32_t N = (uint32_t)n;
    Need need;
    need.sort = sort ? N : 0;
    need.scan = sizes ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    TRY(zero_counts(c, K_WITHIN, count, s));
    WithinArgs a{};
    fill_tree(c, a, QUERY_WITHIN_AT);
    a.points = reinterpret_cast<const float4*>(dev_points);
    a.offsets = reinterpret_cast<unsigned long long*>(dev_offsets);
    a.pairs = reinterpret_cast<uint2*>(dev_pairs);
    a.capacity = capacity;
    a.n = N;
    if (sort) a.perm = walk_order(c, launch_nearest_keys, a.points, N, s);
    TRY(two_passes(c, sizes, fill, a.offsets, N, s, [&](bool fill_pass, bool count_items) {
        a.count_pairs = count_items;
        launch_within(a, fill_pass, count, s);
    }));
    return leave_chain(c, K_WITHIN, count, "within kernels", s);
}

rtbvh_status rtbvh_within_host(rtbvh_ctx* c, const rtbvh_point* points, uint64_t n, uint64_t* offsets,
                               rtbvh_pair* pairs, uint64_t capacity, uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(list_rules(c, WITHIN, mode, nullptr, points, n, offsets, pairs, capacity, &run));
    if (!run) {   // (nothing to stage)
        if (offsets && !(mode & RTBVH_WITHIN_FILL)) offsets[0] = 0;
        return RTBVH_OK;
    }
    return host_lists(c, WITHIN, mode, points, (size_t)n * sizeof(rtbvh_point), n, offsets, pairs, sizeof(rtbvh_pair),
                      capacity, [&](char* in, uint64_t* off, char* items, uint64_t cap) {
                          return rtbvh_within_async(c, reinterpret_cast<const rtbvh_point*>(in), n, off,
                                                    reinterpret_cast<rtbvh_pair*>(items), cap, mode, nullptr);
                      });
}

rtbvh_status rtbvh_within_counts(rtbvh_ctx* c, uint64_t out[4]) { return kind_counts(c, K_WITHIN, out); }

// ---- all-hits ray queries --------------------------------------------------------------------------------
// The two passes, then for RTBVH_ALLHITS_BY_T the ordering pass, which takes the work counters' first word (the
// walks are over) for the length of its list.
rtbvh_status rtbvh_allhits_async(rtbvh_ctx* c, const rtbvh_ray* dev_rays, uint64_t n, uint64_t* dev_offsets,
                                 rtbvh_hit* dev_hits, uint64_t capacity, uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    constexpr uint32_t SIZES_BY_T = RTBVH_ALLHITS_SIZES | RTBVH_ALLHITS_BY_T;   // (nothing stored: nothing to order)
    bool run;
    TRY(list_rules(c, ALLHITS, mode, (mode & SIZES_BY_T) == SIZES_BY_T ? "allhits: bad mode bits" : nullptr, dev_rays, n,
                   dev_offsets, dev_hits, capacity, &run));
    const bool sizes = !(mode & RTBVH_ALLHITS_FILL), fill = !(mode & RTBVH_ALLHITS_SIZES);
    if (!run) return store_no_lists(c, dev_offsets, !sizes, stream);
    const bool sort = (mode & RTBVH_ALLHITS_SORT) != 0, count = (mode & RTBVH_ALLHITS_COUNT) != 0;
    const bool by_t = (mode & RTBVH_ALLHITS_BY_T) != 0 && capacity > 0;   // (nothing stored: nothing to order)
    const uint32_t N = (uint32_t)n;
    Need need;
    need.sort = sort ? N : 0;
    need.scan = sizes ? N : 0;
    need.order = by_t ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    TRY(zero_counts(c, K_ALLHITS, count, s));
    AllhitsArgs a{};
    fill_tree(c, a, QUERY_ALLHITS_AT);
    a.rays = reinterpret_cast<const float4*>(dev_rays);
    a.offsets = reinterpret_cast<unsigned long long*>(dev_offsets);
    a.hits = reinterpret_cast<float4*>(dev_hits);
    a.capacity = capacity;
    a.n = N;
    if (sort) a.perm = walk_order(c, launch_query_keys, a.rays, N, s);
    uint32_t* ord = c->q.order;
    TRY(two_passes(c, sizes, fill, a.offsets, N, s, [&](bool fill_pass, bool count_items) {
        a.count_hits = count_items;
        if (fill_pass && by_t) a.written = ord;
        launch_allhits(a, fill_pass, count, s);
    }));
    if (fill && by_t) {
        HIPC(c, hipMemsetAsync(c->q.scratch, 0, sizeof(uint32_t), s));   // the list's length
        launch_allhits_order(a.hits, a.offsets, ord, N, ord + c->q.order.cap / 2, c->q.scratch, s);
    }
    return leave_chain(c, K_ALLHITS, count, "allhits kernels", s);
}

rtbvh_status rtbvh_allhits_host(rtbvh_ctx* c, const rtbvh_ray* rays, uint64_t n, uint64_t* offsets, rtbvh_hit* hits,
                                uint64_t capacity, uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    constexpr uint32_t SIZES_BY_T = RTBVH_ALLHITS_SIZES | RTBVH_ALLHITS_BY_T;
    bool run;
    TRY(list_rules(c, ALLHITS, mode, (mode & SIZES_BY_T) == SIZES_BY_T ? "allhits: bad mode bits" : nullptr, rays, n,
                   offsets, hits, capacity, &run));
    if (!run) {   // (nothing to stage)
        if (offsets && !(mode & RTBVH_ALLHITS_FILL)) offsets[0] = 0;
        return RTBVH_OK;
    }
    return host_lists(c, ALLHITS, mode, rays, (size_t)n * sizeof(rtbvh_ray), n, offsets, hits, sizeof(rtbvh_hit), capacity,
                      [&](char* in, uint64_t* off, char* items, uint64_t cap) {
                          return rtbvh_allhits_async(c, reinterpret_cast<const rtbvh_ray*>(in), n, off,
                                                     reinterpret_cast<rtbvh_hit*>(items), cap, mode, nullptr);
                      });
}

rtbvh_status rtbvh_allhits_counts(rtbvh_ctx* c, uint64_t out[4]) { return kind_counts(c, K_ALLHITS, out); }

// ---- box-overlap queries -------------------------------------------------------------------------------
rtbvh_status rtbvh_overlap_async(rtbvh_ctx* c, const rtbvh_box* dev_boxes, uint64_t n, uint64_t* dev_offsets,
                                 uint32_t* dev_ids, uint64_t capacity, uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(list_rules(c, OVERLAP, mode, nullptr, dev_boxes, n, dev_offsets, dev_ids, capacity, &run));
    const bool sizes = !(mode & RTBVH_OVERLAP_FILL), fill = !(mode & RTBVH_OVERLAP_SIZES);
    if (!run) return store_no_lists(c, dev_offsets, !sizes, stream);
    static_assert(sizeof(rtbvh_box) == 32 && sizeof(uint64_t) == sizeof(unsigned long long), "box query layouts");
    const bool sort = (mode & RTBVH_OVERLAP_SORT) != 0, count = (mode & RTBVH_OVERLAP_COUNT) != 0;
    const bool tri = (mode & RTBVH_OVERLAP_TRIANGLE) != 0;
    const uint32_t N = (uint32_t)n;
    Need need;
    need.sort = sort ? N : 0;
    need.scan = sizes ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    TRY(zero_counts(c, K_OVERLAP, count, s));
    OverlapArgs a{};
    fill_tree(c, a, QUERY_OVERLAP_AT);
    a.boxes = reinterpret_cast<const float4*>(dev_boxes);
    a.offsets = reinterpret_cast<unsigned long long*>(dev_offsets);
    a.ids = dev_ids;
    a.capacity = capacity;
    a.n = N;
    if (sort) a.perm = walk_order(c, launch_overlap_keys, a.boxes, N, s);
    TRY(two_passes(c, sizes, fill, a.offsets, N, s, [&](bool fill_pass, bool count_items) {
        a.count_ids = count_items;
        launch_overlap(a, fill_pass, count, tri, s);
    }));
    return leave_chain(c, K_OVERLAP, count, "overlap kernels", s);
}

rtbvh_status rtbvh_overlap_host(rtbvh_ctx* c, const rtbvh_box* boxes, uint64_t n, uint64_t* offsets, uint32_t* ids,
                                uint64_t capacity, uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(list_rules(c, OVERLAP, mode, nullptr, boxes, n, offsets, ids, capacity, &run));
    if (!run) {   // (nothing to stage)
        if (offsets && !(mode & RTBVH_OVERLAP_FILL)) offsets[0] = 0;
        return RTBVH_OK;
    }
    return host_lists(c, OVERLAP, mode, boxes, (size_t)n * sizeof(rtbvh_box), n, offsets, ids, sizeof(uint32_t), capacity,
                      [&](char* in, uint64_t* off, char* items, uint64_t cap) {
                          return rtbvh_overlap_async(c, reinterpret_cast<const rtbvh_box*>(in), n, off,
                                                     reinterpret_cast<uint32_t*>(items), cap, mode, nullptr);
                      });
}

rtbvh_status rtbvh_overlap_counts(rtbvh_ctx* c, uint64_t out[4]) { return kind_counts(c, K_OVERLAP, out); }

// ---- self-collision queries ----------------------------------------------------------------------------
// The tree's T leaves are the queries: no walk order.
rtbvh_status rtbvh_collide_async(rtbvh_ctx* c, uint64_t* dev_offsets, uint32_t* dev_ids, uint64_t capacity,
                                 uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(list_rules(c, COLLIDE, mode, nullptr, nullptr, 0, dev_offsets, dev_ids, capacity, &run));
    const bool sizes = !(mode & RTBVH_COLLIDE_FILL), fill = !(mode & RTBVH_COLLIDE_SIZES);
    const bool count = (mode & RTBVH_COLLIDE_COUNT) != 0, tri = (mode & RTBVH_COLLIDE_TRIANGLE) != 0;
    const bool sym = (mode & RTBVH_COLLIDE_SYMMETRIC) != 0;
    const uint32_t N = c->T;
    Need need;
    need.scan = sizes ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    TRY(zero_counts(c, K_COLLIDE, count, s));
    CollideArgs a{};
    fill_tree(c, a, QUERY_COLLIDE_AT);
    a.idx = c->d_idx;
    a.offsets = reinterpret_cast<unsigned long long*>(dev_offsets);
    a.ids = dev_ids;
    a.capacity = capacity;
    TRY(two_passes(c, sizes, fill, a.offsets, N, s, [&](bool fill_pass, bool count_items) {
        a.count_ids = count_items;
        launch_collide(a, fill_pass, count, tri, sym, s);
    }));
    return leave_chain(c, K_COLLIDE, count, "collide kernels", s);
}

rtbvh_status rtbvh_collide_host(rtbvh_ctx* c, uint64_t* offsets, uint32_t* ids, uint64_t capacity, uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(list_rules(c, COLLIDE, mode, nullptr, nullptr, 0, offsets, ids, capacity, &run));
    return host_lists(c, COLLIDE, mode, nullptr, 0, c->T, offsets, ids, sizeof(uint32_t), capacity,
                      [&](char*, uint64_t* off, char* items, uint64_t cap) {
                          return rtbvh_collide_async(c, off, reinterpret_cast<uint32_t*>(items), cap, mode, nullptr);
                      });
}

rtbvh_status rtbvh_collide_counts(rtbvh_ctx* c, uint64_t out[4]) { return kind_counts(c, K_COLLIDE, out); }

// ---- triangle queries ----------------------------------------------------------------------------------
// rtbvh_cross_first_async is [keys + sort] and one launch, with no scan; it shares the count block.
rtbvh_status rtbvh_cross_async(rtbvh_ctx* c, const rtbvh_tri* dev_tris, uint64_t n, uint64_t* dev_offsets,
                               uint32_t* dev_ids, uint64_t capacity, uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(list_rules(c, CROSS, mode, nullptr, dev_tris, n, dev_offsets, dev_ids, capacity, &run));
    const bool sizes = !(mode & RTBVH_CROSS_FILL), fill = !(mode & RTBVH_CROSS_SIZES);
    if (!run) return store_no_lists(c, dev_offsets, !sizes, stream);
    static_assert(sizeof(rtbvh_tri) == 48 && sizeof(uint64_t) == sizeof(unsigned long long), "triangle query layouts");
    const bool sort = (mode & RTBVH_CROSS_SORT) != 0, count = (mode & RTBVH_CROSS_COUNT) != 0;
    const uint32_t N = (uint32_t)n;
    Need need;
    need.sort = sort ? N : 0;
    need.scan = sizes ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    TRY(zero_counts(c, K_CROSS, count, s));
    CrossArgs a{};
    fill_tree(c, a, QUERY_CROSS_AT);
    a.tris = reinterpret_cast<const float4*>(dev_tris);
    a.n = N;
    a.offsets = reinterpret_cast<unsigned long long*>(dev_offsets);
    a.ids = dev_ids;
    a.capacity = capacity;
    if (sort) a.perm = walk_order(c, launch_cross_keys, a.tris, N, s);
    TRY(two_passes(c, sizes, fill, a.offsets, N, s, [&](bool fill_pass, bool count_items) {
        a.count_ids = count_items;
        launch_cross(a, fill_pass ? CROSS_PASS_FILL : CROSS_PASS_SIZES, count, s);
    }));
    return leave_chain(c, K_CROSS, count, "cross kernels", s);
}

rtbvh_status rtbvh_cross_host(rtbvh_ctx* c, const rtbvh_tri* tris, uint64_t n, uint64_t* offsets, uint32_t* ids,
                              uint64_t capacity, uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(list_rules(c, CROSS, mode, nullptr, tris, n, offsets, ids, capacity, &run));
    if (!run) {   // (nothing to stage)
        if (offsets && !(mode & RTBVH_CROSS_FILL)) offsets[0] = 0;
        return RTBVH_OK;
    }
    return host_lists(c, CROSS, mode, tris, (size_t)n * sizeof(rtbvh_tri), n, offsets, ids, sizeof(uint32_t), capacity,
                      [&](char* in, uint64_t* off, char* items, uint64_t cap) {
                          return rtbvh_cross_async(c, reinterpret_cast<const rtbvh_tri*>(in), n, off,
                                                   reinterpret_cast<uint32_t*>(items), cap, mode, nullptr);
                      });
}

rtbvh_status rtbvh_cross_first_async(rtbvh_ctx* c, const rtbvh_tri* dev_tris, uint64_t n, uint32_t* dev_first,
                                     uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, CROSS_FIRST, mode, nullptr, dev_tris, n, dev_first, &run));
    if (!run) return RTBVH_OK;
    const bool sort = (mode & RTBVH_CROSS_SORT) != 0, count = (mode & RTBVH_CROSS_COUNT) != 0;
    const uint32_t N = (uint32_t)n;
    Need need;
    need.sort = sort ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    TRY(zero_counts(c, K_CROSS, count, s));
    CrossArgs a{};
    fill_tree(c, a, QUERY_CROSS_AT);
    a.tris = reinterpret_cast<const float4*>(dev_tris);
    a.n = N;
    a.first = dev_first;
    a.count_ids = true;
    if (sort) a.perm = walk_order(c, launch_cross_keys, a.tris, N, s);
    TRY(zero_work(c, s));
    launch_cross(a, CROSS_PASS_FIRST, count, s);
    return leave_chain(c, K_CROSS, count, "cross_first kernel", s);
}

rtbvh_status rtbvh_cross_first_host(rtbvh_ctx* c, const rtbvh_tri* tris, uint64_t n, uint32_t* first, uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, CROSS_FIRST, mode, nullptr, tris, n, first, &run));
    if (!run) return RTBVH_OK;
    return host_records(c, CROSS_FIRST.name, tris, (size_t)n * sizeof(rtbvh_tri), first, (size_t)n * sizeof(uint32_t),
                        [&](char* in, char* out) {
                            return rtbvh_cross_first_async(c, reinterpret_cast<const rtbvh_tri*>(in), n,
                                                           reinterpret_cast<uint32_t*>(out), mode, nullptr);
                        });
}

rtbvh_status rtbvh_cross_counts(rtbvh_ctx* c, uint64_t out[4]) { return kind_counts(c, K_CROSS, out); }

// ---- clearance queries ---------------------------------------------------------------------------------
// The triangle queries' inputs and walk order, one launch, a count block of its own.
rtbvh_status rtbvh_clearance_async(rtbvh_ctx* c, const rtbvh_tri* dev_tris, uint64_t n, float max_dist2,
                                   rtbvh_clearance* dev_out, uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, CLEARANCE, mode, nullptr, dev_tris, n, dev_out, &run));
    if (!run) return RTBVH_OK;
    static_assert(sizeof(rtbvh_clearance) == 32, "clearance record layout");
    const bool sort = (mode & RTBVH_CLEARANCE_SORT) != 0, count = (mode & RTBVH_CLEARANCE_COUNT) != 0;
    const uint32_t N = (uint32_t)n;
    Need need;
    need.sort = sort ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    ClearanceArgs a{};
    fill_tree(c, a, QUERY_CLEARANCE_AT);
    a.tris = reinterpret_cast<const float4*>(dev_tris);
    a.max_dist2 = max_dist2;
    a.out = reinterpret_cast<float4*>(dev_out);
    a.n = N;
    if (sort) a.perm = walk_order(c, launch_cross_keys, a.tris, N, s);
    TRY(zero_work(c, s));
    TRY(zero_counts(c, K_CLEARANCE, count, s));
    launch_clearance(a, count, s);
    return leave_chain(c, K_CLEARANCE, count, "clearance kernel", s);
}

rtbvh_status rtbvh_clearance_host(rtbvh_ctx* c, const rtbvh_tri* tris, uint64_t n, float max_dist2, rtbvh_clearance* out,
                                  uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, CLEARANCE, mode, nullptr, tris, n, out, &run));
    if (!run) return RTBVH_OK;
    return host_records(c, CLEARANCE.name, tris, (size_t)n * sizeof(rtbvh_tri), out, (size_t)n * sizeof(rtbvh_clearance),
                        [&](char* in, char* res) {
                            return rtbvh_clearance_async(c, reinterpret_cast<const rtbvh_tri*>(in), n, max_dist2,
                                                         reinterpret_cast<rtbvh_clearance*>(res), mode, nullptr);
                        });
}

rtbvh_status rtbvh_clearance_counts(rtbvh_ctx* c, uint64_t out[4]) { return kind_counts(c, K_CLEARANCE, out); }

// ---- region queries --------------------------------------------------------------------------------------
// No walk order (a region has no centre): [the leaf-NaN word, once a tree], then the two passes -- or, split, the
// pieces' passes.
rtbvh_status rtbvh_region_async(rtbvh_ctx* c, const rtbvh_region* dev_regions, uint64_t n, uint64_t* dev_offsets,
                                uint32_t* dev_ids, uint64_t capacity, uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    const uint32_t field = (mode >> RTBVH_REGION_SPLIT_SHIFT) & 15u;
    bool run;
    TRY(list_rules(c, REGION, mode, field > REGION_SPLIT_MAX_SHIFT && field != 15u ? "region: split field 13 or 14" : nullptr,
                   dev_regions, n, dev_offsets, dev_ids, capacity, &run));
    const bool sizes = !(mode & RTBVH_REGION_FILL), fill = !(mode & RTBVH_REGION_SIZES);
    if (!run) return store_no_lists(c, dev_offsets, !sizes, stream);
    static_assert(sizeof(rtbvh_region) == 96, "region query layout");
    static_assert(REGION_SPLIT_MAX_PIECES == RTBVH_REGION_SPLIT_MAX_PIECES && REGION_SPLIT_MAX_SHIFT == 12,
                  "the split field's documented bounds");
    const bool count = (mode & RTBVH_REGION_COUNT) != 0, tri = (mode & RTBVH_REGION_TRIANGLE) != 0;
    const uint32_t N = (uint32_t)n;
    // The split field is an upper limit: K = 2^kshift pieces a region, the largest with n * K <= the product bound
    // (automatic: from 4096 down).  K = 1 is the plain path.
    uint32_t kshift = field == 15u ? REGION_SPLIT_MAX_SHIFT : field;
    while (kshift > 0 && ((uint64_t)N << kshift) > REGION_SPLIT_MAX_PIECES) kshift--;
    const uint32_t slots = N << kshift;
    QueryChain& q = c->q;
    Need need;
    need.scan = sizes ? N : 0;
    need.pieces = kshift ? slots : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    // (behind enter_chain's hipSetDevice: an event of the context's device)
    if (!q.ev_nan) HIPC(c, hipEventCreateWithFlags(q.ev_nan.out(), hipEventDisableTiming));
    uint32_t* nan_word = q.scratch + QUERY_LEAF_NAN_AT;
    if (q.nan_epoch != c->bins_epoch) {   // the first region query of this tree writes the word, behind the tree
        HIPC(c, hipMemsetAsync(nan_word, 0, sizeof(uint32_t), s));
        launch_leaf_nan(c->d_leaf, c->T, nan_word, s);
        HIPC(c, hipEventRecord(q.ev_nan, s));
        q.nan_epoch = c->bins_epoch;
    } else {
        HIPC(c, hipStreamWaitEvent(s, q.ev_nan, 0));   // (written on another stream, perhaps)
    }
    TRY(zero_counts(c, K_REGION, count, s));
    RegionArgs a{};
    fill_tree(c, a, QUERY_REGION_AT);
    a.rootbox = c->d_rootbox;
    a.regions = reinterpret_cast<const float4*>(dev_regions);
    a.offsets = reinterpret_cast<unsigned long long*>(dev_offsets);
    a.ids = dev_ids;
    a.capacity = capacity;
    a.n = N;
    a.accept = !(mode & RTBVH_REGION_NO_ACCEPT);
    a.leaf_nan = nan_word;
    const bool count_split = count && field != 0u;
    TRY(zero_counts(c, K_REGION_SPLIT, count_split, s));
    if (kshift) {
        // [expansion], [piece sizes + scan], then the caller's offsets (not RTBVH_REGION_FILL: those are input) and
        // [piece fill]: a launch sequence fixed by (n, K, mode), all on the caller's stream
        RegionSplitArgs sa{};
        sa.pieces = q.pieces;
        sa.poff = q.poff;
        sa.kshift = kshift;
        sa.split = reinterpret_cast<unsigned long long*>(q.scratch + QUERY_REGION_SPLIT_AT);
        sa.r = a;
        launch_region_expand(sa, count, s);
        TRY(zero_work(c, s));
        sa.r.count_ids = sizes;
        launch_region_piece(sa, false, count, tri, s);
        scan_offsets(sa.poff, slots, q.pscan, s);
        if (sizes) launch_region_offsets(sa.poff, a.offsets, N, kshift, s);
        if (fill) {
            TRY(zero_work(c, s));
            sa.r.count_ids = !sizes;
            launch_region_piece(sa, true, count, tri, s);
        }
    } else {
        TRY(two_passes(c, sizes, fill, a.offsets, N, s, [&](bool fill_pass, bool count_items) {
            a.count_ids = count_items;
            launch_region(a, fill_pass, count, tri, s);
        }));
    }
    const rtbvh_status st = leave_chain(c, K_REGION, count, "region kernels", s);
    if (count_split && !st) {
        q.counted[K_REGION_SPLIT] = true;
        q.split_k = 1ull << kshift;
    }
    return st;
}

rtbvh_status rtbvh_region_host(rtbvh_ctx* c, const rtbvh_region* regions, uint64_t n, uint64_t* offsets, uint32_t* ids,
                               uint64_t capacity, uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    const uint32_t field = (mode >> RTBVH_REGION_SPLIT_SHIFT) & 15u;
    bool run;
    TRY(list_rules(c, REGION, mode, field > REGION_SPLIT_MAX_SHIFT && field != 15u ? "region: split field 13 or 14" : nullptr,
                   regions, n, offsets, ids, capacity, &run));
    if (!run) {   // (nothing to stage)
        if (offsets && !(mode & RTBVH_REGION_FILL)) offsets[0] = 0;
        return RTBVH_OK;
    }
    return host_lists(c, REGION, mode, regions, (size_t)n * sizeof(rtbvh_region), n, offsets, ids, sizeof(uint32_t),
                      capacity, [&](char* in, uint64_t* off, char* items, uint64_t cap) {
                          return rtbvh_region_async(c, reinterpret_cast<const rtbvh_region*>(in), n, off,
                                                    reinterpret_cast<uint32_t*>(items), cap, mode, nullptr);
                      });
}

rtbvh_status rtbvh_region_counts(rtbvh_ctx* c, uint64_t out[6]) { return kind_counts(c, K_REGION, out); }

rtbvh_status rtbvh_region_split_counts(rtbvh_ctx* c, uint64_t out[4]) {
    if (!out) return RTBVH_ERR_INVALID_ARG;
    TRY(kind_counts(c, K_REGION_SPLIT, out + 1));
    out[0] = c->q.split_k;
    return RTBVH_OK;
}

// ---- k-nearest queries ---------------------------------------------------------------------------------
// One walk, no second pass.
rtbvh_status rtbvh_knn_async(rtbvh_ctx* c, const rtbvh_point* dev_points, uint64_t n, uint32_t k, rtbvh_pair* dev_pairs,
                             uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, KNN, mode, k == 0 || k > RTBVH_KNN_MAX_K ? "knn: k must be 1 .. RTBVH_KNN_MAX_K" : nullptr,
                     dev_points, n, dev_pairs, &run));
    if (!run) return RTBVH_OK;
    static_assert(sizeof(rtbvh_point) == 16 && sizeof(rtbvh_pair) == 8, "k-nearest record layouts");
    static_assert(RTBVH_KNN_MAX_K == KNN_MAX_K, "the largest list of k_knn");
    const bool sort = (mode & RTBVH_KNN_SORT) != 0, count = (mode & RTBVH_KNN_COUNT) != 0;
    const uint32_t N = (uint32_t)n;
    Need need;
    need.sort = sort ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    TRY(zero_work(c, s));
    TRY(zero_counts(c, K_KNN, count, s));
    KnnArgs a{};
    fill_tree(c, a, QUERY_KNN_AT);
    a.points = reinterpret_cast<const float4*>(dev_points);
    a.pairs = reinterpret_cast<uint2*>(dev_pairs);
    a.n = N;
    a.k = k;
    if (sort) a.perm = walk_order(c, launch_nearest_keys, a.points, N, s);
    launch_knn(a, count, s);
    return leave_chain(c, K_KNN, count, "knn kernels", s);
}

rtbvh_status rtbvh_knn_host(rtbvh_ctx* c, const rtbvh_point* points, uint64_t n, uint32_t k, rtbvh_pair* pairs,
                            uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, KNN, mode, k == 0 || k > RTBVH_KNN_MAX_K ? "knn: k must be 1 .. RTBVH_KNN_MAX_K" : nullptr, points,
                     n, pairs, &run));
    if (!run) return RTBVH_OK;
    return host_records(c, KNN.name, points, (size_t)n * sizeof(rtbvh_point), pairs, (size_t)n * k * sizeof(rtbvh_pair),
                        [&](char* in, char* out) {
                            return rtbvh_knn_async(c, reinterpret_cast<const rtbvh_point*>(in), n, k,
                                                   reinterpret_cast<rtbvh_pair*>(out), mode, nullptr);
                        });
}

rtbvh_status rtbvh_knn_counts(rtbvh_ctx* c, uint64_t out[4]) { return kind_counts(c, K_KNN, out); }

// ---- signed-distance queries ---------------------------------------------------------------------------
// One link: the closest-point pass (k_nearest, unless RTBVH_SIGNED_INSIDE_ONLY) and the ray pass (k_signed) over the
// same walk order, on the same stream.  Its count blocks are QUERY_SIGNED_AT (the ray pass) and
// QUERY_SIGNED_NEAR_AT (the closest-point pass), zeroed together (INSIDE_ONLY: the second stays zero).
rtbvh_status rtbvh_signed_async(rtbvh_ctx* c, const rtbvh_point* dev_points, uint64_t n, rtbvh_signed* dev_out,
                                uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, SIGNED, mode, nullptr, dev_points, n, dev_out, &run));
    if (!run) return RTBVH_OK;
    static_assert(sizeof(rtbvh_point) == 16 && sizeof(rtbvh_signed) == 32, "signed-distance record layouts");
    const bool sort = (mode & RTBVH_SIGNED_SORT) != 0, count = (mode & RTBVH_SIGNED_COUNT) != 0;
    const bool vote3 = (mode & RTBVH_SIGNED_VOTE3) != 0, near = !(mode & RTBVH_SIGNED_INSIDE_ONLY);
    const uint32_t N = (uint32_t)n;
    Need need;
    need.sort = sort ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    TRY(zero_work(c, s));
    TRY(zero_counts(c, K_SIGNED, count, s));
    SignedArgs a{};
    fill_tree(c, a, QUERY_SIGNED_AT);
    a.points = reinterpret_cast<const float4*>(dev_points);
    a.out = reinterpret_cast<float4*>(dev_out);
    a.n = N;
    if (sort) a.perm = walk_order(c, launch_nearest_keys, a.points, N, s);
    if (near) {   // the closest-point pass: rtbvh_nearest's kernel into the same records, in the same order
        NearestArgs na{};
        fill_tree(c, na, QUERY_SIGNED_NEAR_AT);
        na.points = a.points;
        na.out = a.out;
        na.n = N;
        na.perm = a.perm;
        launch_nearest(na, count, s);
        TRY(zero_work(c, s));   // the work counters, again
    }
    launch_signed(a, count, near, vote3, s);
    return leave_chain(c, K_SIGNED, count, "signed kernels", s);
}

rtbvh_status rtbvh_signed_host(rtbvh_ctx* c, const rtbvh_point* points, uint64_t n, rtbvh_signed* out, uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, SIGNED, mode, nullptr, points, n, out, &run));
    if (!run) return RTBVH_OK;
    return host_records(c, SIGNED.name, points, (size_t)n * sizeof(rtbvh_point), out, (size_t)n * sizeof(rtbvh_signed),
                        [&](char* in, char* res) {
                            return rtbvh_signed_async(c, reinterpret_cast<const rtbvh_point*>(in), n,
                                                      reinterpret_cast<rtbvh_signed*>(res), mode, nullptr);
                        });
}

rtbvh_status rtbvh_signed_counts(rtbvh_ctx* c, uint64_t out[4]) {
    if (!out) return RTBVH_ERR_INVALID_ARG;
    uint64_t w[2 * QUERY_COUNT_WORDS];   // {points, inside, steps} of the ray pass, {points, found, steps} of the other
    TRY(kind_counts(c, K_SIGNED, w));
    out[0] = w[0];
    out[1] = w[1];
    out[2] = w[2] + w[QUERY_COUNT_WORDS + 2];
    out[3] = w[3] + w[QUERY_COUNT_WORDS + 3];
    return RTBVH_OK;
}

// ---- first-k ray queries -------------------------------------------------------------------------------
// One walk, no second pass.
rtbvh_status rtbvh_khits_async(rtbvh_ctx* c, const rtbvh_ray* dev_rays, uint64_t n, uint32_t k, rtbvh_hit* dev_hits,
                               uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, KHITS, mode, k == 0 || k > RTBVH_KHITS_MAX_K ? "khits: k must be 1 .. RTBVH_KHITS_MAX_K" : nullptr,
                     dev_rays, n, dev_hits, &run));
    if (!run) return RTBVH_OK;
    static_assert(sizeof(rtbvh_ray) == 32 && sizeof(rtbvh_hit) == 16, "first-k record layouts");
    static_assert(RTBVH_KHITS_MAX_K == KHITS_MAX_K, "the largest list of k_khits");
    const bool sort = (mode & RTBVH_KHITS_SORT) != 0, count = (mode & RTBVH_KHITS_COUNT) != 0;
    const uint32_t N = (uint32_t)n;
    Need need;
    need.sort = sort ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    TRY(zero_work(c, s));
    TRY(zero_counts(c, K_KHITS, count, s));
    KhitsArgs a{};
    fill_tree(c, a, QUERY_KHITS_AT);
    a.rays = reinterpret_cast<const float4*>(dev_rays);
    a.hits = reinterpret_cast<float4*>(dev_hits);
    a.n = N;
    a.k = k;
    if (sort) a.perm = walk_order(c, launch_query_keys, a.rays, N, s);
    launch_khits(a, count, s);
    return leave_chain(c, K_KHITS, count, "khits kernels", s);
}

rtbvh_status rtbvh_khits_host(rtbvh_ctx* c, const rtbvh_ray* rays, uint64_t n, uint32_t k, rtbvh_hit* hits,
                              uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, KHITS, mode, k == 0 || k > RTBVH_KHITS_MAX_K ? "khits: k must be 1 .. RTBVH_KHITS_MAX_K" : nullptr,
                     rays, n, hits, &run));
    if (!run) return RTBVH_OK;
    return host_records(c, KHITS.name, rays, (size_t)n * sizeof(rtbvh_ray), hits, (size_t)n * k * sizeof(rtbvh_hit),
                        [&](char* in, char* out) {
                            return rtbvh_khits_async(c, reinterpret_cast<const rtbvh_ray*>(in), n, k,
                                                     reinterpret_cast<rtbvh_hit*>(out), mode, nullptr);
                        });
}

rtbvh_status rtbvh_khits_counts(rtbvh_ctx* c, uint64_t out[4]) { return kind_counts(c, K_KHITS, out); }

// ---- sphere-sweep queries ------------------------------------------------------------------------------
// One walk, as the closest-point queries'; the walk order is the ray queries' (a sweep is a ray's two words).
rtbvh_status rtbvh_sweep_async(rtbvh_ctx* c, const rtbvh_sweep* dev_sweeps, uint64_t n, rtbvh_sweep_hit* dev_hits,
                               uint32_t mode, void* stream) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, SWEEP, mode, nullptr, dev_sweeps, n, dev_hits, &run));
    if (!run) return RTBVH_OK;
    static_assert(sizeof(rtbvh_sweep) == 32 && sizeof(rtbvh_sweep_hit) == 32, "sweep record layouts");
    const bool sort = (mode & RTBVH_SWEEP_SORT) != 0, count = (mode & RTBVH_SWEEP_COUNT) != 0;
    const uint32_t N = (uint32_t)n;
    Need need;
    need.sort = sort ? N : 0;
    hipStream_t s;
    TRY(enter_chain(c, stream, need, &s));
    TRY(zero_work(c, s));
    TRY(zero_counts(c, K_SWEEP, count, s));
    SweepArgs a{};
    fill_tree(c, a, QUERY_SWEEP_AT);
    a.sweeps = reinterpret_cast<const float4*>(dev_sweeps);
    a.hits = reinterpret_cast<float4*>(dev_hits);
    a.n = N;
    if (sort) a.perm = walk_order(c, launch_query_keys, a.sweeps, N, s);
    launch_sweep(a, (mode & RTBVH_SWEEP_ANY) != 0, count, s);
    return leave_chain(c, K_SWEEP, count, "sweep kernels", s);
}

rtbvh_status rtbvh_sweep_host(rtbvh_ctx* c, const rtbvh_sweep* sweeps, uint64_t n, rtbvh_sweep_hit* hits,
                              uint32_t mode) {
    if (!c) return RTBVH_ERR_INVALID_ARG;
    bool run;
    TRY(record_rules(c, SWEEP, mode, nullptr, sweeps, n, hits, &run));
    if (!run) return RTBVH_OK;
    return host_records(c, SWEEP.name, sweeps, (size_t)n * sizeof(rtbvh_sweep), hits,
                        (size_t)n * sizeof(rtbvh_sweep_hit), [&](char* in, char* out) {
                            return rtbvh_sweep_async(c, reinterpret_cast<const rtbvh_sweep*>(in), n,
                                                     reinterpret_cast<rtbvh_sweep_hit*>(out), mode, nullptr);
                        });
}

rtbvh_status rtbvh_sweep_counts(rtbvh_ctx* c, uint64_t out[4]) { return kind_counts(c, K_SWEEP, out); }

}  // extern "C"
