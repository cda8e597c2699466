/*
 * rtbvh.h -- C ABI of librtbvh.so, the MI355X (gfx950) LBVH build + ray traversal path.
 *
 * Drop-in boundary for the reference's GPU hot path (Fierykev/RayTraceBVH).  The
 * reference has no plugin API: the whole path is the private member
 * Graphics::computeBVH() (Graphics.cpp:667-831), fed through a D3D12 binding
 * contract (RayTraceGlobal.hlsl:87-120, Graphics.h:50-83, Graphics.cpp:293-303)
 * by Graphics::onUpdate() (Graphics.cpp:40-61) with inputs produced by
 * ObjLoader (ObjectFileLoader.h:120-240).  Each entry point below names the
 * reference interface it replaces.  See INTEGRATION.md for the binding a
 * maintainer adds on the reference side.
 *
 * Conventions: plain pointers and sizes only, no C++ or torch types.  A context
 * is single-thread affine and owns one HIP stream (or uses the caller's) and
 * every device buffer it allocates.  Input arrays are owned by the caller and
 * copied on the call.  Calls never throw; they return rtbvh_status and leave a
 * message for rtbvh_last_error().  All calls are synchronous unless the name
 * says `_async` (those only enqueue on the context stream).
 */
#ifndef RTBVH_H
#define RTBVH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTBVH_ABI_VERSION 8

typedef enum {
    RTBVH_OK = 0,
    RTBVH_ERR_INVALID_ARG = 1,
    RTBVH_ERR_HIP = 2,            /* a HIP runtime call failed (message has the HIP error) */
    RTBVH_ERR_OOM = 3,
    RTBVH_ERR_NOT_READY = 4,      /* e.g. trace before build, build before set_scene */
    RTBVH_ERR_STACK_OVERFLOW = 5, /* rays of a trace hit rtbvh_config.stack_limit (or a cyclic CPUTests-delta
                                     tree tripped the walk-length guard): the frame is complete; a per-lane
                                     walk's ray ended early, a packet walk skipped the subtree for the rays
                                     that hit it, each with the best hit found so far (stats.stack_overflows
                                     counts those rays per event); returned by the synchronising call
                                     after the trace (rtbvh_trace, rtbvh_compute_bvh, rtbvh_trace_tiles,
                                     rtbvh_synchronize), once per new overflow.  The reference's 32-entry
                                     stack is unchecked (RayTraceTraversal.hlsl:9,115,187). */
    RTBVH_ERR_IO = 6,             /* scene file could not be read / parsed */
    RTBVH_ERR_NO_DEVICE = 7,
    RTBVH_ERR_COMM = 8            /* RCCL missing or an RCCL call failed (message has the RCCL error) */
} rtbvh_status;

/* ---- data layouts (byte-identical to the reference's HLSL structs) -------- */

/* Vertex, RayTraceGlobal.hlsl:53-58 / ObjectFileLoader.h:98-103 (32 B) */
typedef struct {
    float position[3];
    float normal[3];
    float texcoord[2];
} rtbvh_vertex;

/* Material as uploaded, RayTraceGlobal.hlsl:60-72 / MaterialUpload ObjectFileLoader.h:79-96 (68 B) */
typedef struct {
    float ambient[4];
    float diffuse[4];
    float specular[4];
    float shininess;
    float optical_density;
    float alpha;
    uint32_t specularb; /* HLSL bool = 4 bytes */
    int32_t tex_num;    /* -1 = untextured */
} rtbvh_material;

/* Node, RayTraceGlobal.hlsl:39-51 / Graphics.h:157-169 (44 B).  Export layout
 * of rtbvh_read_bvh: leaves [0,n), internal node k at n+k, root at n.
 * parent of the root and child_l/child_r of leaves = 0xFFFFFFFF; internal
 * nodes have code = 0 and index = 0 (the reference leaves sort scratch there). */
typedef struct {
    uint32_t parent, child_l, child_r, code;
    float bb_min[3], bb_max[3];
    uint32_t index; /* 3 * triangle id, for leaves */
} rtbvh_node;

/* RayPresent, RayTraceGlobal.hlsl:30-35 (56 B) */
typedef struct {
    float intensity;
    float origin[3], direction[3], inv_direction[3];
    float color[4];
} rtbvh_ray_present;

/* An RGBA8 texture (sRGB encoded, as the reference's R8G8B8A8_UNORM_SRGB, Image.cpp:9).
 * Row 0 is the first row ilCopyPixels returns (Image.cpp:48-49; DevIL without IL_ORIGIN_SET
 * keeps the file's own row order: the bottom row first for BMP, the top row for JPEG) and
 * is texture row v = 0.  Sampling (RayTraceRender.hlsl:22-26, sampler Image.cpp:154-169:
 * MIN_MAG_MIP_LINEAR, WRAP, SampleLevel 0), as restated here (parity unpinned: DevIL and
 * the D3D filter precision are not available): texels decoded sRGB -> linear through the
 * table of rtbvh_srgb_table (alpha / 255), x = u*W - 0.5, y = v*H - 0.5, wrap, and
 * bilinear in fp32 as lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy). */
typedef struct {
    uint32_t width, height;
    const uint8_t* rgba8; /* width*height*4 bytes */
} rtbvh_texture;

enum {
    RTBVH_MORTON_CPUTESTS = 0, /* ShaderSim/main.cpp:292-301: object-space centroid, mesh AABB, x<<2|y<<1|z (default) */
    RTBVH_MORTON_HLSL = 1      /* MortonCodes.hlsl:70-106: clip-space, avg=bbMin/3, config scene box, x|y<<1|z<<2 */
};
enum {
    RTBVH_DELTA_CLZ64 = 0,   /* BVHConstructP1.hlsl:61-72: clz, ties 32 + clz(i^j) (default, always valid) */
    RTBVH_DELTA_CPUTESTS = 1 /* RadixBVHCombo/main.cpp:136-151: ties clz(i^j), De Bruijn quirks */
};
enum {
    RTBVH_FLAG_TIMING = 1u << 0,         /* record per-stage hipEvent times (rtbvh_get_stats) */
    RTBVH_FLAG_COUNT_VISITS = 1u << 1,   /* count traversal visits (slower; for the byte model) */
    RTBVH_FLAG_REFRACT_RECORDS = 1u << 2, /* keep the reflectRay and refractRay RayPresent records
                                             (RayTraceLaunch.hlsl:48-80, RayTraceReflection.hlsl:24-55)
                                             for rtbvh_read_rays */
    RTBVH_FLAG_SORT_BOUNCE = 1u << 3,     /* sort live bounce rays by (octant, origin Morton) before
                                             tracing them: same results, better coherence for the
                                             reference-order traversal */
    RTBVH_FLAG_NEAREST_FIRST = 1u << 4,   /* visit the nearer child first and keep the lexicographic
                                             (t, leaf) minimum: the reference DFS's answer unless
                                             rounding breaks box/triangle containment */
    RTBVH_FLAG_PACKET_PRIMARY = 1u << 5,  /* primary rays: one wave walks its 8x8 tile's rays as a
                                             masked packet with scalar node fetches (same per-ray
                                             visit sequence, same results) */
    RTBVH_FLAG_REFILL_BOUNCE = 1u << 6,   /* bounce rays: persistent traversal whose lanes take a new
                                             ray as soon as theirs is done, then a shading pass */
    RTBVH_FLAG_WIDE_BVH = 1u << 7,        /* trace: walk the node records 4-wide (a node's four grandchild
                                             boxes share one 128-B line), keeping the lexicographic
                                             (t, leaf) minimum as NEAREST_FIRST does */
    RTBVH_FLAG_AUTO_WALK = 1u << 8,       /* choose the walks, ignoring the walk flags (the four above and
                                             BINNED_PRIMARY), and return the reference-order frame always: up
                                             to 65536 triangles the reference-order kernels (exact by
                                             construction; the fastest on the reference's own meshes), the
                                             primary rays per lane or per wave packet, whichever the first
                                             frame of a (W, H, scene) timed faster (stats walk_flags); above
                                             that, the CERTIFIED fast walks: BINNED_PRIMARY and
                                             the 4-wide bounce walk, pruning on boxes grown by the triangle
                                             test's rounding margin so that they see every triangle that could
                                             be accepted below their bound, then a per-ray certificate (the
                                             winning leaf's own box passes the reference slab test at its t);
                                             the rays without one are re-traced in the reference order
                                             (stats walk_state 2, redo_rays).  No per-frame or per-camera check.
                                             The reference order throughout with a stack_limit below the
                                             capacity or the CPUTests delta */
    RTBVH_FLAG_BINNED_PRIMARY = 1u << 9,  /* primary rays: every leaf listed in the 32 x 32 screen tiles its box
                                             covers (the set of orthographic primary rays a box passes is a
                                             pixel rectangle, recorded by the build), then per tile each listed
                                             leaf tested against the pixels of its rectangle whose bound its
                                             min.z does not exceed, nearest depth bucket first, the (t, leaf)
                                             keys in LDS: the lexicographic minimum of the 4-wide walks, with no
                                             dependent record fetches.  Frames up to 32768 pixels
                                             a side (larger ones take the 4-wide packet walk); a tile whose bins
                                             overflow takes the per-lane nearest-first walk */
    RTBVH_FLAG_CERTIFIED = 1u << 10,      /* the certified fast walks of RTBVH_FLAG_AUTO_WALK whatever the scene's
                                             size (the reference-order frame, per-ray certificates) */
    RTBVH_FLAG_MULTI_KERNEL_BUILD = 1u << 16, /* scenes of <= 2048 triangles: use the multi-kernel
                                              build instead of the one-workgroup build (same output) */
    /* bits 17..19: trace chains (0 = automatic, n = 1..4): a trace deals its bands over n
       independent primary -> bounce kernel chains on n streams (same results) */
    RTBVH_FLAG_SPLIT_SHIFT = 17,
    RTBVH_FLAG_GRAPH = 1u << 20   /* rtbvh_compute_bvh replays one hipGraph of the whole frame (build +
                                     trace: ~20 launches and memsets), captured on the first call and
                                     re-captured when W, H, bounces, the flags or the scene change (not
                                     the camera: the kernels read it from a device buffer updated before
                                     each replay); no per-stage times (rtbvh_get_stats) */
};

typedef struct {
    int32_t device;          /* HIP device ordinal */
    uint32_t morton_mode;    /* RTBVH_MORTON_* */
    uint32_t delta_mode;     /* RTBVH_DELTA_* */
    uint32_t flags;          /* RTBVH_FLAG_* */
    float scene_bb_min[3];   /* MORTON_HLSL only: cbuffer sceneBBMin (Graphics.cpp:529 uses -700) */
    float scene_bb_max[3];   /* MORTON_HLSL only: cbuffer sceneBBMax (Graphics.cpp:528 uses +700) */
    void* stream;            /* hipStream_t to use, or NULL: the context creates its own */
    uint32_t stack_limit;    /* traversal stack entries a ray may use, 0 = the compiled capacity (66 binary,
                                100 for the 4-wide primary packets, 192 for the 4-wide bounce walk; a clz64
                                tree never needs more); 32 = the reference's stack
                                (RayTraceTraversal.hlsl:9): rays that would overflow it end early and the
                                trace reports RTBVH_ERR_STACK_OVERFLOW */
    uint32_t reserved;       /* must be 0 */
} rtbvh_config;

typedef struct {
    uint32_t num_tris, num_nodes, width, height;
    uint64_t primary_rays, bounce_rays;        /* rays traced by the last trace */
    /* RTBVH_FLAG_COUNT_VISITS only, last trace; [0] = primary pass, [1] = bounce passes */
    uint64_t internal_visits[2], leaf_visits[2], hits[2];
    uint64_t textured_hits, stack_overflows;
    /* RTBVH_FLAG_TIMING only: hipEvent averages over the builds / traces enqueued on
     * the context stream since rtbvh_reset_stats (the most recent 32 of each) */
    uint32_t timed_builds, timed_traces;
    float ms_build, ms_trace;
    float ms_stage[8];   /* 0 (the mesh box is computed by set_scene), morton, sort, karras, refit (+ leaf and node
                            records, QNodes), primary, bounce (all passes),
                            first bounce pass's traversal kernel (RTBVH_FLAG_REFILL_BOUNCE) */
    /* RTBVH_FLAG_COUNT_VISITS with RTBVH_FLAG_REFILL_BOUNCE: wave iterations of the bounce
     * traversal, those with both a leaf lane and an internal-node lane, and active lanes
     * summed over iterations (lane utilisation = active_lanes / (64 * wave_steps)) */
    uint64_t trav_wave_steps, trav_mixed_steps, trav_active_lanes;
    /* ... and the walk length of the bounce rays (loop iterations per ray): the longest,
     * and a histogram, [k] = rays of floor(log2(iterations)) == k */
    uint64_t trav_max_steps, trav_steps_log2[32];
    uint64_t graph_captures;   /* RTBVH_FLAG_GRAPH: frames captured so far (a replay captures nothing) */
    uint32_t walk_flags;       /* the walk flags the last trace's frame was traced with (RTBVH_FLAG_AUTO_WALK:
                                  the reference order, or the four walk flags once verified) */
    uint32_t walk_state;       /* RTBVH_FLAG_AUTO_WALK, last trace: 0 the reference order (<= 65536 triangles,
                                  a stack limit, the CPUTests delta) or no AUTO; 2 the certified fast walks */
    /* RTBVH_FLAG_COUNT_VISITS, wave-packet primary walks: wave steps (one record fetch for the
     * wave each) at internal nodes [0] and at leaves [1] */
    uint64_t packet_steps[2];
    /* RTBVH_FLAG_AUTO_WALK: traces run with the certified walks since rtbvh_create, and the rays the last
     * one re-traced in the reference order (no certificate: redo_rays[0] + redo_rays[1]).  ABI 7 renamed
     * them (ABI <= 5: walk_checks counted device frame checks and walk_fallbacks frame keys that fell back
     * to the reference order; a re-traced ray is normal, not a wrong fast walk) */
    uint64_t cert_traces, redo_total;
    /* RTBVH_FLAG_COUNT_VISITS, RTBVH_FLAG_BINNED_PRIMARY: (leaf, screen tile) bin entries of the primary
     * pass [0] and those that passed the tile's 8 x 8-block bound test [1] (one leaf-record fetch each) */
    uint64_t bin_entries[2];
    /* RTBVH_FLAG_AUTO_WALK, last trace: the rays re-traced in the reference order because their certificate
     * failed, of the primary pass [0] and of the bounce passes [1] (deferred rays included) */
    uint64_t redo_rays[2];
    /* RTBVH_FLAG_COUNT_VISITS with RTBVH_FLAG_REFILL_BOUNCE, last trace: the longest bounce walk, as its
     * loop iterations << 32 | the pixel (framebuffer index) of its ray */
    uint64_t trav_longest;
    /* RTBVH_FLAG_AUTO_WALK, last trace (ABI 8): of redo_rays[1], the bounce rays the certified walk's margin does
     * not cover (a direction component under 2^-20, |d| off unit, |o| > 2^90), deferred at their first step and
     * walked in the reference order by the walk's drained waves or the re-trace kernel */
    uint64_t redo_deferred;
    /* The walk-only tree (rtbvh_read_walk_qnodes; added at the end, the ABI number stays): how many the context has
     * made since rtbvh_create, and whether the last trace's certified bounce passes walked one (1) or the built
     * tree's QNodes (0) */
    uint64_t walk_tree_builds;
    uint32_t walk_tree_used;
    uint32_t reserved_walk_tree;
} rtbvh_stats;
typedef struct rtbvh_ctx rtbvh_ctx;

/* ---- lifecycle ------------------------------------------------------------ */
/* Fills cfg with defaults (device 0, CPUTests Morton, clz64 delta, +-700 box). */
void rtbvh_config_default(rtbvh_config* cfg);
/* Replaces Graphics::onInit/loadPipeline device + queue creation (Graphics.cpp:34-38,110-235). */
rtbvh_status rtbvh_create(const rtbvh_config* cfg, rtbvh_ctx** out);
/* Replaces Graphics::onDestroy (Graphics.cpp:94-103). NULL is a no-op. */
void rtbvh_destroy(rtbvh_ctx* ctx);
/* Last error message of this context (or of the last failed rtbvh_create when ctx == NULL). */
const char* rtbvh_last_error(const rtbvh_ctx* ctx);
int rtbvh_abi_version(void);
/* sizeof(rtbvh_stats) as this library was built: a binding checks its mirror of the struct against it */
uint32_t rtbvh_stats_size(void);

/* ---- inputs (the binding contract, RayTraceGlobal.hlsl:87-120) ------------ */
/* SRV t0 verts, t1 indices, t2 matIndices, t3 materials, t4.. textures:
 * replaces ObjLoader::UploadData (ObjectFileLoader.cpp:549-624).  nidx must be
 * a positive multiple of 3; mat_idx has nidx/3 entries; textures may be NULL. */
rtbvh_status rtbvh_set_scene(rtbvh_ctx* ctx, const rtbvh_vertex* verts, uint32_t nverts,
                             const uint32_t* indices, uint32_t nidx, const uint32_t* mat_idx,
                             const rtbvh_material* mats, uint32_t nmats,
                             const rtbvh_texture* textures, uint32_t ntex);
/* cbuffer WORLD_POS (b0) {WVP, WV}: replaces the CB write in Graphics::onUpdate
 * (Graphics.cpp:50-53).  Row-major 4x4, row-vector convention (p' = [p 1] * M),
 * i.e. the DirectXMath matrices BEFORE the transpose for HLSL packing. */
rtbvh_status rtbvh_set_camera(rtbvh_ctx* ctx, const float wvp[16], const float wv[16]);

/* ---- the hot path (Graphics::computeBVH, Graphics.cpp:667-831) ------------ */
/* MortonCodes -> radix sort -> BVHConstructP1 -> BVHConstructP2 (Graphics.cpp:705-782). */
rtbvh_status rtbvh_build(rtbvh_ctx* ctx);
rtbvh_status rtbvh_build_async(rtbvh_ctx* ctx);
/* RayTraceLaunch + `bounces` x RayTraceReflection (Graphics.cpp:785-810) at W x H. */
rtbvh_status rtbvh_trace(rtbvh_ctx* ctx, uint32_t width, uint32_t height, uint32_t bounces);
rtbvh_status rtbvh_trace_async(rtbvh_ctx* ctx, uint32_t width, uint32_t height, uint32_t bounces);
/* The whole computeBVH: build + trace (Graphics.cpp:667-831). */
rtbvh_status rtbvh_compute_bvh(rtbvh_ctx* ctx, uint32_t width, uint32_t height, uint32_t bounces);
/* Image-tile shard for multi-GPU (no reference equivalent): trace
 * only this rank's 8-row bands of a W x H frame under the context's deal (rtbvh_set_band_deal;
 * by default b % nranks == rank) and write them compacted (band order) as RGBA f32 into
 * dev_out (device memory, at least rtbvh_deal_rows(H, rank, nranks, share) * W * 4 floats,
 * = rtbvh_band_rows(H, rank, nranks) for the default deal), enqueued on `stream`
 * (hipStream_t, NULL = the context stream).  The caller gathers the shards.
 * Frames in flight: each caller stream other than the context's (up to 3) gets trace
 * buffers of its own over the one BVH, so traces on different streams run concurrently
 * (each into its own dev_out); they wait for the last build, and the next build waits for
 * them; rtbvh_synchronize waits for them too, and rtbvh_get_stats reports the last
 * trace.  Ray records (RTBVH_FLAG_REFRACT_RECORDS) are traced on the context stream only. */
rtbvh_status rtbvh_trace_band_async(rtbvh_ctx* ctx, uint32_t width, uint32_t height, uint32_t bounces,
                                    uint32_t rank, uint32_t nranks, float* dev_out, void* stream);
uint32_t rtbvh_band_rows(uint32_t height, uint32_t rank, uint32_t nranks);
/* The band deal.  Bands b = 0 .. ceil(H/8)-1 go to the ranks by smooth weighted round-robin:
 * rank 0 weighs root_share (0..16), every other rank 16; per band each rank's credit grows by its
 * weight and the rank with the most credit (lowest rank on a tie) takes the band and pays the total
 * weight.  root_share 16 (the default) is b % nranks; below 16, rank 0 -- which also receives and
 * assembles every other rank's bands -- traces root_share/16 of another rank's share, spread evenly
 * over the frame.  rtbvh_deal_bands writes rank's band indices in order (up to capacity) and
 * returns their count; rtbvh_deal_rows returns its rows.  rtbvh_set_band_deal sets the context's
 * deal for rtbvh_trace_band_async, rtbvh_assemble_bands and rtbvh_trace_tiles (every rank must use
 * the same root_share). */
uint32_t rtbvh_deal_bands(uint32_t height, uint32_t rank, uint32_t nranks, uint32_t root_share, uint32_t* bands,
                          uint32_t capacity);
uint32_t rtbvh_deal_rows(uint32_t height, uint32_t rank, uint32_t nranks, uint32_t root_share);
rtbvh_status rtbvh_set_band_deal(rtbvh_ctx* ctx, uint32_t root_share);
/* The per-scene identity check of a fast walk: traces the W x H frame in the reference order
 * (the exact findCollision DFS) and with the context's walk flags, compares the two on the device
 * and stores the number of pixels whose RGBA bits differ (0: the fast walk renders this frame
 * exactly as the reference order).  Synchronous; afterwards the context holds the frame of its
 * own walks, as after rtbvh_trace. */
rtbvh_status rtbvh_verify_walk(rtbvh_ctx* ctx, uint32_t width, uint32_t height, uint32_t bounces,
                               uint64_t* differing_pixels);
/* The frame from the ranks' compact band buffers, all on this device: buffer r (rank r's
 * rtbvh_trace_band_async output) starts stride_rows * W * 4 floats after buffer r-1
 * (stride_rows >= the most rows any rank has under the context's deal: rtbvh_deal_rows);
 * writes W*H*4 floats to dev_frame.
 * Enqueued on `stream` (NULL = the context stream).  rtbvh_trace_tiles uses it on rank 0. */
rtbvh_status rtbvh_assemble_bands(rtbvh_ctx* ctx, uint32_t width, uint32_t height, uint32_t nranks,
                                  const float* dev_bands, uint32_t stride_rows, float* dev_frame, void* stream);

/* ---- multi-GPU inside the library: one context per rank/GPU ----------
 * For a C/C++ host with no framework of its own.  RCCL is resolved at run time: the
 * process's librccl.so.1 if one is loaded (e.g. PyTorch's), else the system's; librtbvh.so
 * has no link-time RCCL dependency (RTBVH_ERR_COMM if none can be loaded).
 * rtbvh_comm_unique_id on rank 0, share the bytes with every rank (any channel), then
 * rtbvh_comm_init on every rank.  `comm` is an ncclComm_t; a host's own communicator
 * (one rank per GPU, same rank numbering) may be passed to rtbvh_trace_tiles instead. */
#define RTBVH_COMM_ID_BYTES 128
rtbvh_status rtbvh_comm_unique_id(uint8_t id[RTBVH_COMM_ID_BYTES]);
rtbvh_status rtbvh_comm_init(rtbvh_ctx* ctx, uint32_t nranks, uint32_t rank, const uint8_t id[RTBVH_COMM_ID_BYTES],
                             void** comm);
rtbvh_status rtbvh_comm_destroy(void* comm);
/* computeBVH's trace on nranks GPUs: this rank traces its 8-row bands (as
 * rtbvh_trace_band_async), every rank sends its bands to rank 0 (ncclSend / ncclRecv on the
 * context stream, one group) and rank 0 assembles the frame.  Collective: every rank calls
 * it with the same W, H, bounces.  Returns when this rank's part is done; afterwards
 * rtbvh_read_framebuffer / rtbvh_present on rank 0 give the whole frame (other ranks:
 * RTBVH_ERR_NOT_READY). */
rtbvh_status rtbvh_trace_tiles(rtbvh_ctx* ctx, uint32_t width, uint32_t height, uint32_t bounces, uint32_t rank,
                               uint32_t nranks, void* comm);
rtbvh_status rtbvh_synchronize(rtbvh_ctx* ctx);

/* ---- animated geometry: vertex updates and the topology-keeping refit ---------------------------
 * (No reference equivalent: the reference uploads its mesh once, ObjLoader::UploadData, and rebuilds the
 * BVH over it every frame, Graphics.cpp:56.)
 *
 * New positions (and normals) for vertices the scene already has.  Indices, materials, texcoords and
 * textures stay, nothing is reallocated, nothing waits on the host, and a captured frame
 * (RTBVH_FLAG_GRAPH) stays valid: rtbvh_update_vertices_async followed by rtbvh_compute_bvh replays it.
 * In RTBVH_MORTON_CPUTESTS mode the object-space mesh box is recomputed on the device in stream order.
 *
 * count vertices starting at `first`: positions (3 floats each, pos_stride floats apart, >= 3) and,
 * if dev_normals != NULL, normals (nrm_stride floats apart, >= 3), from device memory of the
 * context's device, enqueued on `stream` (NULL = the context stream).  A packed (V, 3) array has stride
 * 3, a float4 array 4, an rtbvh_vertex array 8 (positions at its base, normals 3 floats in).
 * Ordering: the update waits for the frames in flight and for the work already on the context stream;
 * the next build or refit waits for the update.  The arrays must stay as they are until the update has
 * run on `stream`.
 * After an update the built tree is not of the geometry: until the next rtbvh_build*, rtbvh_refit* or
 * rtbvh_compute_bvh, rtbvh_trace*, rtbvh_trace_band_async, rtbvh_trace_tiles, rtbvh_query_*, rtbvh_nearest_*,
 * rtbvh_within_*, rtbvh_knn_*, rtbvh_allhits_*, rtbvh_overlap_*, rtbvh_signed_*, rtbvh_khits_* and
 * rtbvh_verify_walk return RTBVH_ERR_NOT_READY, as do rtbvh_collide_async, rtbvh_collide_host, rtbvh_cross_async,
 * rtbvh_cross_host, rtbvh_cross_first_async, rtbvh_cross_first_host, rtbvh_clearance_async,
 * rtbvh_clearance_host, rtbvh_sweep_async and rtbvh_sweep_host, and the rtbvh_read_* calls return the last build's
 * tree.
 * RTBVH_ERR_INVALID_ARG: NULL positions, a stride below 3, first + count past the scene's vertices;
 * RTBVH_ERR_NOT_READY before rtbvh_set_scene; count == 0 is RTBVH_OK and touches nothing. */
rtbvh_status rtbvh_update_vertices_async(rtbvh_ctx* ctx, const float* dev_positions, uint32_t pos_stride,
                                         const float* dev_normals, uint32_t nrm_stride,
                                         uint32_t first, uint32_t count, void* stream);
/* host arrays, synchronous (stages and runs the same kernel) */
rtbvh_status rtbvh_update_vertices_host(rtbvh_ctx* ctx, const float* positions, uint32_t pos_stride,
                                        const float* normals, uint32_t nrm_stride,
                                        uint32_t first, uint32_t count);
/* New boxes over the last build's sort order and topology, for the current positions and camera: the
 * clip-space triangles, the leaf records and footprints, the node boxes or records (whichever the build
 * wrote), the quantized nodes and the root box are recomputed on the context stream; the Morton codes,
 * the sort and the Karras topology are kept (rtbvh_read_morton, rtbvh_read_sorted and the leaves' `code`
 * stay the last build's).  At every size, the one-workgroup build's trees included.  About the cost of
 * the build's last stage.  With RTBVH_MORTON_CPUTESTS (object-space codes) and unchanged vertices -- a
 * camera move -- the refitted tree is the rebuilt one bit for bit; for moved vertices it is a valid BVH
 * of the new geometry whose quality falls off as the mesh leaves the shape it was built for.
 * RTBVH_ERR_NOT_READY without a built tree.  rtbvh_compute_bvh keeps rebuilding; a refit is never part
 * of a captured frame, and RTBVH_FLAG_TIMING does not cover it. */
rtbvh_status rtbvh_refit_async(rtbvh_ctx* ctx);
rtbvh_status rtbvh_refit(rtbvh_ctx* ctx);

/* ---- ray queries: closest-hit and any-hit for rays the caller chose ----------------------------
 * (No reference equivalent: findCollision, RayTraceTraversal.hlsl:106-193, is reachable only through
 * the reference's own pixel rays.)
 *
 * Ray space: rays live in the space the BVH was built in -- vertex positions times the WVP of the last
 * build, .xyz, with no divide: the space of the RayPresent records and of rtbvh_read_bvh's boxes.  The map is
 * affine, so t is the same in object space when the caller transforms the origin as a point and the direction
 * as a vector WITHOUT renormalising it.  With an identity WVP the BVH space is object space.  The direction
 * need not be unit; 1 / direction is computed by the kernel. */
/* A ray, 32 B (two 16-B words): {origin.xyz, t_max}, {direction.xyz, reserved}.  t_max = +inf: no limit. */
typedef struct {
    float origin[3];
    float t_max;
    float direction[3];
    uint32_t reserved;
} rtbvh_ray;
/* A hit, 16 B: the distance t along the ray (hit point = origin + t * direction), the barycentrics of the hit
 * on vertices 1 and 2 of the triangle (rayTriangleCollision's u and v, RayTraceTraversal.hlsl:41-86), and the
 * triangle's id in triangle order (Node.index / 3).  A miss: t = -1, u = v = 0, tri = 0xFFFFFFFF. */
typedef struct {
    float t, u, v;
    uint32_t tri;
} rtbvh_hit;
enum {
    RTBVH_QUERY_CLOSEST = 0,      /* findCollision exactly: the left-first DFS, rayTriangleCollision's EPSILON, the
                                     strict `<` replacement.  t_max enters in two places only: a triangle's t is
                                     accepted iff the reference accepts it and t <= t_max; a box passes iff the
                                     reference's first two conditions hold and (hit ? mn <= dist : !(mn > t_max)).
                                     With t_max = +inf the reference, bit for bit.  A ray with a zero or
                                     non-finite direction or origin is a miss */
    RTBVH_QUERY_ANY = 1u << 0,    /* occlusion: the box test without the `hit` branch, the walk ends at the first
                                     accepted triangle, whose {t, u, v, tri} is the result (which triangle is
                                     unspecified).  Whether a ray hits equals the closest-hit answer */
    RTBVH_QUERY_SORT = 1u << 1,   /* walk the rays in (direction octant, origin Morton) order, as
                                     RTBVH_FLAG_SORT_BOUNCE does: same results, each at its ray's own index */
    RTBVH_QUERY_COUNT = 1u << 2,  /* count rays, hits and visits for rtbvh_query_counts (slower) */
    /* (bits 3-7 are rejected) */
    RTBVH_QUERY_CERTIFIED = 1u << 8 /* the same answer, faster: the certified 4-wide walk of a certified trace
                                      on the quantized nodes, t_max as its initial bound; each hit
                                     is checked against a per-ray certificate, and the rays without one -- and the
                                     rays the walk's margin does not cover: a direction with |d| above 1 or a
                                     component below 2^-20, |origin| above 2^90, NaN -- are re-traced in the reference
                                     order by the plain kernel.  Closest-hit: {t, u, v, tri} bit-identical to
                                     RTBVH_QUERY_CLOSEST's for every ray and t_max; with ANY: the same hit / miss
                                     answer, a reported hit a genuine one within t_max.  Composes with ANY, SORT and
                                     COUNT.  Where a certified trace cannot run -- a tree built with
                                     RTBVH_DELTA_CPUTESTS, or a stack_limit below the capacity -- the plain kernel
                                     takes every ray: RTBVH_OK and the same hits.  A build that wrote no quantized
                                     nodes gets them derived on the first such query */
};
/* n rays at dev_rays and n hits at dev_hits (device memory of the context's device, 16-B aligned), hit k for
 * ray k, enqueued on `stream` (hipStream_t, NULL = the context stream).  The walk reads the tree the last build
 * wrote.  Ordering: a query waits for the last build, the next build waits for the outstanding queries, and
 * rtbvh_synchronize waits for them; queries may be enqueued on any stream -- the library orders them among
 * themselves (they share scratch owned by the context, grown on demand), so queries on different streams run
 * one after the other.  The caller orders the rays' producer before, and the hits' consumer after, on `stream`.
 * The call only enqueues, with one exception: the first RTBVH_QUERY_SORT query of a context, and each one with
 * more rays than any before it, grows the sort's buffers, which waits on the host for the outstanding queries
 * and allocates device memory (size the first SORT query for the largest batch to keep later ones asynchronous).
 * RTBVH_QUERY_CERTIFIED's re-trace list (one word per ray) grows in the same way: the first certified query of a
 * context and each larger one wait on the host for the outstanding queries and allocate.
 * n == 0 returns RTBVH_OK and touches nothing; RTBVH_ERR_NOT_READY before a build; RTBVH_ERR_INVALID_ARG for
 * NULL pointers with n > 0, unknown mode bits, and n >= 2^31.  Rays that hit rtbvh_config.stack_limit end early
 * with the best hit found so far, and the next synchronising call returns RTBVH_ERR_STACK_OVERFLOW as after a
 * trace.  rtbvh_stats.stack_overflows stays the last trace's: the stats are read from the trace's own counter
 * block, which a query on another stream must not write while a trace or rtbvh_get_stats uses it. */
rtbvh_status rtbvh_query_async(rtbvh_ctx* ctx, const rtbvh_ray* dev_rays, uint64_t n, rtbvh_hit* dev_hits,
                               uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream; the hits are complete
 * when it returns RTBVH_ERR_STACK_OVERFLOW). */
rtbvh_status rtbvh_query_host(rtbvh_ctx* ctx, const rtbvh_ray* rays, uint64_t n, rtbvh_hit* hits, uint32_t mode);
/* The last RTBVH_QUERY_COUNT query (waits for it): rays, hits, internal-node visits, leaf visits. */
rtbvh_status rtbvh_query_counts(rtbvh_ctx* ctx, uint64_t out[4]);
/* ... and how its rays were answered: certified (by the 4-wide walk: a hit whose certificate passed, or an
 * exhaustive miss), redone (re-traced in the reference order: the certificate failed, or the walk flagged the ray
 * at a node without a grid or a stack overflow), uncovered (the margin does not cover the ray: the reference order
 * from the start), fallback (a query that took the plain kernel for every ray: one without RTBVH_QUERY_CERTIFIED, or
 * on a context where the certified walk cannot run).  The four sum to the query's rays.  For a certified query
 * rtbvh_query_counts' visit words count what the kernels visited: 4-wide node steps as internal visits, plus the
 * re-traces' visits; rays and hits stay exact.  RTBVH_ERR_NOT_READY before any counting query. */
rtbvh_status rtbvh_query_walk_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- Degenerate and non-finite scene triangles ---------------------------------------------------
 * Every build, refit, trace and query kind takes any scene.  A triangle is what its leaf record holds, and each
 * kind's answer stays the brute force of the kind's own formulas over those records, bit for bit, whatever the tree
 * (tests/test_hostile_gpu.py: points, needles, collinear and repeated-index triangles, duplicates, one-ulp slivers,
 * denormal and 1e25 coordinates, NaN and infinite vertices, mixed into a mesh).  What the formulas give:
 *  - Boxes.  A leaf box is fminf / fmaxf over the three vertices, which drop a NaN: a box is NaN on an axis only
 *    when all three vertices are, and a node's box is NaN iff every leaf below it is.  An infinite coordinate makes
 *    the boxes up to the root infinite.  (The WVP product spreads a non-finite component over its vertex: x * 0 is
 *    NaN.)  A refit back to finite positions leaves no NaN or infinity behind.
 *  - Rays (trace, query, allhits, khits, the signed rays).  A triangle without area (|det| < EPSILON: a point, a
 *    needle, a collinear or repeated-index triangle, a sliver, a denormal one) is never hit.  Nor is one with a NaN
 *    or infinite vertex, or whose products overflow: its t is a NaN or 0, and EPSILON < t is false.
 *  - Points (nearest, within, knn, the signed distance).  A triangle without area answers through `u, v: NaN -> 0`
 *    and the clamp: a point of its leaf box.  A non-finite vertex makes q a NaN, which the clamp fminf(hi, q) turns
 *    into hi: the triangle stands at the max corner of its leaf box, and can be an answer; all three vertices NaN:
 *    dist2 is a NaN, never an answer.  dist2 = +inf (a point or a triangle 1e19 away) satisfies
 *    dist2 <= max_dist2 = +inf: such a triangle is listed by within, returned by nearest when nothing is nearer,
 *    and stands in knn's list before the "none" slots.
 *  - Triangles by distance (clearance).  The same through both clamps: every candidate point is clamped into its own
 *    triangle's box, so a scene triangle with a non-finite vertex stands at a corner of its leaf box and can be an
 *    answer; all three vertices NaN: every candidate's d is a NaN, dist2 is a NaN, never an answer.  dist2 = +inf
 *    satisfies max_dist2 = +inf.  A point or a needle is a valid query, and a valid scene triangle: a zero-length
 *    segment has A or E = 0, its quotients are NaN or infinite, and clamp01 and the box clamps make points of them.
 *  - Sweeps.  A triangle without area has nn = 0 (or a den of 0 or NaN): the face candidate never counts, and a
 *    needle or a point is still touched through its edges and vertices -- a zero-length edge has ee = 0, so a_ = 0
 *    fails `a_ > 0`, and its end points answer as vertices.  The start overlap is the closest-point section's dist2,
 *    with its rules: a triangle with a non-finite vertex stands at a corner of its leaf box there, and feature 1 can
 *    report it.  A NaN fails every test of the candidates as written; all three vertices NaN: the leaf box is NaN,
 *    (B) fails, never a member.  An infinite leaf box passes (B) where the slabs are not NaN.
 *  - Boxes and triangles (overlap, cross, collide).  (B) compares the leaf box: a NaN fails it, an infinity meets.
 *    In RTBVH_OVERLAP_TRIANGLE a NaN separates nothing, so a non-finite triangle whose box meets the query box is
 *    listed, and a needle is decided by its edge axes.  In collide a triangle with one non-finite vertex keeps a
 *    finite edge, which can cross others: it is listed, while the same triangle as a cross QUERY is not walked.
 *  - The certified walks.  A subtree that holds a non-finite triangle carries E = inf and tcap = -1 and is never
 *    pruned by distance; a node whose boxes are non-finite or beyond 2^100 has no QNode frame, and a ray that
 *    reaches it is re-traced in the reference order.  With an infinite root box that is every covered ray:
 *    rtbvh_query_walk_counts reports certified = 0, and a certified trace re-traces every bounce ray (redo_rays[1];
 *    the binned primary pass is not affected).  The answers are the same. */

/* ---- closest-point queries: the nearest triangle to points the caller chose ---------------------
 * (No reference equivalent.)  For each point: which triangle is nearest, where on it, and how far away.
 *
 * Space: the space the BVH was built in, as the ray queries' -- vertex positions times the WVP of the last
 * build, .xyz, with no divide.  The map is affine, not isometric: distances are object-space distances only when
 * the BVH was built with an identity WVP (RTBVH_MORTON_CPUTESTS codes are object-space anyway, so that is the
 * build to use for this).
 *
 * The answer is specified exactly, independent of the tree and of the walk order.  A triangle's dist2 to the
 * point p is computed from its leaf record -- a = p0, e1 = fl(p1 - p0), e2 = fl(p2 - p0) and the leaf box
 * [lo, hi] -- in fp32 without contraction, dots as (x*x' + y*y') + z*z':
 *     ap = p - a;  d1 = dot(e1, ap);  d2 = dot(e2, ap)
 *     e11 = dot(e1, e1);  e12 = dot(e1, e2);  e22 = dot(e2, e2)
 *     d3 = d1 - e11;  d4 = d2 - e12;  d5 = d1 - e12;  d6 = d2 - e22
 *     vc = d1*d4 - d3*d2;  vb = d5*d2 - d1*d6;  va = d3*d6 - d5*d4
 *     (u, v) = the first region that matches:
 *       d1 <= 0 && d2 <= 0                   -> (0, 0)
 *       d3 >= 0 && d4 <= d3                  -> (1, 0)
 *       d6 >= 0 && d5 <= d6                  -> (0, 1)
 *       vc <= 0 && d1 >= 0 && d3 <= 0        -> (d1 / (d1 - d3), 0)
 *       vb <= 0 && d2 >= 0 && d6 <= 0        -> (0, d2 / (d2 - d6))
 *       va <= 0 && d4-d3 >= 0 && d5-d6 >= 0  -> w = (d4-d3) / ((d4-d3) + (d5-d6)); (1 - w, w)
 *       otherwise                            -> den = 1 / ((va + vb) + vc); (vb*den, vc*den)
 *     u, v: NaN -> 0   (a degenerate triangle: vertex 0 stands for it)
 *     q = (a + e1*u) + e2*v, then q = fmaxf(lo, fminf(hi, q)) per component
 *     e = p - q;  dist2 = dot(e, e)
 * The clamp into the leaf's own box makes dist2 never smaller than the point's distance to any box that contains
 * the leaf box, computed as (dx*dx + dy*dy) + dz*dz with dk = fmaxf(fmaxf(lo_k - p_k, p_k - hi_k), 0): the walk
 * prunes on that and still returns the brute-force answer bit for bit.
 * The result for p with bound max_dist2 is the lexicographic minimum of (dist2, triangle id) over the triangles
 * with dist2 <= max_dist2 (the id in triangle order, Node.index / 3); a NaN dist2 never wins.  No result, and no
 * walk: !(max_dist2 >= 0) (NaN included), a non-finite coordinate of p, or no triangle within the bound. */
/* A point, 16 B: {point.xyz, max_dist2}.  max_dist2 = +inf: no limit. */
typedef struct {
    float point[3];
    float max_dist2;
} rtbvh_point;
/* A result, 32 B (two 16-B words): the closest point q on the triangle, its squared distance, its barycentrics
 * on vertices 1 and 2 of the triangle (as rtbvh_hit's), the triangle's id in triangle order.
 * No result: dist2 = -1, point = u = v = 0, tri = 0xFFFFFFFF.  reserved = 0 always. */
typedef struct {
    float point[3];
    float dist2;
    float u, v;
    uint32_t tri;
    uint32_t reserved;
} rtbvh_nearest;
enum {
    RTBVH_NEAREST_SORT = 1u << 1,  /* walk the points in the order of their 30-bit Morton codes in the root box:
                                      same results, each at its point's own index */
    RTBVH_NEAREST_COUNT = 1u << 2  /* count points, results and steps for the counts call below (slower) */
    /* (every other bit is rejected) */
};
/* n points at dev_points and n results at dev_out (device memory of the context's device, 16-B aligned), result k
 * for point k, enqueued on `stream` (hipStream_t, NULL = the context stream).  The rules of rtbvh_query_async hold
 * one for one: the walk reads the tree the last build or refit wrote (node records, or the topology and node
 * boxes; never the quantized nodes); the call waits for the last build and only enqueues; closest-point and ray
 * queries share the context's query scratch, so the library orders them all among themselves -- queries on
 * different streams run one after the other -- and the next build waits for them; the first RTBVH_NEAREST_SORT
 * query and each larger one grow the sort's buffers (shared with RTBVH_QUERY_SORT), which waits on the host.
 * n == 0 returns RTBVH_OK and touches nothing; RTBVH_ERR_NOT_READY before a build and after a vertex update until
 * the next build or refit; RTBVH_ERR_INVALID_ARG for NULL pointers with n > 0, unknown mode bits, and n >= 2^31.
 * A walk that hits rtbvh_config.stack_limit ends with the best found so far, and the next synchronising call
 * returns RTBVH_ERR_STACK_OVERFLOW, as after a ray query. */
rtbvh_status rtbvh_nearest_async(rtbvh_ctx* ctx, const rtbvh_point* dev_points, uint64_t n, rtbvh_nearest* dev_out,
                                 uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream). */
rtbvh_status rtbvh_nearest_host(rtbvh_ctx* ctx, const rtbvh_point* points, uint64_t n, rtbvh_nearest* out,
                                uint32_t mode);
/* The last RTBVH_NEAREST_COUNT query (waits for it): points, results found, internal-node steps, leaf steps.  Its
 * own words: the ray queries' counts above keep reporting the last counting ray query.  RTBVH_ERR_NOT_READY before
 * any counting closest-point query. */
rtbvh_status rtbvh_nearest_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- radius queries: every triangle within a distance of points the caller chose ---------------
 * (No reference equivalent.)  Same points (rtbvh_point: {point.xyz, max_dist2}), same space and the same dist2 as
 * the closest-point queries above -- a triangle's dist2 is that section's, from the leaf record, fp32, no
 * contraction, with the clamp into the leaf's box.  The result of point k is the list of (triangle id, dist2) over
 * exactly the triangles with dist2 <= max_dist2 (the id in triangle order, Node.index / 3); a NaN dist2 is never
 * in the list.  The list is empty, and there is no walk, where the closest-point query has no walk:
 * !(max_dist2 >= 0) (NaN included) or a non-finite coordinate.  -0 counts as +0; max_dist2 = +inf lists every
 * triangle.  The set is exact, whatever the tree: dist2 is never below the distance to a box that contains the
 * leaf box, so pruning on box distance <= max_dist2 skips no member.
 * Order within a point's list: ascending by the triangle's position in the last build's sort order (tri_ids of
 * rtbvh_read_sorted; a refit keeps it) -- the order a left-first depth-first walk meets the leaves in, so the output
 * is reproducible down to the byte.
 * Output in CSR form: dev_offsets[0] = 0, point k's pairs are dev_pairs[dev_offsets[k] .. dev_offsets[k + 1]), and
 * dev_offsets[n] is the true total whatever `capacity` is.  A pair whose index is >= capacity is not written:
 * nothing is ever written past dev_pairs + capacity, capacity may be 0 (dev_pairs may then be NULL), and the
 * caller compares dev_offsets[n] with capacity. */
typedef struct {
    uint32_t tri;
    float dist2;
} rtbvh_pair; /* 8 B */
enum {
    RTBVH_WITHIN_SORT = 1u << 1,  /* walk the points in their Morton order (as RTBVH_NEAREST_SORT): same output */
    RTBVH_WITHIN_COUNT = 1u << 2, /* count points, pairs and steps for rtbvh_within_counts (slower) */
    RTBVH_WITHIN_SIZES = 1u << 4, /* write dev_offsets only; dev_pairs may be NULL */
    RTBVH_WITHIN_FILL = 1u << 5   /* dev_offsets is INPUT (from a SIZES call for the same points and tree): write
                                     the pairs only */
    /* SIZES | FILL together and every other bit: RTBVH_ERR_INVALID_ARG */
};
/* n points at dev_points, n + 1 offsets at dev_offsets (8-B aligned) and room for `capacity` pairs at dev_pairs
 * (device memory of the context's device), enqueued on `stream` (hipStream_t, NULL = the context stream).  Mode 0
 * runs the sizes pass, a scan of the offsets on the device and the fill pass in one call, with no host round trip;
 * RTBVH_WITHIN_SIZES then RTBVH_WITHIN_FILL is the two-call form for a caller who sizes dev_pairs from
 * dev_offsets[n].  A FILL over any non-decreasing offsets writes point k's pairs only inside
 * [dev_offsets[k], min(dev_offsets[k + 1], capacity)): offsets of another tree or bound truncate lists, they never
 * make a write go astray.
 * Everything else follows rtbvh_nearest_async one for one: the walk reads the tree the last build or refit wrote
 * (node records, or the topology and node boxes; never the quantized nodes); the call waits for the last build and
 * only enqueues; the library orders it among the ray and closest-point queries, and the next build waits for it.
 * The first RTBVH_WITHIN_SORT query and each larger one grow the sort's buffers, and the first query that writes
 * offsets and each larger one grow the scan's block sums: growing waits on the host for the outstanding queries.
 * n == 0 returns RTBVH_OK and writes dev_offsets[0] = 0 only if dev_offsets is non-NULL; RTBVH_ERR_NOT_READY before
 * a build and after a vertex update until the next build or refit; RTBVH_ERR_INVALID_ARG for NULL points or offsets
 * with n > 0, NULL pairs with capacity > 0 outside RTBVH_WITHIN_SIZES, bad mode bits, and n >= 2^31.
 * A walk that hits rtbvh_config.stack_limit loses that subtree's pairs -- both passes lose them identically, so
 * offsets and pairs stay consistent -- and the next synchronising call returns RTBVH_ERR_STACK_OVERFLOW. */
rtbvh_status rtbvh_within_async(rtbvh_ctx* ctx, const rtbvh_point* dev_points, uint64_t n, uint64_t* dev_offsets,
                                rtbvh_pair* dev_pairs, uint64_t capacity, uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream): offsets (n + 1) and pairs
 * are host arrays; pairs receives min(total, capacity) entries.  With RTBVH_WITHIN_FILL, offsets is read. */
rtbvh_status rtbvh_within_host(rtbvh_ctx* ctx, const rtbvh_point* points, uint64_t n, uint64_t* offsets,
                               rtbvh_pair* pairs, uint64_t capacity, uint32_t mode);
/* The last RTBVH_WITHIN_COUNT query (waits for it): points, pairs (the true total, counted once), internal-node
 * steps and leaf steps summed over the passes the call ran.  Its own words: the ray and closest-point counts keep
 * theirs.  RTBVH_ERR_NOT_READY before any counting radius query. */
rtbvh_status rtbvh_within_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- k-nearest queries: the k closest triangles to points the caller chose ----------------------
 * (No reference equivalent.)  Same points (rtbvh_point: {point.xyz, max_dist2}), same space and the same dist2 as
 * the closest-point queries above -- a triangle's dist2 is that section's, from the leaf record, fp32, no
 * contraction, with the clamp into the leaf's box.  The result for p with bound max_dist2 and k is the k
 * lexicographically smallest (dist2, triangle id) among the triangles with dist2 <= max_dist2 (the id in triangle
 * order, Node.index / 3), in ascending order.  The order is total, so the result is a function of the point and the
 * triangles alone: whatever the tree, the walk order or the mode, down to the byte.  A NaN dist2 is never a member.
 * There is no walk, and every slot holds "none", where the closest-point query has no walk: !(max_dist2 >= 0) (NaN
 * included) or a non-finite coordinate.  -0 counts as +0; max_dist2 = +inf means no limit.  With k = 1 the pair is
 * rtbvh_nearest's (tri, dist2).  The list is exact: dist2 is never below the distance to a box that contains the
 * leaf box, and the walk prunes on box distance <= the dist2 of the worst of the k kept so far, which is never below
 * the final one's.
 * Output: n * k records of the radius queries' 8-B rtbvh_pair, point i's at [i * k, (i + 1) * k); a slot past the
 * number found holds {0xFFFFFFFF, -1.0f}.  No CSR, no second pass, no capacity. */
#define RTBVH_KNN_MAX_K 32
enum {
    RTBVH_KNN_SORT = 1u << 1,  /* walk the points in Morton order (as RTBVH_NEAREST_SORT): same output */
    RTBVH_KNN_COUNT = 1u << 2  /* count for rtbvh_knn_counts (slower) */
    /* (every other bit is rejected) */
};
/* n points at dev_points and room for n * k pairs at dev_pairs (device memory of the context's device, 8-B aligned),
 * enqueued on `stream` (hipStream_t, NULL = the context stream).  k == 0 or k > RTBVH_KNN_MAX_K is
 * RTBVH_ERR_INVALID_ARG.
 * Everything else follows rtbvh_nearest_async one for one: the walk reads the tree the last build or refit wrote
 * (node records, or the topology and node boxes; never the quantized nodes); the call waits for the last build and
 * only enqueues; the library orders it among all the other queries, and the next build waits for it.  The first
 * RTBVH_KNN_SORT query and each larger one grow the sort's buffers (shared with the other queries' SORT), which
 * waits on the host.  n == 0 returns RTBVH_OK and touches nothing, even before a build; RTBVH_ERR_NOT_READY before
 * a build and after a vertex update until the next build or refit; RTBVH_ERR_INVALID_ARG for NULL pointers with
 * n > 0, bad mode bits, a bad k and n >= 2^31.
 * A walk that hits rtbvh_config.stack_limit ends with the best list found so far, and the next synchronising call
 * returns RTBVH_ERR_STACK_OVERFLOW: every pair of that list is a genuine (tri, dist2), the list is ascending, and
 * slot by slot it is never lexicographically below the true one. */
rtbvh_status rtbvh_knn_async(rtbvh_ctx* ctx, const rtbvh_point* dev_points, uint64_t n, uint32_t k,
                             rtbvh_pair* dev_pairs, uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream). */
rtbvh_status rtbvh_knn_host(rtbvh_ctx* ctx, const rtbvh_point* points, uint64_t n, uint32_t k, rtbvh_pair* pairs,
                            uint32_t mode);
/* The last RTBVH_KNN_COUNT query (waits for it): points, pairs found, internal-node steps, leaf steps.  Its own
 * words: the other queries' counts keep theirs.  RTBVH_ERR_NOT_READY before any counting k-nearest query. */
rtbvh_status rtbvh_knn_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- all-hits ray queries: every triangle a ray crosses within t_max ----------------------------
 * (No reference equivalent.)  Space, rays and hits are the ray queries' above: rtbvh_ray in, rtbvh_hit
 * {t, u, v, tri} out.  The result of ray k is the list of the hits of exactly its MEMBERS, specified independently
 * of the tree and of the walk.  With o, d, t_max the ray's and inv = 1 / d per component (fp32, correctly
 * rounded), triangle x is a member iff both hold, on the floats of its leaf record (p0, e1 = fl(p1 - p0),
 * e2 = fl(p2 - p0), the leaf box [lo, hi]):
 *   (B) its own leaf box passes the any-hit box rule: with t0 = (lo - o) * inv, t1 = (hi - o) * inv per axis,
 *         mn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z))
 *         mx = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z))
 *       (fminf and fmaxf drop NaN), the box passes iff 0 <= mx && mn <= mx && !(mn > t_max);
 *   (T) rayTriangleCollision (RayTraceTraversal.hlsl:41-86, fp32, no contraction) accepts with some t, and
 *       t <= t_max.
 * Its hit is {t, u, v, tri}: the floats the accepting test computed -- the bits rtbvh_query_* reports for that
 * triangle -- and the id in triangle order (Node.index / 3).  (B) is part of the definition because findCollision
 * reaches a triangle only through its leaf box: for an axis-parallel ray that starts exactly on the box's face the
 * reference's own slab test rejects the leaf, and a triangle it never tests is no hit of the ray.  So the list is
 * exactly the set of hits findCollision can ever return for the ray: rtbvh_query_*'s closest hit is always in it,
 * and it is empty iff that query misses.  The set is exact whatever the tree: the slab test is monotone in the
 * box, so every box around a member's leaf box passes too, and a walk with the fixed bound t_max skips no member
 * (DESIGN.md 5f).
 * The list is empty, and there is no walk, for a ray with a non-finite component of o or d, with d all zero, or
 * with !(t_max > 0) (NaN included).  t_max = +inf: no limit.
 * Order within a ray's list: ascending by the triangle's position in the last build's sort order (tri_ids of
 * rtbvh_read_sorted; a refit keeps it), as a radius query's list; with RTBVH_ALLHITS_BY_T ascending by (t, tri)
 * -- t > 0, so by the 64-bit key t bits << 32 | tri -- a total order: the output is then a function of the rays
 * and the triangles alone.
 * Output in CSR form, as rtbvh_within_async's: dev_offsets[0] = 0, ray k's hits are
 * dev_hits[dev_offsets[k] .. dev_offsets[k + 1]), and dev_offsets[n] is the true total whatever `capacity` is.  A
 * hit whose index is >= capacity is not written: nothing is ever written past dev_hits + capacity, capacity may be
 * 0 (dev_hits may then be NULL), and the caller compares dev_offsets[n] with capacity. */
enum {
    RTBVH_ALLHITS_SORT = 1u << 1,  /* walk the rays in (direction octant, origin Morton) order, as RTBVH_QUERY_SORT:
                                      same output */
    RTBVH_ALLHITS_COUNT = 1u << 2, /* count rays, hits and steps for rtbvh_allhits_counts (slower) */
    RTBVH_ALLHITS_BY_T = 1u << 3,  /* each ray's list ascending by (t, tri) instead of sort-order position */
    RTBVH_ALLHITS_SIZES = 1u << 4, /* write dev_offsets only; dev_hits may be NULL */
    RTBVH_ALLHITS_FILL = 1u << 5   /* dev_offsets is INPUT (from a SIZES call for the same rays and tree): write
                                      (and with BY_T order) the hits only */
    /* SIZES | FILL, SIZES | BY_T and every other bit: RTBVH_ERR_INVALID_ARG */
};
/* n rays at dev_rays (16-B aligned), n + 1 offsets at dev_offsets (8-B aligned) and room for `capacity` hits at
 * dev_hits (16-B aligned; device memory of the context's device), enqueued on `stream` (hipStream_t, NULL = the
 * context stream).  Mode 0 runs the sizes pass, a scan of the offsets on the device and the fill pass in one call,
 * with no host round trip; RTBVH_ALLHITS_SIZES then RTBVH_ALLHITS_FILL is the two-call form.  A FILL over any
 * non-decreasing offsets writes ray k's hits only inside [dev_offsets[k], min(dev_offsets[k + 1], capacity)): a
 * list that does not fit its segment is cut to its first hits in sort-order position.  RTBVH_ALLHITS_BY_T orders,
 * in place and after the fill, exactly the hits that were written: a cut list is that prefix, ordered.
 * Everything else follows rtbvh_within_async one for one: the walk reads the tree the last build or refit wrote
 * (node records, or the topology and node boxes; never the quantized nodes); the call waits for the last build and
 * only enqueues; the library orders it among all other queries, and the next build waits for it.  The first
 * RTBVH_ALLHITS_SORT query and each larger one grow the sort's buffers, the first query that writes offsets and
 * each larger one the scan's block sums, the first RTBVH_ALLHITS_BY_T query and each larger one two words per
 * ray: growing waits on the host for the outstanding queries.  No device memory proportional to the output is
 * allocated.
 * n == 0 returns RTBVH_OK and writes dev_offsets[0] = 0 only if dev_offsets is non-NULL; RTBVH_ERR_NOT_READY before
 * a build and after a vertex update until the next build or refit; RTBVH_ERR_INVALID_ARG for NULL rays or offsets
 * with n > 0, NULL hits with capacity > 0 outside RTBVH_ALLHITS_SIZES, bad mode bits, and n >= 2^31.
 * A walk that hits rtbvh_config.stack_limit loses that subtree's hits -- both passes lose them identically, so
 * offsets and hits stay consistent -- and the next synchronising call returns RTBVH_ERR_STACK_OVERFLOW. */
rtbvh_status rtbvh_allhits_async(rtbvh_ctx* ctx, const rtbvh_ray* dev_rays, uint64_t n, uint64_t* dev_offsets,
                                 rtbvh_hit* dev_hits, uint64_t capacity, uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream): offsets (n + 1) and hits
 * are host arrays; hits receives min(total, capacity) entries.  With RTBVH_ALLHITS_FILL, offsets is read. */
rtbvh_status rtbvh_allhits_host(rtbvh_ctx* ctx, const rtbvh_ray* rays, uint64_t n, uint64_t* offsets,
                                rtbvh_hit* hits, uint64_t capacity, uint32_t mode);
/* The last RTBVH_ALLHITS_COUNT query (waits for it): rays, hits (the true total, counted once), internal-node
 * steps and leaf steps summed over the passes the call ran.  Its own words: the other queries' counts keep theirs.
 * RTBVH_ERR_NOT_READY before any counting all-hits query. */
rtbvh_status rtbvh_allhits_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- first-k ray queries: a ray's k nearest crossings (multi-hit traversal) ---------------------
 * (No reference equivalent.)  Rays, space, hits and MEMBERS are the all-hits queries' above: triangle x is a member
 * of a ray iff (B) and (T) of that section hold, there is no walk under the same rules (a non-finite component of o
 * or d, d all zero, !(t_max > 0)), and t_max = +inf means no limit.
 * Key of a member x: with t_x the t of (T) and mn_x the slab entry `mn` of x's own leaf box, computed exactly as in
 * (B), tk_x = fmaxf(t_x, mn_x) (fmaxf drops a NaN).  t_x > EPSILON > 0 and tk_x <= t_max, so tk's bits order as the
 * floats, and the 64-bit key tk bits << 32 | tri is a total order.  The box is in the key because a triangle's t is
 * often a few ulps BELOW the slab entry of its own leaf box: "the first k by t" cannot be walked with pruning,
 * this can, as the closest-point queries clamp into the leaf box.
 * The result for a ray and k is its k members with the smallest keys, in ascending key order, each reported as
 * {t, u, v, tri}: the genuine t, u, v that rtbvh_query_* and rtbvh_allhits_* report for that triangle -- not tk.  It
 * is a function of the ray and the triangles alone: whatever the tree, the walk order or the mode, down to the byte.
 *  - t within a list is ascending except where an entry's key was clamped (tk = mn > t): those entries are within
 *    rounding of their neighbours.
 *  - Exactly coplanar crossings whose leaf boxes start at the same mn order by triangle id, whatever their t's
 *    last bits say.
 *  - Slot 0 is a hit iff the closest-hit query rtbvh_query_* hits.
 *  - With k at least the length of the ray's all-hits list, the list is that set.
 * The list is exact: every box around x's leaf box passes the first two slab conditions when the leaf box does, and
 * starts at mn <= mn_x <= tk_x; the walk enters a box -- a child's, or a leaf's own at the leaf -- iff
 * 0 <= mx && mn <= mx && !(mn > bound), where bound is the tk of the worst of the k kept so far (t_max until k are
 * kept), which only falls and is never below the final one's.
 * Output: n * k rtbvh_hit records, ray i's at [i * k, (i + 1) * k); a slot past the number found holds the miss
 * record {-1, 0, 0, 0xFFFFFFFF}, and a ray with no walk gets k of them.  No CSR, no second pass, no capacity. */
#define RTBVH_KHITS_MAX_K 16
enum {
    RTBVH_KHITS_SORT = 1u << 1,  /* walk the rays in RTBVH_QUERY_SORT's order: same output */
    RTBVH_KHITS_COUNT = 1u << 2  /* count for rtbvh_khits_counts (slower) */
    /* (every other bit is rejected) */
};
/* n rays at dev_rays and room for n * k hits at dev_hits (device memory of the context's device, 16-B aligned),
 * enqueued on `stream` (hipStream_t, NULL = the context stream).  k == 0 or k > RTBVH_KHITS_MAX_K is
 * RTBVH_ERR_INVALID_ARG (a ray that needs more layers has rtbvh_allhits_*).
 * Everything else follows rtbvh_knn_async one for one: the walk reads the tree the last build or refit wrote (node
 * records, or the topology and node boxes; never the quantized nodes); the call waits for the last build and only
 * enqueues; the library orders it among all the other queries, and the next build waits for it.  The first
 * RTBVH_KHITS_SORT query and each larger one grow the sort's buffers (shared with the other queries' SORT), which
 * waits on the host.  n == 0 returns RTBVH_OK and touches nothing, even before a build; RTBVH_ERR_NOT_READY before
 * a build and after a vertex update until the next build or refit; RTBVH_ERR_INVALID_ARG for NULL pointers with
 * n > 0, bad mode bits, a bad k and n >= 2^31.
 * A walk that hits rtbvh_config.stack_limit ends with the best list found so far, and the next synchronising call
 * returns RTBVH_ERR_STACK_OVERFLOW: every listed hit is a genuine member's, the list is ascending by key, and slot
 * by slot its key is never below the true one's. */
rtbvh_status rtbvh_khits_async(rtbvh_ctx* ctx, const rtbvh_ray* dev_rays, uint64_t n, uint32_t k,
                               rtbvh_hit* dev_hits, uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream). */
rtbvh_status rtbvh_khits_host(rtbvh_ctx* ctx, const rtbvh_ray* rays, uint64_t n, uint32_t k, rtbvh_hit* hits,
                              uint32_t mode);
/* The last RTBVH_KHITS_COUNT query (waits for it): rays, hits found, internal-node steps, leaf steps.  Its own
 * words: the other queries' counts keep theirs.  RTBVH_ERR_NOT_READY before any counting first-k query. */
rtbvh_status rtbvh_khits_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- self-collision queries: the pairs of the mesh's own triangles that cross each other --------
 * (No reference equivalent; Embree's rtcCollide of a scene with itself.)  No shapes come from the caller: the
 * query is the built mesh against itself, in the space the BVH was built in.  The result is the set of MEMBER pairs,
 * specified independently of the tree and of the walk.  All floats come from the leaf records of the last build or
 * refit: for a triangle x its a = p0, e1 = fl(p1 - p0), e2 = fl(p2 - p0) and leaf box [lo, hi].  Arithmetic is fp32
 * without contraction, every product rounded, with dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z and
 * cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x).  The three edge segments (P, D) of x
 * are, in this order, S0 = (a, e1), S1 = (a, e2), S2 = (fl(a + e1), fl(e2 - e1)), componentwise.
 * A pair {x, y} of different triangles is a member iff
 *  (N) they are not neighbours: no vertex index of x equals a vertex index of y -- nine integer comparisons on the
 *      scene's index buffer, indices[3x .. 3x + 2] against indices[3y .. 3y + 2].  Triangles that share a vertex
 *      always touch there; listing them would bury the real contacts.
 *  (B) their leaf boxes meet: lo_x <= hi_y && lo_y <= hi_x on every axis.  Closed intervals (touching counts), the
 *      box queries' comparisons, no arithmetic; a NaN fails it.
 *  (X) with RTBVH_COLLIDE_TRIANGLE only: at least one of the six tests "segment S_k(x) crosses triangle y",
 *      "segment S_k(y) crosses triangle x", k = 0 .. 2, holds.  "Segment (P, D) crosses the triangle (p0, e1, e2)"
 *      is the signed-distance queries' rule (X) with the segment's far end added:
 *        tmp = cross(D, e2);  det = dot(e1, tmp);  rt = P - p0
 *        U = dot(rt, tmp);  tmp2 = cross(rt, e1);  V = dot(D, tmp2);  N = dot(e2, tmp2)
 *        if det < 0: negate det, U, V and N (exact)
 *        crosses iff det > 0 && U >= 0 && V >= 0 && U + V <= det && N >= 0 && N <= det
 *      No division, no epsilon; a NaN compares false; touching counts, as in the box queries.  Both orders of a
 *      pair evaluate the same six tests: the rule is symmetric in x and y by construction.
 * Limits: coplanar triangles have det = 0 in every test and are not reported.  A contact within rounding can go
 * either way, but the same way on every tree.  A mesh with unwelded duplicate vertices reports the faces that touch
 * along the duplicated vertices, because (N) looks at indices, not positions.
 * The set is exact whatever the tree: (B) is monotone in the tree's box, so a walk that enters a child iff its box
 * meets x's leaf box reaches every partner of x (the box queries' argument).
 * Output in CSR form over TRIANGLES, indexed by triangle id (triangle order, Node.index / 3): dev_offsets has T + 1
 * entries, dev_offsets[0] = 0, triangle i's partners are dev_ids[dev_offsets[i] .. dev_offsets[i + 1]), and
 * dev_offsets[T] is the true total whatever `capacity` is.  Each list is ascending by the partner's position in the
 * last build's sort order (tri_ids of rtbvh_read_sorted; a refit keeps it).  By default a pair appears once, in the
 * list of the triangle that comes earlier in that sort order; with RTBVH_COLLIDE_SYMMETRIC it appears in both
 * triangles' lists, and a sizes pass alone is then the per-triangle contact count.  An id whose index is >= capacity
 * is not written: nothing is ever written past dev_ids + capacity, capacity may be 0 (dev_ids may then be NULL), and
 * the caller compares dev_offsets[T] with capacity. */
enum {
    RTBVH_COLLIDE_COUNT = 1u << 2,     /* count triangles, entries and steps for rtbvh_collide_counts (slower) */
    RTBVH_COLLIDE_TRIANGLE = 1u << 3,  /* rule (X) as well: the triangles cross, not only their leaf boxes */
    RTBVH_COLLIDE_SIZES = 1u << 4,     /* write dev_offsets only; dev_ids may be NULL */
    RTBVH_COLLIDE_FILL = 1u << 5,      /* dev_offsets is INPUT (from a SIZES call of the same mode and tree): write
                                          the ids only */
    RTBVH_COLLIDE_SYMMETRIC = 1u << 6  /* a pair is listed by both of its triangles */
    /* SIZES | FILL together and every other bit: RTBVH_ERR_INVALID_ARG.  There is no SORT bit: the queries are the
       leaves, walked in sort order, which is the coherent order already. */
};
/* T + 1 offsets at dev_offsets (8-B aligned) and room for `capacity` ids at dev_ids (device memory of the context's
 * device), enqueued on `stream` (hipStream_t, NULL = the context stream).  Mode 0 runs the sizes pass, a scan of the
 * offsets on the device and the fill pass in one call, with no host round trip; RTBVH_COLLIDE_SIZES then
 * RTBVH_COLLIDE_FILL is the two-call form.  A FILL over any non-decreasing offsets writes triangle i's ids only
 * inside [dev_offsets[i], min(dev_offsets[i + 1], capacity)): offsets of another mode or tree truncate lists to
 * their first ids, they never make a write go astray.
 * Everything else follows rtbvh_overlap_async one for one: the walk reads the tree the last build or refit wrote
 * (node records, or the topology and node boxes; never the quantized nodes); the call waits for the last build and
 * only enqueues; the library orders it among all other queries, and the next build waits for it.  The first query
 * that writes offsets and each larger one grow the scan's block sums, which waits on the host for the outstanding
 * queries.  A scene of one triangle gives offsets {0, 0}.
 * RTBVH_ERR_NOT_READY before a build and after a vertex update until the next build or refit;
 * RTBVH_ERR_INVALID_ARG for NULL offsets, NULL ids with capacity > 0 outside RTBVH_COLLIDE_SIZES, and bad mode bits.
 * A walk that hits rtbvh_config.stack_limit loses that subtree's ids -- both passes lose them identically, so
 * offsets and ids stay consistent -- and the next synchronising call returns RTBVH_ERR_STACK_OVERFLOW. */
rtbvh_status rtbvh_collide_async(rtbvh_ctx* ctx, uint64_t* dev_offsets, uint32_t* dev_ids, uint64_t capacity,
                                 uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream): offsets (T + 1) and ids are
 * host arrays; ids receives min(total, capacity) entries.  With RTBVH_COLLIDE_FILL, offsets is read. */
rtbvh_status rtbvh_collide_host(rtbvh_ctx* ctx, uint64_t* offsets, uint32_t* ids, uint64_t capacity, uint32_t mode);
/* The last RTBVH_COLLIDE_COUNT query (waits for it): triangles (T), entries (the true total, counted once),
 * internal-node steps and leaf steps summed over the passes the call ran.  Its own words: the other queries' counts
 * keep theirs.  RTBVH_ERR_NOT_READY before any counting self-collision query. */
rtbvh_status rtbvh_collide_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- triangle queries: the scene triangles that a caller's triangle crosses --------
 * (No reference equivalent; Embree's rtcCollide of a second mesh with the built one.)  The query triangles live in
 * the space the BVH was built in, as every other query's input.  The result of query triangle q is the list of the
 * ids (in triangle order, Node.index / 3) of exactly the scene triangles that are MEMBERS of it, specified operation
 * for operation, independently of the tree and of the walk.  From q's vertices, in fp32 without contraction:
 *     a = v0,  e1 = fl(v1 - v0),  e2 = fl(v2 - v0),
 *     qlo = fminf(fminf(v0, v1), v2),  qhi = fmaxf(fmaxf(v0, v1), v2), per component
 * -- the floats a leaf record would hold if q were a scene triangle.  For a scene triangle x its leaf record's p0,
 * e1, e2 and its leaf box [lo, hi], as in the self-collision section.  x is a member of q iff
 *  (B) on every axis k: qlo_k <= hi_k && lo_k <= qhi_k.  Closed intervals (touching counts), no arithmetic; a NaN
 *      fails it.
 *  (X) at least one of the six tests "segment S_k(q) crosses triangle x", "segment S_k(x) crosses triangle q",
 *      k = 0 .. 2, holds: the self-collision section's segments S0, S1, S2 and its rule "segment (P, D) crosses the
 *      triangle (p0, e1, e2)", unchanged, with q's (a, e1, e2) in the place of a leaf record's.
 * There is no rule (N): the caller's mesh has no indices in common with the scene's.
 * Limits: coplanar pairs have det = 0 in every test and are not listed.  A contact within rounding can go either
 * way, but the same way on every tree.  A query triangle that lies entirely inside a closed mesh crosses nothing: its
 * list is empty (containment is rtbvh_signed_*'s question).  A scene triangle queried with its own floats may or may
 * not list itself (rounding in det).
 * The list is empty, and there is no walk, for a query triangle with a non-finite component in any vertex.
 * Degenerate triangles (a point, a needle) are valid queries and follow the rules above.
 * The set is exact whatever the tree: (B) is monotone in the tree's box, so a walk that enters a child iff its box
 * meets [qlo, qhi] reaches every member (the box queries' argument).
 * Order and output are rtbvh_overlap_async's, word for word: each list ascends by the member's position in the last
 * build's sort order (tri_ids of rtbvh_read_sorted; a refit keeps it); CSR form, dev_offsets[0] = 0, query k's ids
 * are dev_ids[dev_offsets[k] .. dev_offsets[k + 1]), and dev_offsets[n] is the true total whatever `capacity` is.  An
 * id whose index is >= capacity is not written: nothing is ever written at or past dev_ids + capacity, capacity may
 * be 0 (dev_ids may then be NULL), and the caller compares dev_offsets[n] with capacity. */
typedef struct {
    float v0[3];
    uint32_t reserved0; /* ignored */
    float v1[3];
    uint32_t reserved1; /* ignored */
    float v2[3];
    uint32_t reserved2; /* ignored */
} rtbvh_tri; /* 48 B: three 16-B words */
enum {
    RTBVH_CROSS_SORT = 1u << 1,  /* walk the queries in the Morton order of their box centres: same output */
    RTBVH_CROSS_COUNT = 1u << 2, /* count queries, ids and steps for rtbvh_cross_counts (slower) */
    RTBVH_CROSS_SIZES = 1u << 4, /* write dev_offsets only; dev_ids may be NULL */
    RTBVH_CROSS_FILL = 1u << 5   /* dev_offsets is INPUT (from a SIZES call for the same triangles and tree): write
                                    the ids only */
    /* SIZES | FILL together and every other bit: RTBVH_ERR_INVALID_ARG */
};
/* n triangles at dev_tris (16-B aligned), n + 1 offsets at dev_offsets (8-B aligned) and room for `capacity` ids at
 * dev_ids (device memory of the context's device), enqueued on `stream` (hipStream_t, NULL = the context stream).
 * Mode 0 runs the sizes pass, a scan of the offsets on the device and the fill pass in one call, with no host round
 * trip; RTBVH_CROSS_SIZES then RTBVH_CROSS_FILL is the two-call form.  A FILL over any non-decreasing offsets writes
 * query k's ids only inside [dev_offsets[k], min(dev_offsets[k + 1], capacity)): offsets of another tree or of other
 * triangles truncate lists, they never make a write go astray.  RTBVH_CROSS_SORT's key is the 30-bit Morton code, in
 * the root box, of (qlo + qhi) * 0.5f, as RTBVH_OVERLAP_SORT's; one permutation serves both passes.
 * Everything else follows rtbvh_overlap_async one for one: the tree forms read, the waits, the place among the other
 * queries, the growing of the sort's buffers and the scan's block sums.  n == 0 returns RTBVH_OK and writes
 * dev_offsets[0] = 0 only if dev_offsets is non-NULL; RTBVH_ERR_NOT_READY before a build and after a vertex update
 * until the next build or refit; RTBVH_ERR_INVALID_ARG for NULL triangles or offsets with n > 0, NULL ids with
 * capacity > 0 outside RTBVH_CROSS_SIZES, bad mode bits, and n >= 2^31.
 * A walk that hits rtbvh_config.stack_limit loses that subtree's ids -- both passes lose the same ids, so offsets and
 * ids stay consistent -- and the next synchronising call returns RTBVH_ERR_STACK_OVERFLOW. */
rtbvh_status rtbvh_cross_async(rtbvh_ctx* ctx, const rtbvh_tri* dev_tris, uint64_t n, uint64_t* dev_offsets,
                               uint32_t* dev_ids, uint64_t capacity, uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream): offsets (n + 1) and ids are
 * host arrays; ids receives min(total, capacity) entries.  With RTBVH_CROSS_FILL, offsets is read. */
rtbvh_status rtbvh_cross_host(rtbvh_ctx* ctx, const rtbvh_tri* tris, uint64_t n, uint64_t* offsets, uint32_t* ids,
                              uint64_t capacity, uint32_t mode);
/* "Does it touch anything, and what first": dev_first[k] (n uint32, 4-B aligned) = the first id of query k's list
 * -- the member at the lowest sort position -- or 0xFFFFFFFF for an empty list.  One pass, no CSR; the walk of a
 * query ends at its first member.  Exactly the head of rtbvh_cross_async's list on every tree: a left-first
 * depth-first walk meets the leaves in ascending sort position, which the list order above already relies on.
 * mode: RTBVH_CROSS_SORT and RTBVH_CROSS_COUNT only.  n == 0 returns RTBVH_OK and touches nothing; NULL triangles
 * or dev_first with n > 0, other mode bits and n >= 2^31 are RTBVH_ERR_INVALID_ARG; RTBVH_ERR_NOT_READY as above.
 * A walk that hits rtbvh_config.stack_limit returns the head of the shortened list, and the next synchronising call
 * returns RTBVH_ERR_STACK_OVERFLOW. */
rtbvh_status rtbvh_cross_first_async(rtbvh_ctx* ctx, const rtbvh_tri* dev_tris, uint64_t n, uint32_t* dev_first,
                                     uint32_t mode, void* stream);
/* Host-memory wrapper of the above (synchronous, on the context stream): first receives n entries. */
rtbvh_status rtbvh_cross_first_host(rtbvh_ctx* ctx, const rtbvh_tri* tris, uint64_t n, uint32_t* first,
                                    uint32_t mode);
/* The last RTBVH_CROSS_COUNT query of either entry (waits for it): queries, ids (the true total, counted once; for
 * rtbvh_cross_first_* the queries with a member), internal-node steps and leaf steps summed over the passes the call
 * ran.  Its own words: the other queries' counts keep theirs.  RTBVH_ERR_NOT_READY before any counting triangle
 * query. */
rtbvh_status rtbvh_cross_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- clearance queries: the nearest scene triangle to a caller's triangle --------
 * (No reference equivalent; the distance query of FCL or PQP for a second mesh against the built one.)  For each
 * query triangle: which scene triangle is nearest, how far, and between which two points.  Specified operation for
 * operation, in fp32 without contraction, dots as (x*x' + y*y') + z*z', independently of the tree and of the walk: the
 * answer is the brute force over all scene triangles, byte for byte.
 * Inputs.  A query triangle q is an rtbvh_tri, reduced as in the triangle queries above to (qa, qe1, qe2, [qlo, qhi]);
 * a scene triangle x is its leaf record (a, e1, e2, [lo, hi]).  The vertices of a record are V0 = a, V1 = fl(a + e1),
 * V2 = fl(a + e2); its segments S0, S1, S2 are the self-collision section's.  One bound max_dist2 serves the call.
 * dist2(q, x) comes from fifteen candidate point pairs (cq, cx), in this order:
 *   0..2   cq = Vi(q);  cx = the closest-point section's q of triangle x for the point Vi(q): that section's formulas
 *          unchanged, its clamp into [lo, hi] included.
 *   3..5   cx = Vj(x);  cq = the same formulas of triangle q and its box [qlo, qhi] for the point Vj(x).
 *   6..14  the segment pairs (Si(q), Sj(x)), i major, (P1, D1) = Si(q), (P2, D2) = Sj(x); a division is the IEEE
 *          quotient and clamp01(x) = fminf(fmaxf(x, 0), 1), which makes 0 of a NaN:
 *              r = P1 - P2;  A = dot(D1,D1);  E = dot(D2,D2);  F = dot(D2,r);  C = dot(D1,r);  B = dot(D1,D2)
 *              den = A*E - B*B
 *              s = den > 0 ? clamp01((B*F - C*E) / den) : 0
 *              t = (B*s + F) / E
 *              if t < 0: s = clamp01(-C / A)   else if t > 1: s = clamp01((B - C) / A)
 *              t = clamp01(t)
 *              cq = P1 + D1*s;  cx = P2 + D2*t
 * Every candidate then gets, per component, cq = fmaxf(qlo, fminf(qhi, cq)) and cx = fmaxf(lo, fminf(hi, cx)), then
 * e = cq - cx and d = dot(e, e).  The pair's dist2 and its witness points (point_q, point_x) are those of the FIRST
 * candidate with the smallest d: a later one replaces an earlier one only if its d is strictly smaller, and a NaN d
 * never wins (all fifteen NaN: dist2 is a NaN).
 *  (X) If the triangle queries' (B) and (X) both hold for (q, x) -- x would be in q's rtbvh_cross list -- dist2 = +0.
 *      The witness points stay the winning candidate's: they are then the NEAREST FEATURE PAIR of two crossing
 *      triangles, not a contact point, and their own distance is not 0.
 * The result of q is the lexicographic minimum of (dist2, triangle id) over the triangles with dist2 <= max_dist2.
 * There is no result, and no walk, when !(max_dist2 >= 0) (a NaN included; -0 counts as +0) or when a vertex of q has
 * a non-finite component; nor is there one when no triangle is within the bound.
 * Every candidate is a pair of points of the two triangles, up to rounding, so dist2 never undershoots the true
 * distance by more than rounding; in exact arithmetic the minimum of the fifteen IS the distance of two triangles that
 * do not cross (it is attained at a vertex of one or between two edges).  Limits: those of (X) -- coplanar crossing
 * pairs are not seen by it and get their feature distance, which is then 0 up to rounding.
 * Pruning.  Let bb(q, box) = (dx*dx + dy*dy) + dz*dz with dk = fmaxf(fmaxf(lo_k - qhi_k, qlo_k - hi_k), 0).  Then
 * dist2(q, x) >= bb(q, any box that contains x's leaf box): the two clamps give cq_k >= qlo_k and cx_k <= hi_k, and
 * rounding is monotone, so fl(cq_k - cx_k) >= fl(qlo_k - hi_k), and the other sign likewise; squares and the
 * fixed-association sum of non-negative terms are monotone; under (B) every dk is 0, which covers (X).  So a walk
 * that enters a box iff bb <= the best dist2 so far (non-strict: ties are visited for the id tie-break) reaches every
 * triangle that can win, whatever order it visits in. */
typedef struct {
    float point_q[3]; /* on the query triangle, in its box */
    float dist2;
    float point_x[3]; /* on the scene triangle, in its leaf box */
    uint32_t tri;     /* triangle id (Node.index / 3) */
} rtbvh_clearance; /* 32 B.  No result: dist2 = -1, both points 0, tri = 0xFFFFFFFF */
enum {
    RTBVH_CLEARANCE_SORT = 1u << 1, /* walk the queries in the Morton order of their box centres (RTBVH_CROSS_SORT's
                                       keys): the same results, each at its query's own index */
    RTBVH_CLEARANCE_COUNT = 1u << 2 /* count queries, results and steps for rtbvh_clearance_counts (slower) */
    /* every other bit: RTBVH_ERR_INVALID_ARG */
};
/* n triangles at dev_tris and n results at dev_out (device memory of the context's device, 16-B aligned), enqueued on
 * `stream` (hipStream_t, NULL = the context stream).  Everything else follows rtbvh_cross_first_async and
 * rtbvh_nearest_async one for one: it reads the node records, or the topology plus node boxes, never the quantized
 * nodes; the call waits for the last build and only enqueues; the library orders it among all other queries, which
 * share the query scratch, and the next build waits for it.  n == 0 returns RTBVH_OK and touches nothing;
 * RTBVH_ERR_NOT_READY before a build and after a vertex update until the next build or refit;
 * RTBVH_ERR_INVALID_ARG for NULL pointers with n > 0, unknown mode bits and n >= 2^31.
 * A walk that hits rtbvh_config.stack_limit ends with the best found so far -- a genuine (dist2, triangle) pair, not
 * necessarily the nearest -- and the next synchronising call returns RTBVH_ERR_STACK_OVERFLOW. */
rtbvh_status rtbvh_clearance_async(rtbvh_ctx* ctx, const rtbvh_tri* dev_tris, uint64_t n, float max_dist2,
                                   rtbvh_clearance* dev_out, uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream). */
rtbvh_status rtbvh_clearance_host(rtbvh_ctx* ctx, const rtbvh_tri* tris, uint64_t n, float max_dist2,
                                  rtbvh_clearance* out, uint32_t mode);
/* The last RTBVH_CLEARANCE_COUNT query (waits for it): queries, results found, internal-node steps, leaf steps.  Its
 * own words: the other queries' counts keep theirs.  RTBVH_ERR_NOT_READY before any counting clearance query. */
rtbvh_status rtbvh_clearance_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- sphere-sweep queries: the first contact of a moving sphere ---------------------------------
 * (No reference equivalent; the sweep of the raycast / overlap / sweep triad of collision queries.)  A sphere of
 * radius r starts with its centre at c and moves along d: centre(t) = c + t * d.  The query asks for the first t in
 * [0, t_max] at which it touches the mesh, where, and on which feature.  c, d and r live in the space the BVH was
 * built in, as the rays'; d need not be unit, and r is a distance of that space (an object-space distance only under
 * an identity WVP, as for the closest-point queries).
 * Specified operation for operation, in fp32 without contraction, dots as (x*x' + y*y') + z*z', cross as in the
 * self-collision section, `/` and sqrtf the IEEE (correctly rounded) results, independently of the tree and of the
 * walk: the answer is the brute force over all scene triangles, byte for byte.
 * A scene triangle x is its leaf record (a, e1, e2, [lo, hi]); V0 = a, V1 = fl(a + e1), V2 = fl(a + e2) and the
 * segments S0 = (a, e1), S1 = (a, e2), S2 = (V1, fl(e2 - e1)) are the clearance and self-collision sections'.
 * For a sweep (c, d, r, t_max) let dd = dot(d, d) and inv = 1 / d per component.
 * There is no walk and no result for: a non-finite component of c or d; d all zero; !(r >= 0) or r infinite;
 * !(t_max >= 0) (NaN included).  -0 counts as +0 for r and t_max; t_max = +inf: no limit.
 *  (B) The leaf box grown by r, [fl(lo - r), fl(hi + r)] per component, passes the all-hits box rule with t_max: with
 *      t0 = (fl(lo - r) - c) * inv, t1 = (fl(hi + r) - c) * inv per axis and mn, mx as in that section's (B), the box
 *      passes iff 0 <= mx && mn <= mx && !(mn > t_max).  mn_x is that mn.
 *  (T) The pair's t, point and feature:
 *      1. Start overlap.  dist2 and q of the closest-point section for the point c (its clamp into [lo, hi] included).
 *         If dist2 <= r*r: t = +0, point = q, feature = 1, and nothing else is tried.
 *      2. Otherwise the first smallest of up to seven candidates, in the order face, S0, S1, S2, V0, V1, V2.  A
 *         candidate counts only if every "needs" below holds and 0 <= t && t <= t_max; a NaN fails each comparison
 *         as written; a later candidate replaces an earlier one only if its t is strictly smaller.
 *         Face (feature 2):
 *             n = cross(e1, e2);  nn = dot(n, n);                       needs nn > 0
 *             s = dot(n, c - a);  if s < 0: n = -n, s = -s
 *             ln = sqrtf(nn);  h = s - r*ln;  dn = dot(n, d);           needs dn < 0 && h >= 0
 *             t = h / (-dn);  p = (c + d*t) - n*(r/ln);  ap = p - a
 *             d1 = dot(e1, ap);  d2 = dot(e2, ap);  e11 = dot(e1, e1);  e12 = dot(e1, e2);  e22 = dot(e2, e2)
 *             den = e11*e22 - e12*e12;  u = (e22*d1 - e12*d2) / den;  v = (e11*d2 - e12*d1) / den
 *                                                                       needs u >= 0 && v >= 0 && u + v <= 1
 *             point = p
 *         Edge (A, E) = Si (feature 3 + i):
 *             m = c - A;  ee = dot(E, E);  md = dot(m, E);  nd = dot(d, E);  mm = dot(m, m);  mdd = dot(m, d)
 *             a_ = ee*dd - nd*nd;  k = mm - r*r;  c_ = ee*k - md*md;  b_ = ee*mdd - nd*md
 *                                                                       needs a_ > 0 && c_ > 0 && b_ < 0
 *             disc = b_*b_ - a_*c_;                                     needs disc >= 0
 *             t = c_ / (sqrtf(disc) - b_)        (the root without cancellation)
 *             s_ = md + t*nd;                                           needs 0 <= s_ && s_ <= ee
 *             point = A + E*(s_/ee)
 *         Vertex V = Vi (feature 6 + i):
 *             m = c - V;  b = dot(m, d);  cc = dot(m, m) - r*r;         needs cc > 0 && b < 0
 *             disc = b*b - dd*cc;                                       needs disc >= 0
 *             t = cc / (sqrtf(disc) - b);  point = V
 *      Every reported point is then clamped per component, point = fmaxf(lo, fminf(hi, point)), as the closest-point
 *      section's q.
 * x is a MEMBER of the sweep iff (B) holds and (T) yields a t.  Its key is tk_x = fmaxf(t_x, mn_x) + 0 (fmaxf drops a
 * NaN; the + 0 makes +0 of a -0, which h = -0 can give at r = 0): 0 <= tk_x <= t_max, so its bits order as the floats.
 * The result is the member with the smallest (tk bits, triangle id), reported with its genuine t, point and feature,
 * never with tk: khits at k = 1 with another leaf test.  The box is in the key for khits' reason: t_x can be a few
 * ulps below mn_x, and only a key that no box around x undershoots can be walked with pruning.
 * In exact arithmetic the smallest candidate IS the first contact: each candidate is a moment the centre is exactly
 * r from a point of the triangle's plane, of an edge's line or of a vertex, kept only where that point lies on the
 * triangle; the first such moment touches the face's interior, an edge's interior or a vertex.  r = 0 is allowed: a
 * thin ray by these formulas (no EPSILON; a triangle is hit from either side); no equality with rtbvh_query_*'s bits
 * is promised.  Limits: a contact within rounding of two features reports either, the same on every tree; the clamped
 * key orders contacts whose t differ by rounding by their leaf boxes' entries, as khits does.
 * Exactness.  Rounding is monotone, so the grown boxes nest as the boxes do; the slab test is monotone in the box, so
 * every tree box B around x, grown, passes the first two slab conditions when x's grown leaf box does, and starts at
 * mn(B) <= mn_x <= tk_x.  The walk enters a box, grown by r, iff 0 <= mx && mn <= mx && !(mn > bound), bound = t_max
 * until a member is found, then the best tk (non-strict: ties are visited for the id tie-break).  A leaf's own box is
 * tested by (B) as written.  A child's box is tested without the axes whose inv is infinite: there 0 * inf = NaN
 * drops a face at exactly c_k, so a flat grown leaf box passes (B) while a box around it fails -- the one case where
 * the slab test is not monotone (the all-hits queries' exception, where the ray test never accepts such a triangle;
 * a sphere does touch it, through its edges).  Without those axes the test is monotone, enters every box (B) enters,
 * and its mn is not above (B)'s; with no axis left (|d_k| <= 2^-128 on all three) every child is entered.  So visiting order, tree form, refit or rebuild and RTBVH_SWEEP_SORT cannot change a
 * byte. */
/* A sweep, 32 B (two 16-B words): rtbvh_ray's layout with the reserved word as the radius. */
typedef struct {
    float origin[3];
    float t_max;
    float direction[3];
    float radius;
} rtbvh_sweep;
/* A result, 32 B (two 16-B words): t of first contact (centre = origin + t * direction), the contact point on the
 * triangle (in its leaf box), the triangle's id in triangle order, and the feature touched: 1 the sphere overlaps the
 * triangle at t = 0 (point: the closest point to the origin), 2 the face, 3..5 the edge segment S0..S2, 6..8 the
 * vertex V0..V2.  A miss: t = -1, point = 0, tri = 0xFFFFFFFF, feature = 0.  reserved = 0 always. */
typedef struct {
    float t;
    float point[3];
    uint32_t tri;
    uint32_t feature;
    uint32_t reserved[2];
} rtbvh_sweep_hit;
enum {
    RTBVH_SWEEP_ANY = 1u << 0,   /* does it touch anything within t_max: the walk ends at the first member, whose own
                                    record {t, point, tri, feature} is the result (which member is unspecified).
                                    Whether a sweep hits equals the default mode's answer */
    RTBVH_SWEEP_SORT = 1u << 1,  /* walk the sweeps in RTBVH_QUERY_SORT's order of (direction octant, origin Morton):
                                    same results, each at its sweep's own index */
    RTBVH_SWEEP_COUNT = 1u << 2  /* count sweeps, hits and steps for rtbvh_sweep_counts (slower) */
    /* (every other bit is rejected) */
};
/* n sweeps at dev_sweeps and n results at dev_hits (device memory of the context's device, 16-B aligned), result k for
 * sweep k, enqueued on `stream` (hipStream_t, NULL = the context stream).  The rules of rtbvh_nearest_async hold one
 * for one: the walk reads the tree the last build or refit wrote (node records, or the topology and node boxes; never
 * the quantized nodes); the call waits for the last build and only enqueues; the library orders it among all the other
 * queries, which share the query scratch, and the next build waits for it; the first RTBVH_SWEEP_SORT query and each
 * larger one grow the sort's buffers (shared with the other queries' SORT), which waits on the host.
 * n == 0 returns RTBVH_OK and touches nothing; RTBVH_ERR_NOT_READY before a build and after a vertex update until
 * the next build or refit; RTBVH_ERR_INVALID_ARG for NULL pointers with n > 0, unknown mode bits, and n >= 2^31.
 * A walk that hits rtbvh_config.stack_limit ends with the best found so far -- a genuine member's record, its key not
 * below the true best -- and the next synchronising call returns RTBVH_ERR_STACK_OVERFLOW. */
rtbvh_status rtbvh_sweep_async(rtbvh_ctx* ctx, const rtbvh_sweep* dev_sweeps, uint64_t n, rtbvh_sweep_hit* dev_hits,
                               uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream). */
rtbvh_status rtbvh_sweep_host(rtbvh_ctx* ctx, const rtbvh_sweep* sweeps, uint64_t n, rtbvh_sweep_hit* hits,
                              uint32_t mode);
/* The last RTBVH_SWEEP_COUNT query (waits for it): sweeps, hits, internal-node steps, leaf steps.  Its own words: the
 * other queries' counts keep theirs.  RTBVH_ERR_NOT_READY before any counting sweep query. */
rtbvh_status rtbvh_sweep_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- box-overlap queries: every triangle that meets an axis-aligned box the caller chose --------
 * (No reference equivalent.)  The boxes live in the space the BVH was built in, as the other queries' inputs.  The
 * result of box k is the list of the ids (in triangle order, Node.index / 3) of exactly the triangles that are
 * members of it.  Membership is defined on the floats of the triangle's leaf record -- a = p0, e1 = fl(p1 - p0),
 * e2 = fl(p2 - p0) and the leaf box [lo, hi] -- independently of the tree and of the walk; arithmetic is fp32
 * without contraction.  Triangle x is a member of the query box [qlo, qhi] iff
 *  (B) on every axis k: qlo_k <= hi_k && lo_k <= qhi_k.  The intervals are closed: touching counts.  There is no
 *      arithmetic, so no rounding; a NaN in a leaf box fails it.
 *  (T) with RTBVH_OVERLAP_TRIANGLE only: none of the ten axes below separates the triangle from the box (the three
 *      box-face axes are (B)).  In every `separated` comparison a NaN compares false: it does not separate.
 *      Set-up, per component: c = (qlo + qhi) * 0.5f, h = (qhi - qlo) * 0.5f; v0 = a - c, v1 = v0 + e1, v2 = v0 + e2.
 *      Plane: n = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x);
 *             d = (n.x*v0.x + n.y*v0.y) + n.z*v0.z;  r = (h.x*|n.x| + h.y*|n.y|) + h.z*|n.z|;
 *             separated iff d > r || d < -r.
 *      Edges: for each edge f of e1, fl(e2 - e1), e2, in that order, and each of three axes, the projections p_i of
 *             v0, v1, v2 and a radius rr:
 *               x: p_i = v_i.z*f.y - v_i.y*f.z,  rr = h.y*|f.z| + h.z*|f.y|;
 *               y: p_i = v_i.x*f.z - v_i.z*f.x,  rr = h.x*|f.z| + h.z*|f.x|;
 *               z: p_i = v_i.y*f.x - v_i.x*f.y,  rr = h.x*|f.y| + h.y*|f.x|;
 *             separated iff fminf(fminf(p0, p1), p2) > rr || fmaxf(fmaxf(p0, p1), p2) < -rr.
 *      (T) is the usual separating-axis test evaluated in fp32 with no error margins: a contact within rounding
 *      can go either way, as with rayTriangleCollision's EPSILON.  It is the same answer on every tree.
 * The list is empty, and there is no walk, for a box with a non-finite bound or with !(qlo_k <= qhi_k) on any axis.
 * A point box (qlo == qhi) and a flat box are valid; -0 and +0 bounds behave alike.  The set is exact, whatever the
 * tree: (B) is monotone in the tree's box, so a walk that enters a child iff its box passes (B) reaches every member
 * (DESIGN.md 5g).
 * Order within a box's list: ascending by the triangle's position in the last build's sort order (tri_ids of
 * rtbvh_read_sorted; a refit keeps it), as rtbvh_within_async's lists: reproducible down to the byte.
 * Output in CSR form: dev_offsets[0] = 0, box k's ids are dev_ids[dev_offsets[k] .. dev_offsets[k + 1]), and
 * dev_offsets[n] is the true total whatever `capacity` is.  An id whose index is >= capacity is not written:
 * nothing is ever written past dev_ids + capacity, capacity may be 0 (dev_ids may then be NULL), and the caller
 * compares dev_offsets[n] with capacity. */
typedef struct {
    float lo[3];
    uint32_t reserved0; /* ignored */
    float hi[3];
    uint32_t reserved1; /* ignored */
} rtbvh_box; /* 32 B: two 16-B words */
enum {
    RTBVH_OVERLAP_SORT = 1u << 1,     /* walk the boxes in the Morton order of their centres: same output */
    RTBVH_OVERLAP_COUNT = 1u << 2,    /* count boxes, ids and steps for rtbvh_overlap_counts (slower) */
    RTBVH_OVERLAP_TRIANGLE = 1u << 3, /* members must also pass the triangle-box test (T) above */
    RTBVH_OVERLAP_SIZES = 1u << 4,    /* write dev_offsets only; dev_ids may be NULL */
    RTBVH_OVERLAP_FILL = 1u << 5      /* dev_offsets is INPUT (from a SIZES call for the same boxes, tree and
                                         TRIANGLE bit): write the ids only */
    /* SIZES | FILL together and every other bit: RTBVH_ERR_INVALID_ARG */
};
/* n boxes at dev_boxes (16-B aligned), n + 1 offsets at dev_offsets (8-B aligned) and room for `capacity` ids at
 * dev_ids (device memory of the context's device), enqueued on `stream` (hipStream_t, NULL = the context stream).
 * Mode 0 runs the sizes pass, a scan of the offsets on the device and the fill pass in one call, with no host round
 * trip; RTBVH_OVERLAP_SIZES then RTBVH_OVERLAP_FILL is the two-call form for a caller who sizes dev_ids from
 * dev_offsets[n].  A FILL over any non-decreasing offsets writes box k's ids only inside
 * [dev_offsets[k], min(dev_offsets[k + 1], capacity)): offsets of another tree or of other boxes truncate lists, they
 * never make a write go astray.  RTBVH_OVERLAP_SORT's key is the 30-bit Morton code, in the root box, of the box's
 * centre (lo + hi) * 0.5f, as RTBVH_NEAREST_SORT's of its point; one permutation serves both passes.
 * Everything else follows rtbvh_within_async one for one: the walk reads the tree the last build or refit wrote
 * (node records, or the topology and node boxes; never the quantized nodes); the call waits for the last build and
 * only enqueues; the library orders it among all the other queries, and the next build waits for it.  The first
 * RTBVH_OVERLAP_SORT query and each larger one grow the sort's buffers, and the first query that writes offsets and
 * each larger one grow the scan's block sums: growing waits on the host for the outstanding queries.
 * n == 0 returns RTBVH_OK and writes dev_offsets[0] = 0 only if dev_offsets is non-NULL; RTBVH_ERR_NOT_READY before
 * a build and after a vertex update until the next build or refit; RTBVH_ERR_INVALID_ARG for NULL boxes or offsets
 * with n > 0, NULL ids with capacity > 0 outside RTBVH_OVERLAP_SIZES, bad mode bits, and n >= 2^31.
 * A walk that hits rtbvh_config.stack_limit loses that subtree's ids -- both passes lose them identically, so
 * offsets and ids stay consistent -- and the next synchronising call returns RTBVH_ERR_STACK_OVERFLOW. */
rtbvh_status rtbvh_overlap_async(rtbvh_ctx* ctx, const rtbvh_box* dev_boxes, uint64_t n, uint64_t* dev_offsets,
                                 uint32_t* dev_ids, uint64_t capacity, uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream): offsets (n + 1) and ids are
 * host arrays; ids receives min(total, capacity) entries.  With RTBVH_OVERLAP_FILL, offsets is read. */
rtbvh_status rtbvh_overlap_host(rtbvh_ctx* ctx, const rtbvh_box* boxes, uint64_t n, uint64_t* offsets,
                                uint32_t* ids, uint64_t capacity, uint32_t mode);
/* The last RTBVH_OVERLAP_COUNT query (waits for it): boxes, ids (the true total, counted once), internal-node
 * steps and leaf steps summed over the passes the call ran.  Its own words: the other queries' counts keep theirs.
 * RTBVH_ERR_NOT_READY before any counting box query. */
rtbvh_status rtbvh_overlap_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- region queries: every triangle within up to six planes the caller chose -----------------------
 * (No reference equivalent.)  A region is the intersection of up to six half-spaces: a frustum, an oriented box, a
 * single half-space (a clip or section plane), a slab between two parallel planes -- a slab of zero thickness
 * lists the triangles one layer of a slicer cuts.  The planes live in the space the BVH was built in, as the other
 * queries' inputs.  Plane i is {nx, ny, nz, d}; point x is on its inner side when n.x + d <= 0.  An unused plane is
 * all zeros: its value is +0 everywhere, so it holds everywhere and there is no count field.
 * The value of plane P = {n, d} at x, fp32 without contraction:
 *     t_k = (n_k == 0) ? +0 : fl(n_k * x_k)   for k = x, y, z  (a zero component is skipped: 0 * inf makes no NaN)
 *     s(P, x) = fl(fl(fl(t_x + t_y) + t_z) + d)
 * For a box [lo, hi] the near corner takes lo_k where n_k >= 0 and hi_k elsewhere, and m(P, box) is s there; the far
 * corner is the opposite choice, and M(P, box) is s there.
 * Membership is defined on the floats of the triangle's leaf record -- a = p0, e1 = fl(p1 - p0), e2 = fl(p2 - p0)
 * and the leaf box [lo, hi] -- independently of the tree and of the walk.  Triangle x is a member of the region iff
 *  (B) for every plane i: m(P_i, leaf box) <= 0.  A NaN fails it.
 *  (V) with RTBVH_REGION_TRIANGLE only: with v0 = a, v1 = clamp(fl(a + e1)), v2 = clamp(fl(a + e2)), where
 *      clamp(q)_k = fmaxf(lo_k, fminf(hi_k, q_k)) (the clearance queries' clamping into the triangle's own box), for
 *      every plane i: s(P_i, v0) <= 0 || s(P_i, v1) <= 0 || s(P_i, v2) <= 0.
 *      (V) is the usual conservative frustum test on the vertices: no single plane has all three vertices outside.
 *      It is NOT an exact triangle-polytope intersection -- a triangle outside the region near an edge or a corner
 *      of it can pass -- but for the slab {n, d}, {-n, -d} it is exact: some vertex on each side.
 * The list is empty, and there is no walk, for a region with a non-finite float among its 24.
 * The set is exact, whatever the tree: rounded products and sums are monotone, so for nested boxes and a vertex
 * inside them m(node) <= m(leaf) <= s(v) <= M(leaf) <= M(node); a walk that enters a child iff m <= 0 on every plane
 * reaches every member, and a subtree whose box has M <= 0 on every plane holds members only and is taken whole --
 * its leaves are one run of the sort order -- while no leaf box of the tree holds a NaN.  The cost
 * follows the region's boundary, not its contents.
 * Order, output (CSR: dev_offsets, dev_ids) and `capacity` are rtbvh_overlap_async's, word for word: each list
 * ascends by the member's position in the last build's sort order, dev_offsets[n] is the true total, and nothing is
 * ever written past dev_ids + capacity. */
typedef struct rtbvh_region {
    float plane[6][4]; /* plane i: {nx, ny, nz, d} */
} rtbvh_region;        /* 96 B: six 16-B words */
enum {
    RTBVH_REGION_COUNT = 1u << 2,    /* count regions, ids, steps and accepts for rtbvh_region_counts (slower) */
    RTBVH_REGION_TRIANGLE = 1u << 3, /* members must also pass the vertex test (V) above */
    RTBVH_REGION_SIZES = 1u << 4,    /* write dev_offsets only; dev_ids may be NULL */
    RTBVH_REGION_FILL = 1u << 5,     /* dev_offsets is INPUT (from a SIZES call for the same regions, tree and
                                        TRIANGLE bit): write the ids only */
    RTBVH_REGION_NO_ACCEPT = 1u << 6, /* never take a subtree whole: descend to every leaf.  The same bytes; for
                                         A/B runs and tests */
    /* Bits 16..19: the split field (below).  0: one lane walks one region. */
    RTBVH_REGION_SPLIT_SHIFT = 16,
    RTBVH_REGION_SPLIT_AUTO = 15u << 16
    /* SIZES | FILL together, the split field values 13 and 14 and every other bit: RTBVH_ERR_INVALID_ARG.  There is
       no SORT mode: a region has no centre. */
};
/* The split field: the same lists from many lanes, for few and large regions (one frustum, a slicer's layers).
 * A value v = 1..12 at bits 16..19 of `mode` (v << RTBVH_REGION_SPLIT_SHIFT) cuts each region into at most K = 2^v
 * pieces; RTBVH_REGION_SPLIT_AUTO (v = 15) takes K = 4096.  Either way K is then halved until
 * n * K <= RTBVH_REGION_SPLIT_MAX_PIECES, so the field is an upper limit, and K = 1 (many regions) is the plain path.
 * A piece is a subtree of the BVH: one run of the sort order.  The library expands each region's frontier from the
 * root, in order and on the device -- a node is replaced by those of its two children the region enters, a child the
 * region holds whole becomes a finished range -- until K pieces are reached, then walks one piece a lane and lays the
 * pieces' lists end to end.  The offsets, the ids and their order, `capacity`, the FILL rule above, the NaN word and
 * its ordering, both tree forms, n == 0 and every error are those of the plain query, byte for byte; SIZES and FILL
 * pair up with or without the field in all four ways.  A FILL call with the field computes the pieces and their
 * sizes again, into the context's buffers, and fills against the caller's offsets.
 * The context owns the piece buffers (16 B a piece slot, n * K slots): the first query with a field and each larger one waits on
 * the host for the outstanding queries and allocates, as RTBVH_QUERY_SORT's buffers do.
 * Stack limit: a piece's walk starts at its own node with an empty stack, so under rtbvh_config.stack_limit a split
 * query may lose FEWER subtrees than the plain one.  Its lists are then subsequences of the true lists, both passes
 * of a call lose the same subtrees, and RTBVH_ERR_STACK_OVERFLOW is reported as above.  Without an overflow the bytes
 * are the plain query's. */
#define RTBVH_REGION_SPLIT_MAX_PIECES (1u << 20)
/* n regions at dev_regions (16-B aligned), n + 1 offsets at dev_offsets (8-B aligned) and room for `capacity` ids at
 * dev_ids (device memory of the context's device), enqueued on `stream` (hipStream_t, NULL = the context stream).
 * Mode 0 runs the sizes pass, a scan of the offsets on the device and the fill pass in one call, with no host round
 * trip; RTBVH_REGION_SIZES then RTBVH_REGION_FILL is the two-call form.  A FILL over any non-decreasing offsets
 * writes region k's ids only inside [dev_offsets[k], min(dev_offsets[k + 1], capacity)), whether an id comes from a
 * leaf or from a subtree taken whole: foreign offsets truncate lists, they never make a write go astray.
 * The first region query after a build or a refit runs one pass over the leaf records on its stream (is there a
 * NaN in a leaf box?); the region queries of that tree on other streams are ordered behind it on the device.
 * Everything else follows rtbvh_overlap_async one for one: the tree forms read (and the topology's leaf ranges in
 * both), the waits, the place among the other queries, growing the scan's block sums, n == 0, the errors
 * (RTBVH_ERR_NOT_READY before a build and after a vertex update; RTBVH_ERR_INVALID_ARG for NULL regions or offsets
 * with n > 0, NULL ids with capacity > 0 outside RTBVH_REGION_SIZES, bad mode bits, n >= 2^31) and the stack limit:
 * a walk that hits rtbvh_config.stack_limit loses that subtree's ids, both passes alike, and the next synchronising
 * call returns RTBVH_ERR_STACK_OVERFLOW. */
rtbvh_status rtbvh_region_async(rtbvh_ctx* ctx, const rtbvh_region* dev_regions, uint64_t n, uint64_t* dev_offsets,
                                uint32_t* dev_ids, uint64_t capacity, uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream): offsets (n + 1) and ids are
 * host arrays; ids receives min(total, capacity) entries.  With RTBVH_REGION_FILL, offsets is read. */
rtbvh_status rtbvh_region_host(rtbvh_ctx* ctx, const rtbvh_region* regions, uint64_t n, uint64_t* offsets,
                               uint32_t* ids, uint64_t capacity, uint32_t mode);
/* The last RTBVH_REGION_COUNT query (waits for it): regions, ids (the true total, counted once), internal-node steps,
 * leaf steps, subtrees taken whole (these three summed over the passes the call ran) and the ids that came from
 * them (counted once).  Its own words.  RTBVH_ERR_NOT_READY before any counting region query. */
rtbvh_status rtbvh_region_counts(rtbvh_ctx* ctx, uint64_t out[6]);
/* With a split field, rtbvh_region_counts counts regions (not pieces) and ids once; the internal-node steps include
 * the expansion's node tests (made once a call, where the plain query makes them once a pass), and the subtrees
 * taken whole include the ranges the expansion finished.
 * The last RTBVH_REGION_COUNT query that had a split field (waits for it): out[0] the K used (1: the plain path ran,
 * the other words are 0), out[1] the non-empty pieces, out[2] the node tests the expansion made, out[3] the longest
 * single piece walk in node + leaf steps.  RTBVH_ERR_NOT_READY before any such query. */
rtbvh_status rtbvh_region_split_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- signed-distance queries: the nearest triangle, and on which side of the surface the point is ----
 * (No reference equivalent.)  Same points (rtbvh_point: {point.xyz, max_dist2}) and the same space as the
 * closest-point queries above.  For each point: rtbvh_nearest's fields, and the number of triangles crossed by one
 * or three fixed rays that start at the point -- for a closed surface, an odd count means inside.
 *
 * Rays: ray j starts at the point p; its direction is a constant, exactly representable, with no zero component, so
 * inv = 1 / d is finite:
 *     D0 = ( 0.75,    0.5,   0.4375)
 *     D1 = (-0.5,     0.75, -0.4375)
 *     D2 = ( 0.4375, -0.5,  -0.75)
 * and t_max = +inf.
 * Crossing: triangle x is crossed by ray j iff (B) and (X) hold, both evaluated on the floats of its leaf record --
 * p0, e1 = fl(p1 - p0), e2 = fl(p2 - p0) and the leaf box [lo, hi] -- in fp32 without contraction, dots as
 * (x*x' + y*y') + z*z':
 *   (B) the leaf box passes the any-hit box rule of the all-hits section with t_max = +inf:
 *       0 <= mx && mn <= mx && !(mn > t_max);
 *   (X) rayTriangleCollision's arithmetic in its operation order, without its division and its EPSILON:
 *       tmp = cross(d, e2);  det = dot(e1, tmp);  rt = p - p0
 *       U = dot(rt, tmp);  tmp2 = cross(rt, e1);  V = dot(d, tmp2);  N = dot(e2, tmp2)
 *       if det < 0: negate det, U, V and N (exact)
 *       crossed iff det > 0 && U >= 0 && V >= 0 && U + V <= det && N > 0.
 * A NaN makes a comparison false: the triangle is not crossed.  There is no epsilon anywhere, so scaling the mesh and
 * the points by a power of two changes no decision (short of overflow and underflow).
 * The counts are exact, whatever the tree: (B) is monotone in the box, so a walk that enters a child
 * iff its box passes the rule reaches every crossed triangle.  A one-triangle tree has no parent that
 * tests the leaf's box: it is tested at the leaf.
 *
 * flags, with c_j the number of triangles ray j crosses, over all triangles (0 for a ray not cast):
 *     bit 0        inside: c_0 odd, or with RTBVH_SIGNED_VOTE3 at least two of the three c_j odd
 *     bits 1..3    c_j & 1 for j = 0..2 (the parity of the true count, not of the saturated byte)
 *     bits 4..7    0
 *     bits 8..15, 16..23, 24..31    min(c_j, 255) for j = 0, 1, 2
 * The nearest fields are exactly what rtbvh_nearest_* returns for the same point and bound: the lexicographic minimum
 * of (dist2, tri), the same bits; "no result" is dist2 = -1, point = u = v = 0, tri = 0xFFFFFFFF.
 * No walk: a non-finite coordinate gives no rays and no closest-point walk -- the "no result" fields and flags = 0.
 * !(max_dist2 >= 0) (NaN included), or RTBVH_SIGNED_INSIDE_ONLY, gives the "no result" nearest fields, and the rays
 * are still cast: a bound makes a narrow band, max_dist2 = -1 an occupancy query.  -0 counts as +0. */
typedef struct {
    float point[3]; float dist2;      /* rtbvh_nearest's fields, the same bits */
    float u, v; uint32_t tri;
    uint32_t flags;                   /* see above */
} rtbvh_signed;
enum { RTBVH_SIGNED_SORT = 1u << 1, RTBVH_SIGNED_COUNT = 1u << 2,
       RTBVH_SIGNED_VOTE3 = 1u << 3,        /* three rays, majority; default: ray 0 alone */
       RTBVH_SIGNED_INSIDE_ONLY = 1u << 4   /* no closest-point walk: the nearest fields are "no result" */
       /* (every other bit is rejected) */ };
/* n points at dev_points and n records at dev_out (device memory of the context's device, 16-B aligned), record k
 * for point k, enqueued on `stream` (hipStream_t, NULL = the context stream).  Status, ordering, the sharing of the
 * query scratch and of the sort's buffers (RTBVH_SIGNED_SORT: the order of RTBVH_NEAREST_SORT, the same output),
 * n == 0, n >= 2^31, NULL pointers and unknown mode bits are rtbvh_nearest_async's rules, one for one.
 * A walk that hits rtbvh_config.stack_limit may lose crossings, and the next synchronising call returns
 * RTBVH_ERR_STACK_OVERFLOW; the nearest fields keep rtbvh_nearest's guarantee (the best found so far). */
rtbvh_status rtbvh_signed_async(rtbvh_ctx* ctx, const rtbvh_point* dev_points, uint64_t n, rtbvh_signed* dev_out,
                                uint32_t mode, void* stream);
/* Host-memory convenience wrapper of the above (synchronous, on the context stream). */
rtbvh_status rtbvh_signed_host(rtbvh_ctx* ctx, const rtbvh_point* points, uint64_t n, rtbvh_signed* out,
                               uint32_t mode);
/* The last RTBVH_SIGNED_COUNT query (waits for it): points, points inside, internal-node steps and leaf steps summed
 * over all its walks.  Its own words: the other queries' counts keep theirs.  RTBVH_ERR_NOT_READY before any
 * counting signed-distance query. */
rtbvh_status rtbvh_signed_counts(rtbvh_ctx* ctx, uint64_t out[4]);

/* ---- outputs --------------------------------------------------------------- */
/* reflectRay[].color, the framebuffer of record (RayTraceBVHPS.hlsl:13-16): W*H*4 floats, row y at y*W. */
rtbvh_status rtbvh_read_framebuffer(rtbvh_ctx* ctx, float* rgba);
/* Final reflectRay[].intensity per pixel (W*H floats). */
rtbvh_status rtbvh_read_intensity(rtbvh_ctx* ctx, float* intensity);
/* What the presentation pass shows (RayTraceBVHPS.hlsl:13-16 into the R8G8B8A8_UNORM swap
 * chain, Graphics.cpp:163): screen row y (top = 0) is framebuffer row H-1-y (the shader's
 * index at pixel centres), each channel floor(saturate(c) * 255 + 0.5).  W*H*4 bytes, of
 * the last full-frame trace (not of a band trace). */
rtbvh_status rtbvh_present(rtbvh_ctx* ctx, uint8_t* rgba8);
/* SaveBMP (SaveBMP.cpp:3-62): 24-bit BI_RGB file, 0x0ec4 pixels per metre, rows bottom-up;
 * `rgba8` is a presented image (top row first).  Rows are padded to 4 bytes as BMP
 * requires (the reference writes them unpadded; identical when 3*W is a multiple of 4). */
rtbvh_status rtbvh_save_bmp(const char* path, const uint8_t* rgba8, uint32_t width, uint32_t height);
/* Device pointer of the W*H*4-float framebuffer (valid until the next trace/destroy). */
const float* rtbvh_framebuffer_device(rtbvh_ctx* ctx);
/* BVHTree UAV u0 in the reference layout (2n-1 nodes, see rtbvh_node). */
rtbvh_status rtbvh_read_bvh(rtbvh_ctx* ctx, rtbvh_node* out, uint32_t capacity);
/* Node records in slots (the layout every traversal walk reads): 2(n-1) records of 16 u32;
 * record 2p+side belongs to c = child `side` of internal node p and holds the boxes of
 * c's children L and R as words {L.min.x, L.min.y, L.max.x, L.max.y, R.min.x, R.min.y,
 * R.max.x, R.max.y, L.min.z, L.max.z, R.min.z, R.max.z, id_L, id_R, c, 0}; ids: internal k,
 * or 0x80000000|j for sorted leaf j.  A leaf child c holds {its box as L and as R,
 * 0x80000000|c, ~0u, 0x80000000|c, 0}.  (The root's record follows at slot 2(n-1).)  Only the
 * packet primary walks read the leaf children's records: a build for other walks (binned, AUTO)
 * leaves them out, and the first packet walk or this call writes them. */
rtbvh_status rtbvh_read_wide(rtbvh_ctx* ctx, uint32_t* records, uint64_t capacity);
/* Quantized 4-wide nodes of the bounce walk, one 64-B record (16 words) per slot (2n-1):
 * internal node k's at the slot of its record (2 * parent + side; the root's at 2n-2;
 * slots of leaves unused): words 0-2 grid origin xyz, 3-5 grid step xyz (f32; step x ==
 * 0: not quantized), 6-8 lo bytes x/y/z, 9-11 hi bytes x/y/z (byte c = grandchild c),
 * 12-15 grandchildren (slot, 0x80000000 | leaf, or 0xFFFFFFFF); decoded corner = origin +
 * q * step.  The low 16 bits of words 4 and 5 carry the certified walk's margin codes (the
 * largest edge bound of the node's leaves and its margin range, as the high half of an f32):
 * mask them off (& 0xFF800000) to read the steps.  Only the QNodes the walk reads are
 * written -- the root's and, recursively, those of the internal grandchildren listed in words
 * 12-15 (a build of more than 2048 triangles leaves the others untouched); capacity in records
 * (>= 2n-1). */
rtbvh_status rtbvh_read_qnodes(rtbvh_ctx* ctx, uint32_t* nodes, uint64_t capacity);
/* The walk-only tree's quantized nodes, in rtbvh_read_qnodes' format (every internal node's is written): a second
 * tree over the same sorted leaves -- the built tree's top, every maximal subtree of <= 512 leaves rebuilt by binned
 * SAH -- that the certified 4-wide bounce walk reads from the third trace of a build on (environment
 * RTBVH_WALK_TREE at rtbvh_create: 0 never, 1 from the first).  Nothing else reads it: queries, the other walks
 * and every other read-back keep the built tree.  RTBVH_ERR_NOT_READY when the context holds none for the
 * current build (rtbvh_stats.walk_tree_builds counts them). */
rtbvh_status rtbvh_read_walk_qnodes(rtbvh_ctx* ctx, uint32_t* nodes, uint64_t capacity);
/* Per-triangle Morton codes in triangle order (MortonCodes.hlsl:104-112). */
rtbvh_status rtbvh_read_morton(rtbvh_ctx* ctx, uint32_t* codes);
/* Stable radix order: sorted codes and the triangle id of each sorted position. */
rtbvh_status rtbvh_read_sorted(rtbvh_ctx* ctx, uint32_t* sorted_codes, uint32_t* tri_ids);
/* reflectRay (after the last pass) and refractRay records of the last trace, one per traced
 * pixel in framebuffer order; needs RTBVH_FLAG_REFRACT_RECORDS at trace time.  Ray fields
 * HLSL leaves unset (a hit whose intensity is 0) are 0.  Either pointer may be NULL. */
rtbvh_status rtbvh_read_rays(rtbvh_ctx* ctx, rtbvh_ray_present* reflect_out, rtbvh_ray_present* refract_out);
rtbvh_status rtbvh_get_stats(rtbvh_ctx* ctx, rtbvh_stats* out);
/* Restart the timing averages of rtbvh_get_stats. */
rtbvh_status rtbvh_reset_stats(rtbvh_ctx* ctx);
/* Replace the RTBVH_FLAG_* bits of the context (takes effect for the next build/trace). */
rtbvh_status rtbvh_set_flags(rtbvh_ctx* ctx, uint32_t flags);
/* The binned primary pass lists every leaf in the screen-tile bins it covers.  The bins depend on the built tree
 * and the frame shape only (size, rank, band deal), so a context fills a bin set once and every later binned trace
 * of the same tree and shape, on any stream, reads it (environment RTBVH_BINS_REUSE=0 at rtbvh_create: a fill per
 * trace).  rtbvh_bin_builds: the fills enqueued since rtbvh_create; rtbvh_bin_sets: the bin sets the context
 * holds in device memory.  Both 0 for a NULL context. */
uint64_t rtbvh_bin_builds(rtbvh_ctx* ctx);
uint32_t rtbvh_bin_sets(rtbvh_ctx* ctx);

/* ---- primitives (exposed for tests and callers with their own buffers) ---- */
/* Stable LSD radix sort of (key, value) pairs, 8-bit digits over bits [0, key_bits).
 * Device pointers; keys/vals_in may be overwritten (ping-pong); the sorted
 * result lands in keys_out/vals_out.  Enqueued on the context stream. */
rtbvh_status rtbvh_sort_pairs_async(rtbvh_ctx* ctx, uint32_t* keys_in, uint32_t* vals_in,
                                    uint32_t* keys_out, uint32_t* vals_out, uint32_t n,
                                    uint32_t key_bits);
/* Host-memory convenience wrapper of the above (synchronous). */
rtbvh_status rtbvh_sort_pairs_host(rtbvh_ctx* ctx, const uint32_t* keys, const uint32_t* vals,
                                   uint32_t* keys_out, uint32_t* vals_out, uint32_t n, uint32_t key_bits);
/* Karras + refit on caller-given sorted codes and leaf boxes (host arrays; leaf
 * boxes n x 6 floats {min xyz, max xyz}); writes 2n-1 nodes (reference layout).
 * Lets the build kernels be checked on the reference's own RadixBVHCombo data. */
rtbvh_status rtbvh_build_from_codes(rtbvh_ctx* ctx, const uint32_t* sorted_codes,
                                    const float* leaf_boxes, uint32_t n, rtbvh_node* out);

/* ---- host-side scene helpers (ObjLoader replacement, camera) ---------------- */
/* Decode an uncompressed BMP (BI_RGB 1/4/8-bit paletted or 24/32-bit, BI_BITFIELDS 32-bit) into RGBA8 rows in
 * file order (bottom row first for the usual positive height), as DevIL hands them to
 * Image.cpp:48-49.  Free with rtbvh_texture_free. */
rtbvh_status rtbvh_texture_load_bmp(const char* path, rtbvh_texture* out);
/* Decode a baseline (sequential DCT, Huffman, 8-bit, 1 or 3 components, sampling up to 2x2)
 * JPEG file / memory buffer into RGBA8 rows, top row first, as DevIL hands them to
 * Image.cpp:48-49 (Test.mtl:12 binds Balls.jpg).  The arithmetic of libjpeg's default
 * decompression (islow IDCT, fancy upsampling, fixed-point YCbCr -> RGB), restated: bit-exact
 * against libjpeg-turbo on the reference's files.  RTBVH_ERR_IO for other or malformed files.
 * Free with rtbvh_texture_free. */
rtbvh_status rtbvh_texture_load_jpeg(const char* path, rtbvh_texture* out);
rtbvh_status rtbvh_texture_decode_jpeg(const uint8_t* data, size_t size, rtbvh_texture* out);
/* BMP or JPEG by the file's magic bytes (ObjLoader's map_Kd files, Image::loadImage). */
rtbvh_status rtbvh_texture_load(const char* path, rtbvh_texture* out);
void rtbvh_texture_free(rtbvh_texture* tex);
/* The 256-entry sRGB -> linear table the texture sampling uses (IEC 61966-2-1, in double). */
void rtbvh_srgb_table(float out[256]);
typedef struct rtbvh_scene rtbvh_scene;
/* ObjLoader::Load (ObjectFileLoader.cpp:212-547) incl. its de-duplication rules. */
rtbvh_status rtbvh_scene_load_obj(const char* path, rtbvh_scene** out);
/* Synthetic random triangles: splitmix64(seed), centroids uniform
 * in [-half,+half], vertex offsets (u-0.5)*1.0, face normals, one material. */
rtbvh_status rtbvh_scene_synthetic(uint64_t seed, uint32_t ntris, const float half_extent[3],
                                   rtbvh_scene** out);
void rtbvh_scene_free(rtbvh_scene* s);
uint32_t rtbvh_scene_num_vertices(const rtbvh_scene* s);
uint32_t rtbvh_scene_num_indices(const rtbvh_scene* s);
uint32_t rtbvh_scene_num_materials(const rtbvh_scene* s);
uint32_t rtbvh_scene_num_textures(const rtbvh_scene* s);
const rtbvh_vertex* rtbvh_scene_vertices(const rtbvh_scene* s);
const uint32_t* rtbvh_scene_indices(const rtbvh_scene* s);
const uint32_t* rtbvh_scene_mat_indices(const rtbvh_scene* s);
const rtbvh_material* rtbvh_scene_materials(const rtbvh_scene* s);
/* texture path of texture k (as named by map_Kd), or NULL */
const char* rtbvh_scene_texture_path(const rtbvh_scene* s, uint32_t k);
/* Upload a loaded scene (set_scene with the scene's arrays; textures as given). */
rtbvh_status rtbvh_set_scene_obj(rtbvh_ctx* ctx, const rtbvh_scene* s, const rtbvh_texture* textures,
                                 uint32_t ntex);
/* Graphics::onUpdate's camera (Graphics.cpp:44-53, Graphics.h:200-204):
 * LookAtLH(eye (0,5,-100), at 0, up +y) * PerspectiveFovLH(pi/4, H/W, 0.1, 1000). */
void rtbvh_camera_reference(uint32_t width, uint32_t height, float wvp[16], float wv[16]);
/* The same camera from any eye (at 0, up +y): Graphics::onUpdate after the eye has moved. */
void rtbvh_camera_look(const float eye[3], uint32_t width, uint32_t height, float wvp[16], float wv[16]);
/* Graphics::onKeyDown (Graphics.cpp:937-960): the eye rotated about `at` = 0 by CAM_DELTA = 0.1 rad
 * (Graphics.h:14): key 0 VK_LEFT (RotationY(-0.1)), 1 VK_RIGHT (RotationY(0.1)), 2 VK_UP (RotationX(0.1)),
 * 3 VK_DOWN (RotationX(-0.1)); the vector times the rotation matrix, row-vector convention (XMVector4Transform).
 * Other keys leave the eye unchanged.  (DirectXMath's own sin/cos approximation is not restated: libm's.) */
void rtbvh_camera_orbit(float eye[3], uint32_t key);

#ifdef __cplusplus
}
#endif
#endif /* RTBVH_H */
