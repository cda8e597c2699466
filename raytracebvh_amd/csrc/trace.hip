// trace.hip -- closest-hit traversal + shading kernels for gfx950.
//
// RayTraceLaunch.hlsl (primary rays, 15x15 thread groups) and
// RayTraceReflection.hlsl (bounce, every pixel re-dispatched, idle lanes for
// rays with intensity 0) on top of findCollision (RayTraceTraversal.hlsl:106-193).
// Here: a wave64 traces one 8x8 pixel tile (a 256-thread workgroup = 4 tiles
// side by side in one 8-row band, which is also the multi-GPU sharding unit);
// every child-pair test reads ONE 64-B node record; leaves read a 64-B record
// holding the clip-space triangle as (v0, e1 = v1-v0, e2 = v2-v0) -- the same
// floats the reference computes per test -- so getUpdateVerts and the edge
// subtractions are hoisted to the build; the bounce pass runs only over a
// wave-compacted queue of live rays (ballot + one atomic per wave).
//
// Traversal orders (DESIGN.md "Traversal"):
//  * reference order (default): the left-first DFS of findCollision exactly,
//    same pruning, strict `<` replacement -> bit-identical to the CPU oracle;
//  * nearest-first (RTBVH_FLAG_NEAREST_FIRST): the nearer child first, with the
//    lexicographic (t, leaf index) minimum kept, which is what the left-first DFS
//    returns whenever box/triangle rounding is consistent.
// The walks that lost their A/B measurements are not compiled here.
//
// Stack limit: the reference keeps a 32-entry stack and never checks it
// (RayTraceTraversal.hlsl:9,115,187).  Every walk here checks its own stack against
// a run-time limit (TraceArgs::stack_limit, <= the compiled capacity); a ray that would
// overflow ends with the best hit found so far, counts into counters[8] (the last
// trace's stats) and into *overflow (never reset: the API turns a change of it into
// RTBVH_ERR_STACK_OVERFLOW).  The walk-length guard (2T + 2 steps, only a cyclic tree
// from the CPUTests delta can trip it) counts the same way.
#include "rtbvh_internal.h"

#include <type_traits>

namespace rtbvh {
namespace {

constexpr uint32_t BLOCK = 256;
constexpr float EPSILON = 0.01f;   // RayTraceTraversal.hlsl:7

struct Counts { uint32_t internal, leaf, overflow, wint, wleaf; };   // w*: packet wave steps (lane 0)

typedef float f2v __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

// Node records live in SLOTS (rtbvh_device.h): the binary walks keep slots on their
// stacks.  The record of internal node k holds k's own index, so its internal
// children's records are at slots 2k and 2k+1; a leaf child is LEAF_BIT | j.
__device__ __forceinline__ uint32_t child_slot(uint32_t id, uint32_t own, uint32_t side) {
    return (id & LEAF_BIT) ? id : 2 * own + side;
}
__device__ __forceinline__ uint32_t root_slot(uint32_t T) { return T == 1 ? LEAF_BIT : 2 * T - 2; }

// Make loaded values live at this point, so the compiler issues every load of a
// record together (one memory round trip) instead of sinking some of them below
// an early-exit branch that needs only part of the record (ISA showed the leaf's
// v0 fetched in a second dependent round trip after the determinant test).
__device__ __forceinline__ void pin(float4& a) {
    float x = a.x, y = a.y, z = a.z, w = a.w;
    asm volatile("" : "+v"(x), "+v"(y), "+v"(z), "+v"(w));
    a = make_float4(x, y, z, w);
}
__device__ __forceinline__ void pin(float& a) { asm volatile("" : "+v"(a)); }
__device__ __forceinline__ void pin(v4f& a) { asm volatile("" : "+v"(a)); }

// rayTriangleCollision, RayTraceTraversal.hlsl:41-86, with edge1/edge2 precomputed
// by the build (identical floats: the same single subtraction)
__device__ __forceinline__ float ray_triangle(f3 o, f3 d, f3 p0, f3 e1, f3 e2) {
    f3 tmp = cross(d, e2);
    const float dx = dot(e1, tmp);
    if (fabsf(dx) < EPSILON) return -1.f;
    const float idx = 1.f / dx;
    const f3 rt = sub(o, p0);
    const float u = dot(rt, tmp) * idx;
    if (u < .0f || 1.f < u) return -1.f;
    tmp = cross(rt, e1);
    const float v = dot(d, tmp) * idx;
    if (v < .0f || 1.f < u + v) return -1.f;
    const float t = dot(e2, tmp) * idx;
    if (EPSILON < t) return t;
    return -1.f;
}

// rayBoxCollision, RayTraceTraversal.hlsl:92-104 (fminf/fmaxf drop NaN like HLSL
// min/max).  Also returns the entry distance, used by the nearest-first order.
__device__ __forceinline__ bool ray_box(f3 o, f3 inv, float bx0, float by0, float bz0, float bx1, float by1, float bz1,
                                        bool hit, float best, float& tmin) {
    const float tx0 = (bx0 - o.x) * inv.x, ty0 = (by0 - o.y) * inv.y, tz0 = (bz0 - o.z) * inv.z;
    const float tx1 = (bx1 - o.x) * inv.x, ty1 = (by1 - o.y) * inv.y, tz1 = (bz1 - o.z) * inv.z;
    const float mn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fminf(tz0, tz1));
    const float mx = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
    tmin = mn;
    return 0 <= mx && mn <= mx && (!hit || mn <= best);
}

// ray_box on a node record's layout (rtbvh_device.h): the (x, y) of a box corner is an
// aligned register pair, so the x and y slabs run as packed fp32 (v_pk_add_f32 /
// v_pk_mul_f32: two IEEE operations per instruction, the roundings of the scalar form,
// no contraction under -ffp-contract=off).
__device__ __forceinline__ bool ray_box_xy(f3 o, f3 inv, f2v lo, f2v hi, float lz, float hz, bool hit, float best,
                                           float& tmin) {
    const f2v oxy = {o.x, o.y}, ixy = {inv.x, inv.y};
    const f2v t0 = (lo - oxy) * ixy, t1 = (hi - oxy) * ixy;
    const float tz0 = (lz - o.z) * inv.z, tz1 = (hz - o.z) * inv.z;
    const float mn = fmaxf(fmaxf(fminf(t0.x, t1.x), fminf(t0.y, t1.y)), fminf(tz0, tz1));
    const float mx = fminf(fminf(fmaxf(t0.x, t1.x), fmaxf(t0.y, t1.y)), fmaxf(tz0, tz1));
    tmin = mn;
    return 0 <= mx && mn <= mx && (!hit || mn <= best);
}

// ---- the per-lane binary walk: findCollision, RayTraceTraversal.hlsl:106-193 ------------------
// One ray's walk state.  The reference keeps stack[0] = -1 and loops `do { ... } while (stackIndex != -1)`;
// here the entry at the top of the stack is cached in a register (`top`), so a pop hands over the next node
// at once and refills `top` from the stack in the background.  sp: the reference stack index (entries
// [0, sp) below the cached top; entry 0 is the sentinel = top at start; -1: the walk is over).
// bl: the best hit's sorted leaf index.  guard: a valid tree is walked in <= 2T-1 steps.
struct Walk {
    uint32_t node, top;
    int sp;
    bool hit;
    float best;
    uint32_t bl, guard;
};
__device__ __forceinline__ Walk walk_start(uint32_t root, uint32_t T) {
    return Walk{root, INVALID, 0, false, 0.f, 0u, 2 * T + 2};
}

// The rules of a walk: its order, which triangle distance replaces the best hit, and which box is entered.
// WalkRule: the reference's (strict `<` replacement; NEAREST: the nearer child first, the lexicographic
// (t, leaf index) minimum kept).
template <bool NEAREST_FIRST> struct WalkRule {
    static constexpr bool NEAREST = NEAREST_FIRST, FIRST_HIT = false;
    __device__ __forceinline__ bool accept(const Walk& w, float t, uint32_t j) const {
        return t != -1.f && (!w.hit || t < w.best || (NEAREST && t == w.best && j < w.bl));
    }
    __device__ __forceinline__ bool box(f3 o, f3 inv, f2v lo, f2v hi, float lz, float hz, const Walk& w,
                                        float& tmin) const {
        return ray_box_xy(o, inv, lo, hi, lz, hz, w.hit, w.best, tmin);
    }
};
// QueryRule (k_query): t_max enters in two places only: a triangle's t is accepted iff the reference accepts
// it and t <= t_max; a box passes iff the reference's first two conditions hold and
// (hit ? mn <= dist : !(mn > t_max)) -- with t_max = +inf the reference, bit for bit.
// ANY: the box test without the `hit` branch, the walk ends at the first accepted triangle.
template <bool ANY>
__device__ __forceinline__ bool query_box(f3 o, f3 inv, f2v lo, f2v hi, float lz, float hz, bool hit, float best,
                                          float tmax, float& mn) {
    const bool base = ray_box_xy(o, inv, lo, hi, lz, hz, false, 0.f, mn);
    return base && (!ANY && hit ? mn <= best : !(mn > tmax));
}
template <bool ANY> struct QueryRule {
    static constexpr bool NEAREST = false, FIRST_HIT = ANY;
    float tmax;
    __device__ __forceinline__ bool accept(const Walk& w, float t, uint32_t) const {
        return t != -1.f && t <= tmax && (ANY || !w.hit || t < w.best);
    }
    __device__ __forceinline__ bool box(f3 o, f3 inv, f2v lo, f2v hi, float lz, float hz, const Walk& w,
                                        float& tmin) const {
        return query_box<ANY>(o, inv, lo, hi, lz, hz, w.hit, w.best, tmax, tmin);
    }
};

// The stack of a one-ray-per-lane kernel (a Stack supplies store(k, v) and load(k) of entry k): entries
// [0, LSB) in LDS (`lst`: this lane's column, entry k at lst[k * BLOCK]; a wave's lanes on 64 distinct banks),
// deeper ones in scratch (`s`: the walk's own array); LSB = 0: all in scratch.  The pop is one flat load of a
// selected pointer (LDS or scratch); forcing ds_read (a module-scope array, every lane reading LDS and the
// deeper ones scratch as well) was 1-2% slower at C3.  The push stays a ds_write or a scratch store: `s` is
// typed as a scratch pointer, or the compiler merges the two into one flat store of a selected pointer too.
// (The persistent kernels' stack: BlockStack, below.)
#ifndef RTBVH_LANE_LSB
#define RTBVH_LANE_LSB 16
#endif
constexpr int LANE_LSB = RTBVH_LANE_LSB;
template <int LSB> struct LaneStack {
    uint32_t* lst;
    __attribute__((address_space(5))) uint32_t* s;
    __device__ __forceinline__ void store(int k, uint32_t v) {
        if (LSB > 0 && k < LSB) lst[k * BLOCK] = v;
        else s[k] = v;
    }
    __device__ __forceinline__ uint32_t load(int k) const {
        return LSB > 0 ? *(k < LSB ? lst + k * BLOCK : (uint32_t*)(s + k)) : s[k];
    }
};

// pop: the next node from the cached top; refill the top from entry --sp
template <class Stack> __device__ __forceinline__ void walk_pop(Walk& w, const Stack& st) {
    w.node = w.top;
    if (--w.sp >= 0) w.top = st.load(w.sp);
}
// The ray is at leaf j (its triangle p0, e1, e2 already fetched): the triangle test, the rule's replacement of
// the best hit, the pop.  Returns whether the triangle was accepted (a FIRST_HIT walk then stays at the leaf).
template <bool COUNT, class Rule, class Stack>
__device__ __forceinline__ bool walk_leaf(Walk& w, Stack& st, const Rule& rule, Counts& c, f3 o, f3 d, uint32_t j,
                                          f3 p0, f3 e1, f3 e2) {
    if (COUNT) c.leaf++;
    const float t = ray_triangle(o, d, p0, e1, e2);
    const bool acc = rule.accept(w, t, j);
    if (acc) {
        w.best = t;
        w.bl = j;
        w.hit = true;
    }
    if (!(Rule::FIRST_HIT && acc)) walk_pop(w, st);
    return acc;
}
// the two children of an internal node: ids as the walk keeps them (a Tree's), boxes as aligned (x, y) pairs and z
struct ChildPair {
    uint32_t cl, cr;
    f2v llo, lhi, rlo, rhi;
    float lz0, lz1, rz0, rz1;
};
// The ray is at an internal node (its children already fetched): the two slab tests, the order, the push of
// the second child -- a ray that would exceed `limit` entries loses both children, counted -- or the pop.
template <bool COUNT, class Rule, class Stack>
__device__ __forceinline__ void walk_node(Walk& w, Stack& st, const Rule& rule, Counts& c, f3 o, f3 inv, int limit,
                                          const ChildPair& ch) {
    if (COUNT) c.internal++;
    float tl, tr;
    const bool lh = rule.box(o, inv, ch.llo, ch.lhi, ch.lz0, ch.lz1, w, tl);
    const bool rh = rule.box(o, inv, ch.rlo, ch.rhi, ch.rz0, ch.rz1, w, tr);
    if (!lh && !rh) {
        walk_pop(w, st);
        return;
    }
    const bool swap = Rule::NEAREST && lh && rh && tr < tl;
    if (lh && rh) {
        if (w.sp + 1 >= limit) {
            c.overflow++;
            walk_pop(w, st);
            return;
        }
        st.store(w.sp, w.top);   // push the second child
        w.sp++;
        w.top = swap ? ch.cl : ch.cr;
    }
    w.node = swap ? ch.cr : (lh ? ch.cl : ch.cr);
}

// The two forms of the tree (a Tree supplies root(T) and children(node)).
// Node records live in SLOTS (rtbvh_device.h): the walk keeps slots on its stack, and every child-pair test
// reads ONE 64-B record (words 0..11 the boxes, 12..14 the children's ids and the node's own index).
__device__ __forceinline__ ChildPair record_children(v4f q0, v4f q1, v4f q2, uint32_t cl, uint32_t cr) {
    return ChildPair{cl, cr, q0.xy, q0.zw, q1.xy, q1.zw, q2.x, q2.y, q2.z, q2.w};
}
struct RecordTree {
    const Inner* __restrict__ inner;
    __device__ __forceinline__ uint32_t root(uint32_t T) const { return root_slot(T); }
    __device__ __forceinline__ ChildPair children(uint32_t node) const {
        const v4f* r = reinterpret_cast<const v4f*>(inner + node);
        const v4f q0 = r[0], q1 = r[1], q2 = r[2];
        const uint4 q3 = reinterpret_cast<const uint4*>(r)[3];
        return record_children(q0, q1, q2, child_slot(q3.x, q3.z, 0), child_slot(q3.y, q3.z, 1));
    }
};
// The topology and the node boxes, for a build that wrote no node records (api.hip: a certified-only context's):
// at internal node k its children from topo[k], their boxes from nbox (internal) or the leaf record (words
// 10..15), the same slab test in the same operations -- the same visits, in the same order, and the same hit.
// Two dependent fetches a step instead of one: the certified walks' few re-traced rays only.
__device__ __forceinline__ void nb_child_box(const float* __restrict__ nbox, const float4* __restrict__ leaf, uint32_t c,
                                             f2v& mnxy, f2v& mxxy, float& mnz, float& mxz) {
    if (c & LEAF_BIT) {
        const float4* r = leaf + 4 * (size_t)(c & ~LEAF_BIT);
        const float4 w2 = r[2], w3 = r[3];
        mnxy = f2v{w2.z, w2.w}; mnz = w3.x; mxxy = f2v{w3.y, w3.z}; mxz = w3.w;
    } else {
        const float2* d = reinterpret_cast<const float2*>(nbox + 6 * (size_t)c);
        const float2 x = d[0], y = d[1], z = d[2];
        mnxy = f2v{x.x, x.y}; mnz = y.x; mxxy = f2v{y.y, z.x}; mxz = z.y;
    }
}
struct NodeBoxTree {
    const uint4* __restrict__ topo;
    const float* __restrict__ nbox;
    const float4* __restrict__ leaf;
    // the root: internal node 0 (a one-leaf tree: the leaf)
    __device__ __forceinline__ uint32_t root(uint32_t T) const { return T > 1 ? 0u : LEAF_BIT; }
    __device__ __forceinline__ ChildPair children(uint32_t node) const {
        const uint4 q = topo[node];
        ChildPair ch;
        ch.cl = q.x;
        ch.cr = q.y;
        nb_child_box(nbox, leaf, ch.cl, ch.llo, ch.lhi, ch.lz0, ch.lz1);
        nb_child_box(nbox, leaf, ch.cr, ch.rlo, ch.rhi, ch.rz0, ch.rz1);
        return ch;
    }
};

// findCollision for one ray per lane: each branch fetches what it needs (a leaf 2 1/4 words of its record, a
// node its children).  Returns hit; best_leaf = sorted leaf index.  `limit` <= STACK_SIZE entries.
template <bool COUNT, bool NEAREST, int LSB = 0, class Tree>
__device__ __forceinline__ bool traverse(const Tree& tree, const float4* __restrict__ leaf, uint32_t T, f3 o, f3 d,
                                         f3 inv, int limit, float& best, uint32_t& best_leaf, Counts& c,
                                         uint32_t* lst = nullptr) {
    const WalkRule<NEAREST> rule;
    uint32_t stack[STACK_SIZE];
    LaneStack<LSB> st{lst, (__attribute__((address_space(5))) uint32_t*)stack};
    Walk w = walk_start(tree.root(T), T);
    do {
        if (--w.guard == 0) { c.overflow++; break; }
        if (w.node & LEAF_BIT) {
            const uint32_t j = w.node & ~LEAF_BIT;
            const float4* r = leaf + 4 * (size_t)j;
            float4 a = r[0], b = r[1];
            float e2z = r[2].x;
            pin(a); pin(b); pin(e2z);
            walk_leaf<COUNT>(w, st, rule, c, o, d, j, mk(a.x, a.y, a.z), mk(a.w, b.x, b.y), mk(b.z, b.w, e2z));
        } else {
            walk_node<COUNT>(w, st, rule, c, o, inv, limit, tree.children(w.node));
        }
    } while (w.sp != -1);
    best = w.best;
    best_leaf = w.bl;
    return w.hit;
}
// the reference-order walk of a re-traced ray: on the records, or (nb) the topology and node boxes
template <bool COUNT>
__device__ __forceinline__ bool traverse_ref(bool nb, const Inner* __restrict__ inner, const uint4* __restrict__ topo,
                                             const float* __restrict__ nbox, const float4* __restrict__ leaf,
                                             uint32_t T, f3 o, f3 d, f3 inv, float& best, uint32_t& bl, Counts& c) {
    return nb ? traverse<COUNT, false>(NodeBoxTree{topo, nbox, leaf}, leaf, T, o, d, inv, STACK_SIZE, best, bl, c)
              : traverse<COUNT, false>(RecordTree{inner}, leaf, T, o, d, inv, STACK_SIZE, best, bl, c);
}
template <bool COUNT>
__device__ __forceinline__ bool traverse_ref(const TraceArgs& a, f3 o, f3 d, f3 inv, float& best, uint32_t& bl,
                                             Counts& c) {
    return traverse_ref<COUNT>(a.nb, a.inner, a.topo, a.nbox, a.leaf, a.T, o, d, inv, best, bl, c);
}

// ---- wave-packet traversal (primary rays) -------------------------------------
// The 64 rays of an 8x8 pixel tile are nearly parallel neighbours, so a wave walks
// ONE node at a time with a per-node lane mask: the node record is fetched by the
// scalar unit (s_load through the constant address space: no vector-memory/TA
// work, which PMC showed saturated), each masked lane tests the child boxes with
// its own (hit, best), and the children are visited with the ballots of the lanes
// that hit them.  In reference order every lane sees exactly its own findCollision
// sequence (the nodes it visits are a subsequence of the wave's walk, in the same
// order, and nothing changes its state in between), so results and per-lane visit
// counts are identical to the per-lane DFS.  In nearest-first mode the wave takes
// the child most of its lanes see first.
typedef float v16f __attribute__((ext_vector_type(16)));
typedef const v16f __attribute__((address_space(4))) cv16f;

// the whole 64-B record in one s_load_dwordx16 (one scalar-memory round trip per step)
__device__ __forceinline__ v16f sload16(const void* p) { return *(cv16f*)p; }

template <bool COUNT, bool NEAREST>
__device__ __forceinline__ bool traverse_packet(const Inner* __restrict__ inner, const float4* __restrict__ leaf,
                                                uint32_t T, f3 o, f3 d, f3 inv, bool valid, int limit, float& best,
                                                uint32_t& best_leaf, Counts& c, uint32_t* s_st /* per wave [3*STACK_SIZE] */) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lanebit = 1ull << lane;
    bool hit = false;
    best = 0.f;
    best_leaf = 0;
    uint64_t mask = __ballot(valid);
    int sp = 0;                      // entries on the wave stack; the top one is cached below
    uint32_t node = root_slot(T), top_node = 0;
    uint64_t top_mask = 0;
    if (mask == 0) return false;
    uint32_t guard = 2 * T + 2;
    while (true) {
        if (--guard == 0) { c.overflow += valid; break; }   // the wave's rays in the frame end early
        bool pop = false;
        if (node & LEAF_BIT) {
            const uint32_t j = node & ~LEAF_BIT;
            const v16f q = sload16(leaf + 4 * (size_t)j);
            if (COUNT && lane == 0) c.wleaf++;
            if (mask & lanebit) {
                if (COUNT) c.leaf++;
                const float t = ray_triangle(o, d, mk(q[0], q[1], q[2]), mk(q[3], q[4], q[5]), mk(q[6], q[7], q[8]));
                if (t != -1.f && (!hit || t < best || (NEAREST && t == best && j < best_leaf))) {
                    best = t;
                    best_leaf = j;
                    hit = true;
                }
            }
            pop = true;
        } else {
            const v16f q = sload16(inner + node);
            if (COUNT && lane == 0) c.wint++;
            const uint32_t own = __float_as_uint(q[14]);
            const uint32_t cl = child_slot(__float_as_uint(q[12]), own, 0), cr = child_slot(__float_as_uint(q[13]), own, 1);
            bool lh = false, rh = false;
            float tl = 0.f, tr = 0.f;
            if (mask & lanebit) {
                if (COUNT) c.internal++;
                lh = ray_box_xy(o, inv, q.s01, q.s23, q[8], q[9], hit, best, tl);
                rh = ray_box_xy(o, inv, q.s45, q.s67, q[10], q[11], hit, best, tr);
            }
            const uint64_t ml = __ballot(lh), mr = __ballot(rh);
            if ((ml | mr) == 0) {
                pop = true;
            } else if (ml && mr) {
                bool swap = false;
                if (NEAREST) {
                    const uint64_t both = __ballot(lh && rh);
                    const uint64_t rfirst = __ballot(lh && rh && tr < tl);
                    swap = 2 * __popcll(rfirst) > __popcll(both);
                }
                if (sp + 1 >= limit) {   // the lanes of both children lose them
                    c.overflow += ((ml | mr) & lanebit) != 0;
                    pop = true;
                } else {
                    // push the second child and its lanes: the old top goes to LDS, the
                    // new entry stays in SGPRs (top cache, as in the per-lane loop)
                    if (sp > 0 && lane == 0) {
                        s_st[3 * sp] = top_node;
                        s_st[3 * sp + 1] = (uint32_t)top_mask;
                        s_st[3 * sp + 2] = (uint32_t)(top_mask >> 32);
                    }
                    ++sp;
                    top_node = swap ? cl : cr;
                    top_mask = swap ? ml : mr;
                    node = swap ? cr : cl;
                    mask = swap ? mr : ml;
                }
            } else {
                node = ml ? cl : cr;
                mask = ml ? ml : mr;
            }
        }
        if (pop) {
            if (sp == 0) break;
            node = top_node;
            mask = top_mask;
            if (--sp > 0) {   // refill the cached top from LDS (lane 0's earlier write)
                top_node = __builtin_amdgcn_readfirstlane(s_st[3 * sp]);
                const uint32_t lo = __builtin_amdgcn_readfirstlane(s_st[3 * sp + 1]);
                const uint32_t hi = __builtin_amdgcn_readfirstlane(s_st[3 * sp + 2]);
                top_mask = ((uint64_t)hi << 32) | lo;
            }
        }
    }
    return hit;
}

// ray_triangle without early exits, for the packet walk's leaf step: every lane evaluates
// the same operations, and each rejection of the reference's order becomes a select of -1
// (pinned, so the six tests stay VALU selects rather than lane masks combined on the SALU).
// The same floats and the same accept predicate: the same result.  `in` false also gives -1.
__device__ __forceinline__ float ray_triangle_flat(f3 o, f3 d, f3 p0, f3 e1, f3 e2, bool in) {
    const f3 tmp = cross(d, e2);
    const float dx = dot(e1, tmp);
    const float idx = recip(dx);
    const f3 rt = sub(o, p0);
    const float u = dot(rt, tmp) * idx;
    const f3 q = cross(rt, e1);
    const float v = dot(d, q) * idx;
    const float t = dot(e2, q) * idx;
    float r = EPSILON < t ? t : -1.f;
    pin(r);
    r = fabsf(dx) < EPSILON ? -1.f : r;
    pin(r);
    r = u < .0f ? -1.f : r;
    pin(r);
    r = 1.f < u ? -1.f : r;
    pin(r);
    r = v < .0f ? -1.f : r;
    pin(r);
    r = 1.f < u + v ? -1.f : r;
    pin(r);
    return in ? r : -1.f;
}

// (t, leaf) of the best hit as one u64 key, t's bits above: t > EPSILON > 0, so the u64 order is
// the (t, leaf) order; before any hit (+inf, ~0), which every hit beats.  The entry distance of a
// box is then compared with the key's t alone: with no hit it is +inf, and a box whose entry is
// not <= +inf (NaN) fails the slab test's own mn <= mx too, as the reference's !hit || ... does.
constexpr uint64_t NO_HIT = 0x7F800000FFFFFFFFull;
__device__ __forceinline__ float key_t(uint64_t key) { return __uint_as_float((uint32_t)(key >> 32)); }
// a bounce hit record's word (the triangle, INVALID for a miss) with bit 30 flipped: the certified walk
// could not vouch for the ray (k_bounce_trav CERT); the shading hands it to the reference-order re-trace
constexpr uint32_t HIT_FLAG = 0x40000000u;
__device__ __forceinline__ bool hit_flagged(uint32_t w) { return ((w >> 31) ^ (w >> 30)) & 1u; }

// v_writelane_b32: lane K of v := the wave-uniform s (a VALU op, no scalar work)
template <int K> __device__ __forceinline__ void writelane(uint32_t& v, uint32_t s) {
    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(s), "i"(K));
}

// ---- wave-packet traversal on the 4-wide view (primary rays) -------------------
// As traverse_packet, but one step reads the 128-B record pair inner4[2p], inner4[2p+1]
// (two s_load_dwordx16 of one line): the boxes of p's four grandchildren.  Children are
// taken left to right (the left-first DFS's order LL, LR, RL, RR); the per-lane result is
// the (t, leaf) minimum, as for the 4-wide bounce walk.
//
// Axis-parallel box test: the rays run along d = (0, 0, 1) from z = 0 (k_primary), so
// inv = (inf, inf, 1) and each x/y slab of ray_box_xy yields [-inf, inf] (or NaNs that
// fminf/fmaxf drop) exactly when min < o < max, and an empty slab otherwise.  For a box
// whose record bit (word 15, build.hip general_box) is clear -- min < max in x and y,
// min.z <= max.z, 0 <= max.z < inf -- the test is therefore exactly
//     min.x < o.x < max.x  &&  min.y < o.y < max.y  &&  (!hit || min.z <= best)
// (denormals are kept, so min < o has the sign of min - o), evaluated as o - min and
// max - o as packed differences and min(...) > 0.  A node with any bit set takes the
// general test.
//
// Per-step work (one wave step is ~100 instructions, and 32 waves share the CU's one
// scalar unit):
//  * lanes 0..3 of (vid, vlo, vhi) hold child k's id and lane mask (v_writelane), so the hit
//    set is one ballot, the next node a v_readlane and the pushes one vector store per word;
//  * the fast box test needs no AND with the parent's lanes: a box whose bit is clear lies
//    inside its parent's box, so a lane that passes it passed the parent's test (at a bound
//    >= today's) -- lanes outside the frame get a NaN origin, which fails every fast test,
//    and a pseudo-record's absent child has a NaN min.z (build.hip store_pseudo_record);
//  * the leaf test runs on every lane without branches (ray_triangle_flat) and the (t, leaf)
//    minimum is one u64 compare;
//  * stack entry 0 is a sentinel, so a pop has no empty-stack test and the loop one exit.
// A/B at C5 (10M triangles, 3840x2160, frame identical): 2.60 ms for the per-child lane-0
// pushes with the parent-mask AND, 2.23 with the lanes-0..3 form, 2.20 with the sentinel and
// the NaN min.z, 2.18 with the z test as its own lane mask (VALU -> SALU); a branchless tail
// (descend or pop by selects, the stack top read at the step's start) ran 2.45.
// GUARD false (a clz64 tree, k_primary walk 5): no walk-length guard, and without a run-time
// stack limit (CHECK false) no stack check either: a clz64 tree has <= 64 internal levels (each
// child's common-prefix length exceeds its parent's, 0..63), a step descends two levels and
// pushes <= 3 entries, so the stack holds <= 3 * 32 + 1 < STACK4 + 1 entries.
// No lane masks on the stack: a wave needs the lanes that reach a node only at a leaf (which
// lanes test its triangle), and those are the lanes whose ray passes the leaf's own box with the
// current bound -- its record holds the box (words 10..15), so the leaf step tests it again, with
// the fast or the general form as the parent step did.  Every lane the parent step let through
// passes it unless its bound has since fallen below the box's entry, and such a lane cannot improve
// its (t, leaf) minimum there.  Internal steps never needed the masks (a child's box lies inside its
// parent's, and the slab test is monotone in the box), so a stack entry is a node id alone: one
// v_writelane per child for its id and one for its any-lane bit instead of three, one word per push
// and pop.  The visit counters (COUNT) still keep each entry's lanes, beside the same walk.
template <bool COUNT, bool GUARD, bool CHECK>
__device__ __forceinline__ bool traverse_packet4(const Inner* __restrict__ inner4, const float4* __restrict__ leaf,
                                                 uint32_t T, f3 o, f3 d, f3 inv, bool valid, int limit, float& best,
                                                 uint32_t& best_leaf, Counts& c, uint32_t* s_st /* [3*(STACK4+1)] */) {
    constexpr int EW = COUNT ? 3 : 1;   // words per stack entry: the node, and its lanes for the counters
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t mask = __ballot(valid);
    best = 0.f;
    best_leaf = 0;
    if (mask == 0) return false;
    const float qnan = __builtin_nanf("");
    const f2v oxy = valid ? f2v{o.x, o.y} : f2v{qnan, qnan};
    uint64_t key = NO_HIT;
    uint32_t vid = 0, vlo = 0, vhi = 0;
    // entry 0 is a sentinel (node INVALID): popping it ends the walk, so a pop needs no
    // empty-stack test and the loop has one exit
    if (lane == 0) s_st[0] = INVALID;
    int sp = 1;
    uint32_t node = (T == 1) ? LEAF_BIT : 0u;
    uint32_t guard = 2 * T + 2;
    do {
        node = __builtin_amdgcn_readfirstlane(node);
        if (node & LEAF_BIT) {
            const uint32_t j = node & ~LEAF_BIT;
            const v16f q = sload16(leaf + 4 * (size_t)j);
            if (COUNT && lane == 0) c.wleaf++;
            // the lanes that need this leaf: its own box {min q[10..12], max q[13..15]}, tested as the
            // parent step tested it (rtbvh_device.h word 15: the fast form for a box that allows it)
            const float lx = q[10], ly = q[11], lz = q[12], hx = q[13], hy = q[14], hz = q[15];
            const float bound = __uint_as_float((uint32_t)(key >> 32));
            bool in;
            if (!(__float_as_uint(q[9]) & LEAF_BIT)) {   // the box allows the fast form (build.hip leaf_tri_word)
                const f2v d0 = oxy - f2v{lx, ly}, d1 = f2v{hx, hy} - oxy;
                in = fminf(fminf(d0.x, d0.y), fminf(d1.x, d1.y)) > 0.f && lz <= bound;
            } else {
                const bool hit = key != NO_HIT;
                float tt;
                in = valid && ray_box_xy(o, inv, f2v{lx, ly}, f2v{hx, hy}, lz, hz, hit, hit ? bound : 0.f, tt);
            }
            if (COUNT) c.leaf += (mask >> lane) & 1u;
            const float t =
                ray_triangle_flat(o, d, mk(q[0], q[1], q[2]), mk(q[3], q[4], q[5]), mk(q[6], q[7], q[8]), in);
            const uint64_t k = t == -1.f ? ~0ull : (uint64_t)__float_as_uint(t) << 32 | j;
            key = k < key ? k : key;
        } else {
            const v16f A = sload16(inner4 + 2 * (size_t)node);
            const v16f B = sload16(inner4 + 2 * (size_t)node + 1);
            if (COUNT && lane == 0) c.wint++;
            if (COUNT) c.internal += (mask >> lane) & 1u;
            const uint32_t id0 = __float_as_uint(A[12]), id1 = __float_as_uint(A[13]);
            const uint32_t id2 = __float_as_uint(B[12]), id3 = __float_as_uint(B[13]);
            uint64_t m0, m1, m2, m3;
            const float bound = __uint_as_float((uint32_t)(key >> 32));
            if ((__float_as_uint(A[15]) | __float_as_uint(B[15])) == 0) {   // wave-uniform
                // min(o - lo, hi - o) > 0 with lz <= bound folded in as a select (pinned, so the
                // compiler keeps it a VALU select instead of ANDing two lane masks on the SALU)
                const auto lanes = [&](f2v lo, f2v hi, float lz) {
                    const f2v d0 = oxy - lo, d1 = hi - oxy;
                    float m = fminf(fminf(d0.x, d0.y), fminf(d1.x, d1.y));
                    return __builtin_amdgcn_ballot_w64(m > 0.f) & __builtin_amdgcn_ballot_w64(lz <= bound);
                };
                m0 = lanes(A.s01, A.s23, A[8]);
                m1 = lanes(A.s45, A.s67, A[10]);
                m2 = lanes(B.s01, B.s23, B[8]);
                m3 = lanes(B.s45, B.s67, B[10]);
            } else {
                const bool hit = key != NO_HIT;
                const float bst = hit ? bound : 0.f;
                bool h0 = false, h1 = false, h2 = false, h3 = false;
                float t0, t1, t2, t3;
                if (valid) {   // a lane the parent let not through fails these too (monotone)
                    h0 = ray_box_xy(o, inv, A.s01, A.s23, A[8], A[9], hit, bst, t0);
                    h1 = ray_box_xy(o, inv, A.s45, A.s67, A[10], A[11], hit, bst, t1) & (id1 != INVALID);
                    h2 = ray_box_xy(o, inv, B.s01, B.s23, B[8], B[9], hit, bst, t2);
                    h3 = ray_box_xy(o, inv, B.s45, B.s67, B[10], B[11], hit, bst, t3) & (id3 != INVALID);
                }
                m0 = __ballot(h0); m1 = __ballot(h1); m2 = __ballot(h2); m3 = __ballot(h3);
            }
            writelane<0>(vid, id0);
            writelane<1>(vid, id1);
            writelane<2>(vid, id2);
            writelane<3>(vid, id3);
            if (COUNT) {
                writelane<0>(vlo, (uint32_t)m0);
                writelane<1>(vlo, (uint32_t)m1);
                writelane<2>(vlo, (uint32_t)m2);
                writelane<3>(vlo, (uint32_t)m3);
                writelane<0>(vhi, (uint32_t)(m0 >> 32));
                writelane<1>(vhi, (uint32_t)(m1 >> 32));
                writelane<2>(vhi, (uint32_t)(m2 >> 32));
                writelane<3>(vhi, (uint32_t)(m3 >> 32));
            }
            // (an absent second child -- INVALID id, a leaf's pseudo-record -- has a NaN min.z and
            // hits no lane in the fast test; the general test checks its id)
            // which children any lane hits: the OR of each mask's halves in lanes 0..3, one ballot
            // (the same from four 64-bit compares on the SALU: +45% SALU, primary +2%)
            uint32_t vor = 0;
            writelane<0>(vor, (uint32_t)m0 | (uint32_t)(m0 >> 32));
            writelane<1>(vor, (uint32_t)m1 | (uint32_t)(m1 >> 32));
            writelane<2>(vor, (uint32_t)m2 | (uint32_t)(m2 >> 32));
            writelane<3>(vor, (uint32_t)m3 | (uint32_t)(m3 >> 32));
            const uint32_t hs = (uint32_t)__builtin_amdgcn_ballot_w64(vor != 0);   // lanes >= 4 stay 0
            if (hs != 0) {
                const uint32_t rest = hs & (hs - 1);
                const int npush = __builtin_popcount(rest);
                if (!CHECK || sp + npush <= limit + 1) {
                    const uint32_t first = (uint32_t)__builtin_ctz(hs);
                    node = __builtin_amdgcn_readlane(vid, first);
                    if (COUNT)
                        mask = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(vhi, first) << 32 |
                               (uint32_t)__builtin_amdgcn_readlane(vlo, first);
                    if (((uint64_t)rest >> lane) & 1u) {   // the later a child, the deeper its entry
                        const int pos = sp + __builtin_popcount(rest >> (lane + 1));
                        s_st[EW * pos] = vid;
                        if (COUNT) {
                            s_st[EW * pos + 1] = vlo;
                            s_st[EW * pos + 2] = vhi;
                        }
                    }
                    sp += npush;
                    continue;
                }
                // the step's children are skipped: count the rays that hit one of them (once per lane,
                // not 64 per wave event)
                c.overflow += (uint32_t)(((m0 | m1 | m2 | m3) >> lane) & 1u);
            }
        }
        --sp;
        node = __builtin_amdgcn_readfirstlane(s_st[EW * sp]);
        if (COUNT) {
            const uint32_t lo = __builtin_amdgcn_readfirstlane(s_st[EW * sp + 1]);
            const uint32_t hi = __builtin_amdgcn_readfirstlane(s_st[EW * sp + 2]);
            mask = ((uint64_t)hi << 32) | lo;
        }
    } while (node != INVALID && (!GUARD || --guard != 0));
    if (GUARD && guard == 0) c.overflow += valid;
    const bool hit = key != NO_HIT;
    if (hit) { best = __uint_as_float((uint32_t)(key >> 32)); best_leaf = (uint32_t)key; }
    return hit;
}

// Primary walks: 0 per-lane reference order, 1 per-lane nearest-first,
// 2 packet reference order, 3 packet nearest-first, 4 4-wide packet (axis-parallel test),
// 5 the same without the walk-length guard (a clz64 tree has no cycles; ~6 SALU per step)
// 6: the reference order per lane on the topology and the node boxes (a certified trace's overflowed tiles and
// frames past the binned pass's size, on a build without node records: traverse on a NodeBoxTree)
template <int K> struct PrimaryWalk {
    static constexpr bool NEAREST = (K == 1 || K == 3);
    static constexpr bool PACKET = (K >= 2 && K <= 5);
    static constexpr bool WIDE = (K == 4 || K == 5);
    static constexpr bool GUARD = (K != 5);   // 5: the 4-wide walk on a clz64 tree (acyclic)
    static constexpr bool NB = (K == 6);
};

struct HitInfo {
    float4 color;   // renderPixel(...) * specular
    f3 hitp, nrm;
    float shininess, alpha, optical_density;
    bool textured;
};

// HLSL refract(i, n, eta) as documented (see oracle refract_hlsl; same operation order)
__device__ __forceinline__ f3 refract_hlsl(f3 i, f3 n, float eta) {
    const float cosi = dot(mk(-i.x, -i.y, -i.z), n);
    const float cost2 = 1.0f - eta * eta * (1.0f - cosi * cosi);
    const float s = eta * cosi - sqrtf(fabsf(cost2));
    const f3 t = add(mul(i, eta), mul(n, s));
    const float keep = cost2 > 0.0f ? 1.0f : 0.0f;
    return mul(t, keep);
}

// RayPresent record (RayTraceGlobal.hlsl:30-35), 14 floats at 56*idx (8-B aligned):
// intensity, origin, direction, invDirection, color.  `ray` false writes a zero ray
// (fields HLSL leaves unset when the intensity is 0, and clearRayPresent on a miss).
__device__ __forceinline__ void put_record(float* rec, size_t idx, float intensity, bool ray, f3 o, f3 d,
                                           float4 color) {
    float2* r = reinterpret_cast<float2*>(rec + 14 * idx);
    if (!ray) { o = mk(0.f, 0.f, 0.f); d = o; }
    const f3 inv = ray ? mk(1.f / d.x, 1.f / d.y, 1.f / d.z) : mk(0.f, 0.f, 0.f);
    r[0] = make_float2(intensity, o.x);
    r[1] = make_float2(o.y, o.z);
    r[2] = make_float2(d.x, d.y);
    r[3] = make_float2(d.z, inv.x);
    r[4] = make_float2(inv.y, inv.z);
    r[5] = make_float2(color.x, color.y);
    r[6] = make_float2(color.z, color.w);
}

// diffuseTex[k].SampleLevel(compSample, uv, 0) as restated in include/rtbvh.h
// (rtbvh_texture): sRGB texels -> linear by table, wrap, fp32 bilinear.
__device__ __forceinline__ float4 texel(const TraceArgs& a, uint32_t first, uint32_t w, uint32_t x, uint32_t y) {
    const uint32_t p = a.texels[first + (size_t)y * w + x];
    return make_float4(a.srgb[p & 255u], a.srgb[(p >> 8) & 255u], a.srgb[(p >> 16) & 255u], (float)(p >> 24) / 255.f);
}
__device__ __forceinline__ uint32_t wrap_index(float f, uint32_t n) {
    if (!(fabsf(f) < 2147483648.f)) f = 0.f;   // NaN / huge coordinates: texel 0 (never out of bounds)
    int64_t i = (int64_t)f % (int64_t)n;
    return (uint32_t)(i < 0 ? i + n : i);
}
__device__ __forceinline__ float4 sample_texture(const TraceArgs& a, uint32_t k, float u, float v) {
    const uint4 ti = a.texinfo[k];
    const float x = u * (float)ti.y - 0.5f, y = v * (float)ti.z - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    const float fx = x - x0, fy = y - y0;
    const uint32_t ix = wrap_index(x0, ti.y), iy = wrap_index(y0, ti.z);
    const uint32_t ix1 = ix + 1 == ti.y ? 0u : ix + 1, iy1 = iy + 1 == ti.z ? 0u : iy + 1;
    const float4 t00 = texel(a, ti.x, ti.y, ix, iy), t10 = texel(a, ti.x, ti.y, ix1, iy);
    const float4 t01 = texel(a, ti.x, ti.y, ix, iy1), t11 = texel(a, ti.x, ti.y, ix1, iy1);
    const float4 top = make_float4(lerpf(t00.x, t10.x, fx), lerpf(t00.y, t10.y, fx), lerpf(t00.z, t10.z, fx),
                                   lerpf(t00.w, t10.w, fx));
    const float4 bot = make_float4(lerpf(t01.x, t11.x, fx), lerpf(t01.y, t11.y, fx), lerpf(t01.z, t11.z, fx),
                                   lerpf(t01.w, t11.w, fx));
    return make_float4(lerpf(top.x, bot.x, fy), lerpf(top.y, bot.y, fy), lerpf(top.z, bot.z, fy),
                       lerpf(top.w, bot.w, fy));
}

// getHitLoc (:15-19) + getNromalTexCoord (RayTraceHelper.hlsl:12-35) + renderPixel*specular
// (RayTraceRender.hlsl:16-29, RayTraceLaunch.hlsl:57-59) for the hit triangle only
// (the reference transforms all three vertices at every leaf it visits).
__device__ __forceinline__ HitInfo shade_hit_tri(const TraceArgs& a, uint32_t tri, f3 o, f3 d, float t) {
    HitInfo h;
    const float4* P = a.tclip + TCS * (size_t)tri;
    const float4 a0 = P[0], a1 = P[1], a2 = P[2];
    // vertex and material indices: the record's fourth float4 (k_morton), else the index arrays
    uint32_t vi[3], mi;
    if (TCS == 4) {
        const float4 a3 = P[3];
        vi[0] = __float_as_uint(a3.x); vi[1] = __float_as_uint(a3.y); vi[2] = __float_as_uint(a3.z);
        mi = __float_as_uint(a3.w);
    } else {
        vi[0] = a.idx[3 * (size_t)tri]; vi[1] = a.idx[3 * (size_t)tri + 1]; vi[2] = a.idx[3 * (size_t)tri + 2];
        mi = a.matidx[tri];
    }
    const f3 P0 = mk(a0.x, a0.y, a0.z), P1 = mk(a1.x, a1.y, a1.z), P2 = mk(a2.x, a2.y, a2.z);
    f3 n[3];
    float uv[3][2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float* v = a.verts + 8 * (size_t)vi[k];
        n[k] = xform_normal(a.cam + 16, mk(v[3], v[4], v[5]));
        uv[k][0] = v[6];
        uv[k][1] = v[7];
    }
    h.hitp = add(o, mul(d, t));
    const f3 v0 = sub(P0, h.hitp), v1 = sub(P1, h.hitp), v2 = sub(P2, h.hitp);
    const float a_0 = magnitude(cross(sub(P0, P1), sub(P0, P2)));
    const float w1 = magnitude(cross(v1, v2)) / a_0;
    const float w2 = magnitude(cross(v2, v0)) / a_0;
    const float w3 = magnitude(cross(v0, v1)) / a_0;
    const float tu = (uv[0][0] * w1 + uv[1][0] * w2) + uv[2][0] * w3;
    const float tv = (uv[0][1] * w1 + uv[1][1] * w2) + uv[2][1] * w3;
    h.nrm = add(add(mul(n[0], w1), mul(n[1], w2)), mul(n[2], w3));
    const Mat& m = a.mats[mi];
    h.textured = m.tex_num != -1;
    float tx = 1.f, ty = 1.f, tz = 1.f, tw = 1.f;   // RayTraceRender.hlsl:19
    if (h.textured && (uint32_t)m.tex_num < a.ntex) {   // :22-26 (no texture bound: white)
        const float4 t = sample_texture(a, (uint32_t)m.tex_num, tu, tv);
        tx = t.x; ty = t.y; tz = t.z; tw = t.w;
    }
    h.color = make_float4(sat(m.ambient[0] + m.diffuse[0] * tx) * m.specular[0],
                          sat(m.ambient[1] + m.diffuse[1] * ty) * m.specular[1],
                          sat(m.ambient[2] + m.diffuse[2] * tz) * m.specular[2],
                          sat(m.ambient[3] + m.diffuse[3] * tw) * m.specular[3]);
    h.shininess = m.shininess;
    h.alpha = m.alpha;
    h.optical_density = m.optical_density;
    return h;
}

// the same for sorted leaf best_leaf (its record holds the triangle index)
__device__ __forceinline__ HitInfo shade_hit(const TraceArgs& a, uint32_t best_leaf, f3 o, f3 d, float t) {
    return shade_hit_tri(a, __float_as_uint(a.leaf[4 * (size_t)best_leaf + 2].y) & ~LEAF_BIT, o, d, t);
}

// A hit record written through to memory (agent scope, 8 B): the certified walk's early shading reads and claims
// records from other XCDs while the walk runs, and a record left dirty in the writer's L2 would be written back over
// the claim (trace.hip RTBVH_EARLY_SHADE)
__device__ __forceinline__ void st_hitrec(float2* p, float2 v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p),
                       (unsigned long long)__float_as_uint(v.x) | (unsigned long long)__float_as_uint(v.y) << 32,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// the set lanes of mask below this lane (v_mbcnt: no 64-bit lane mask held in VGPRs)
__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
// wave-aggregated append: one atomic per wave, lanes keep their order
__device__ __forceinline__ uint32_t wave_append(bool active, uint32_t* counter) {
    const uint64_t mask = __ballot(active);
    if (mask == 0) return 0;
    const uint32_t lane = lane_id();
    const int leader = __ffsll((unsigned long long)mask) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
    return base + lane_rank(mask);
}
// the sum of v over the wave's 64 lanes, in every lane; and of each element of an array
template <class V> __device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <class V, int N> __device__ __forceinline__ void wave_sum(V (&v)[N]) {
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = wave_sum(v[k]);
}
// the ray of a queue entry (o = words 2..4, d = words 5..7, as two 16-B loads) and its reciprocal direction
__device__ __forceinline__ void load_ray(const RayQ* e, f3& o, f3& d, f3& inv) {
    const float4 q0 = reinterpret_cast<const float4*>(e)[0], q1 = reinterpret_cast<const float4*>(e)[1];
    o = mk(q0.z, q0.w, q1.x);
    d = mk(q1.y, q1.z, q1.w);
    inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
}

// counters: [base] internal visits, [base+1] leaf visits, [base+2] hits (base 2 primary,
// 5 bounce), [8] stack overflows / guard trips (also added to *overflow), [9] textured hits,
// [14] / [15] internal / leaf wave steps of the primary packet walks (one record fetch each),
// [16] / [17] bin entries of k_primary_binned and those it fetched a leaf record for
template <bool COUNT, bool BINS = false>
__device__ __forceinline__ void flush_counts(const TraceArgs& a, const Counts& c, uint32_t hits, uint32_t tex,
                                             int base) {
    unsigned long long v[7] = {c.internal, c.leaf, hits, c.overflow, tex, c.wint, c.wleaf};
    wave_sum(v);
    if (lane_id() == 0) {
        if (COUNT) {
            atomicAdd(&a.counters[base], v[0]);
            atomicAdd(&a.counters[base + 1], v[1]);
            atomicAdd(&a.counters[base + 2], v[2]);
            atomicAdd(&a.counters[9], v[4]);
            if (v[5] | v[6]) {   // wave steps of the primary packet walks, or bin entries (k_primary_binned)
                atomicAdd(&a.counters[base == 2 && BINS ? 16 : 14], v[5]);
                atomicAdd(&a.counters[base == 2 && BINS ? 17 : 15], v[6]);
            }
        }
        if (v[3]) {
            atomicAdd(&a.counters[8], v[3]);
            atomicAdd(a.overflow, v[3]);
        }
    }
}

// RayTraceLaunch.hlsl:40-86 for one pixel of the frame, from its closest hit (phit: sorted leaf bl
// at distance best): colour, intensity, the RayPresent records, and the reflection ray in e
// (returns whether it is live, i.e. traced by RayTraceReflection.hlsl:17-18)
// REC false: a trace without RayPresent records (a.refl_rec, a.refr_rec null; the binned pass's shading then
// holds its registers at 8 waves per SIMD)
// qdst: where a live ray goes, when the caller knows it before the shading (the binned pass: no RayQ held
// across the shading)
template <bool REC = true>
__device__ __forceinline__ bool primary_pixel(const TraceArgs& a, size_t out, f3 o, f3 d, bool phit, float best,
                                              uint32_t bl, uint32_t& hits, uint32_t& tex, RayQ& e,
                                              RayQ* qdst = nullptr) {
    float4 color;
    float intensity = 0.f;
    bool live = false;
    if (phit) {
        hits = 1;
        const HitInfo h = shade_hit(a, bl, o, d, best);
        tex = h.textured;
        intensity = h.shininess / 1000.f * 1;   // :48 (REFLECTION_DECAY 1)
        color = h.color;
        if (0 < intensity) {   // traced by RayTraceReflection.hlsl:17-18 only when > INTENSITY_MIN
            const f3 ro = add(h.hitp, mul(h.nrm, .001f));   // RAY_OFFSET .001
            const f3 rd = normalize(reflect(d, h.nrm));
            e.idx = (uint32_t)out;
            e.intensity = intensity;
            e.ox = ro.x; e.oy = ro.y; e.oz = ro.z;
            e.dx = rd.x; e.dy = rd.y; e.dz = rd.z;
            live = true;
            if (qdst) *qdst = e;
        }
        if (REC && a.refl_rec) {   // :48-67 (the ray is set only when the intensity is not 0)
            const bool rr = intensity != 0;
            put_record(a.refl_rec, out, intensity, rr, rr ? add(h.hitp, mul(h.nrm, .001f)) : o,
                       rr ? normalize(reflect(d, h.nrm)) : d, color);
        }
        if (REC && a.refr_rec) {   // :70-80, REFRACTION_DECAY 1
            const float ri = (1.f - h.alpha) * 1;
            const bool rr = ri != 0;
            put_record(a.refr_rec, out, ri, rr, rr ? sub(h.hitp, mul(h.nrm, .001f)) : o,
                       rr ? normalize(refract_hlsl(d, h.nrm, h.optical_density)) : d,
                       make_float4(1.f, 1.f, 1.f, 1.f));
        }
    } else {
        color = make_float4(.5f, .5f, .5f, 1.f);   // getBackground, :85-86
        if (REC && a.refl_rec) put_record(a.refl_rec, out, 0.f, false, o, d, color);   // clearRayPresent
        if (REC && a.refr_rec) put_record(a.refr_rec, out, 0.f, false, o, d, color);
    }
    a.color[out] = color;
    if (a.intensity) a.intensity[out] = intensity;
    return live;
}

// RayTraceLaunch.hlsl:6-93.  LIM: a run-time stack limit (rtbvh_config.stack_limit); without
// it the limit is the compiled capacity, a constant (a run-time limit kept in the walk loop
// costs the SGPR-bound packet walks a kernel-argument reload per step)
template <bool COUNT, int K, bool LIM>
__global__ __launch_bounds__(BLOCK, 8) void k_primary(TraceArgs a, RayQ* __restrict__ q, uint32_t* __restrict__ qcount,
                                                      int emit) {
    using PW = PrimaryWalk<K>;
    const int lim = LIM ? a.stack_limit : STACK_SIZE, lim4 = LIM ? a.stack_limit4 : STACK4;
    constexpr int PST = PW::WIDE ? 3 * (STACK4 + 1) : 3 * STACK_SIZE;   // per-wave packet stack words (+ sentinel)
    __shared__ uint32_t s_pst[PW::PACKET ? 4 * PST : 1];
    __shared__ uint32_t s_lst[PW::PACKET || PW::NB || LANE_LSB == 0 ? 1 : LANE_LSB * BLOCK];
    const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * 32 + w * 8 + (lane & 7);
    const uint32_t k = a.band0 + blockIdx.y * a.bstep;   // the rank's k-th band
    // behind k_primary_binned: trace only the blocks whose 32 x 32 screen tile overflowed its bins
    if (a.pb_gate && a.pb_gate[(((k * 8) >> 5) * a.pb_ntx + blockIdx.x + 1) * PB_NZ] <= a.pb_cap) return;
    const uint32_t band = a.band_list ? a.band_list[k] : k * a.nranks + a.rank;
    const uint32_t y = band * 8 + (lane >> 3);
    const bool valid = x < a.W && y < a.H;
    const size_t out = ((size_t)k * 8 + (lane >> 3)) * a.W + x;
    Counts c = {0, 0, 0, 0, 0};
    uint32_t hits = 0, tex = 0;
    bool live = false;
    RayQ e;
    const float hw = (float)(a.W >> 1), hh = (float)(a.H >> 1);
    const f3 o = mk(((float)x - hw) / 4.f, ((float)y - hh) / 4.f, 0.f);   // :23-24
    const f3 d = mk(0.f, 0.f, 1.f);
    const f3 inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
    float best = 0.f;
    uint32_t bl = 0;
    bool phit = false;
    if (PW::WIDE)     // whole wave, before any divergence
        phit = traverse_packet4<COUNT, PW::GUARD, PW::GUARD || LIM>(a.inner, a.leaf, a.T, o, d, inv, valid, lim4, best, bl, c,
                                            s_pst + w * PST);
    else if (PW::PACKET)
        phit = traverse_packet<COUNT, PW::NEAREST>(a.inner, a.leaf, a.T, o, d, inv, valid, lim, best, bl, c,
                                                   s_pst + w * PST);
    if (valid) {
        bool h = phit;
        if (PW::NB) {   // (all in scratch, the compiled capacity: the few rays of a certified trace)
            h = traverse_ref<COUNT>(true, a.inner, a.topo, a.nbox, a.leaf, a.T, o, d, inv, best, bl, c);
        } else if (!PW::PACKET) {
            h = traverse<COUNT, PW::NEAREST, LANE_LSB>(RecordTree{a.inner}, a.leaf, a.T, o, d, inv, lim, best, bl, c,
                                                       s_lst + threadIdx.x);
        }
        live = primary_pixel(a, out, o, d, h, best, bl, hits, tex, e);
    }
    const uint32_t slot = wave_append(emit && live, qcount);
    if (emit && live) q[slot] = e;
    flush_counts<COUNT>(a, c, hits, tex, 2);
}

// the trace's counters and bin counts zeroed by one launch instead of a memset each (blockIdx.y: the array)
__global__ __launch_bounds__(BLOCK) void k_zero(ZeroList z) {
    uint32_t* p = z.ptr[blockIdx.y];
    const size_t n = z.words[blockIdx.y];
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) p[i] = 0;
}

// ---- binned primary rays (RTBVH_FLAG_BINNED_PRIMARY) ----------------------------------------
// The primary rays are orthographic: pixel (x, y) is the ray o = ((x - W/2) / 4, (y - H/2) / 4, 0),
// d = (0, 0, 1) (RayTraceLaunch.hlsl:16-30).  The 4-wide packet walk (traverse_packet4) returns, per
// pixel, the lexicographic (t, leaf) minimum over the leaves whose box passes the axis-parallel test
// -- min.x < o.x < max.x, min.y < o.y < max.y (the general slab test for a box whose bit is set) --
// and whose triangle it hits; its box tests on the way down and its z pruning (min.z <= bound) only
// skip leaves that cannot beat the bound (containment).  On a regular pixel grid the
// pixels a box passes form a rectangle, which the build records exactly per leaf (rtbvh_device.h
// leaf_footprint).  So the same minimum is found level-synchronously at the leaves: every leaf is
// listed in the (32 x 32 screen tile, depth bucket) bins its rectangle covers (k_pb_bin, two passes
// streaming the leaves in slot order), then per tile (k_primary_binned) each listed leaf is tested
// against the pixels of its rectangle whose current bound its min.z does not exceed, nearest depth
// bucket first, the per-pixel (t, leaf) keys in LDS -- the bound carried from bucket to bucket.  Order
// only changes which tests the bound skips, never the minimum.  At C5: 13.7M (leaf, tile) entries,
// a third of them past the 8 x 8-block bound test, 35M triangle tests, all independent, in place of
// 17.9M dependent record fetches of 8x8-pixel packets.  k_pb_shade then writes k_primary's outputs
// (shading, RayPresent records, the bounce queue).  A tile whose bins overflowed the buffer is
// traced by k_primary (the per-lane nearest-first walk) behind these kernels (pb_gate).

#include "pb_bin.h"
// image row of the rank's compact row
__device__ __forceinline__ uint32_t pb_image_row(const TraceArgs& a, uint32_t crow) {
    const uint32_t k = crow >> 3;
    return (a.band_list ? a.band_list[k] : k * a.nranks + a.rank) * 8 + (crow & 7u);
}

template <bool FILL>
__global__ __launch_bounds__(BLOCK) void k_pb_bin(TraceArgs a, uint32_t* __restrict__ off,
                                                  uint32_t* __restrict__ cur, uint4* __restrict__ bins, uint32_t cap,
                                                  uint32_t ntx) {
    pb_bin_block<FILL>(a, blockIdx.x, off, cur, bins, cap, ntx);
}

// exclusive scan of the n bin counts in place, off[n] = the total, the fill cursors zeroed: blocks of
// PB_SCAN counts, first each block's total (k_pb_sums), then each block adds the totals of the blocks
// before it to its own scan (k_pb_scan; C5: 130,560 counts, 128 blocks)
constexpr uint32_t PB_SCAN = 1024;
__device__ __forceinline__ uint32_t block_sum_1024(uint32_t v, uint32_t* s_w) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    v = wave_sum(v);
    if (lane == 0) s_w[w] = v;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) t += s_w[k];
    return t;
}
__global__ __launch_bounds__(1024) void k_pb_sums(const uint32_t* __restrict__ off, uint32_t* __restrict__ sums,
                                                  uint32_t n) {
    __shared__ uint32_t s_w[16];
    const uint32_t i = blockIdx.x * PB_SCAN + threadIdx.x;
    const uint32_t t = block_sum_1024(i < n ? off[i] : 0u, s_w);
    if (threadIdx.x == 0) sums[blockIdx.x] = t;
}
__global__ __launch_bounds__(1024) void k_pb_scan(uint32_t* __restrict__ off, uint32_t* __restrict__ cur,
                                                  const uint32_t* __restrict__ sums, uint32_t n) {
    __shared__ uint32_t s_w[16], s_v[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    // the totals of the blocks before this one
    uint32_t p = 0;
    for (uint32_t k = tid; k < blockIdx.x; k += 1024) p += sums[k];
    const uint32_t before = block_sum_1024(p, s_v);
    const uint32_t i = blockIdx.x * PB_SCAN + tid;
    const uint32_t v = i < n ? off[i] : 0u;
    uint32_t x = v;   // inclusive scan over the wave, then over the waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if ((int)lane >= d) x += y;
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    uint32_t run = before + x - v;
    for (uint32_t k = 0; k < w; k++) run += s_w[k];
    if (i < n) { off[i] = run; cur[i] = 0; }
    if (i == n - 1) off[n] = run + v;
}

// one 32 x 32 tile of the rank's frame per workgroup: the (t, leaf) keys of its pixels in LDS and
// the largest bound of each 8 x 8 block.  The waves claim the tile's bins in batches of 64 entries
// (one per lane; nearest depth bucket first; the next batch's entries load while this one runs):
//  1. coarse: an entry whose min.z exceeds the largest bound of every block its rectangle touches
//     cannot win any of its pixels (C5: two thirds of the entries end here, before any leaf fetch);
//  2. the survivors' triangles (v0, e1, e2), one vector load per lane;
//  3. fine: per survivor, its rectangle's pixels as lanes; those whose bound min.z does not exceed go
//     to the wave's queue of (entry, pixel) tests;
//  4. the queue, 64 tests at a time (every lane a test: the triangle from its entry's lane by
//     ds_bpermute, the bound re-read), folded into the keys with an LDS atomic min;
//  then the block maxima are refreshed.  The keys go to `keys` (the frame's (t, leaf) per pixel);
//  k_pb_shade turns them into k_primary's outputs.
// A stale bound (another wave's newer key, a maximum refreshed later) only tests more, never less.
constexpr uint32_t PB_QCAP = 256;   // queued tests per wave
// a pixel's key slot: rows 40 keys (80 words, 16 banks) apart, so that the t words read by the lanes
// of an 8 x 8, 16 x 4 or 32 x 2 pixel block spread over the 32 odd banks two to a bank, the fewest
// (a 32-key row is 64 words: every row on the same banks, 8-way conflicts)
constexpr uint32_t PB_KS = 40;
__device__ __forceinline__ uint32_t pb_slot(uint32_t pi) { return (pi / PB_TILE) * PB_KS + (pi % PB_TILE); }
static_assert(PB_TILE == 32, "k_primary_binned: 10-bit pixel indices, 4 x 4 blocks of 8 x 8, a row per half-wave");
// RTBVH_PB_PROF builds: shader-clock cycles per phase of k_primary_binned, summed over the waves into
// counters[32..39] (read back as rtbvh_stats.trav_steps_log2[0..7]; scripts/pb_phases.py)
#ifdef RTBVH_PB_PROF
#define PB_T(i) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const uint64_t _t = clock64(); pt[i] += _t - pt_last; pt_last = _t; } while (0)
#else
#define PB_T(i) do { } while (0)
#endif
#ifndef RTBVH_PB_RASTER_BLOCK
#define RTBVH_PB_RASTER_BLOCK 256
#endif
constexpr uint32_t PB_RASTER_BLOCK = RTBVH_PB_RASTER_BLOCK;   // threads per tile of k_primary_binned
constexpr uint32_t PB_RASTER_BLOCK_SMALL = 512;   // ... for a small pass one frame at a time (launch_pb_pass)
// cost probes (A/B builds only, wrong frames): 1 = no fine phase, 2 = the fine phase's tests skipped
#ifndef RTBVH_PB_PROBE
#define RTBVH_PB_PROBE 0
#endif
// CERT (the certified pass): the binned pass tested every leaf whose triangle could be
// accepted below a pixel's bound (its depth key, margin.h); a pixel's (t, leaf) is the reference's when
// the leaf's own box passes the reference slab test with the bound t (k_bounce_shade's leaf_certified,
// here from the leaf record's box).  Pixels that fail it go to the re-trace list (redo: compact pixel
// index) and are left to k_primary_redo, outside the block's bounce-queue claim.
// One tile of k_pb_shade's work over NT threads, the pixels' keys from key_at(compact row, x).  s_cnt: 16
// words of LDS, s_mask: 2 x 16 words, s_base: one.  The 16 sub-tiles of 8 x 8 pixels go to the waves in
// turn; a first pass counts each one's live rays (and certificates) into LDS, the tile claims its queue
// range, then a second pass shades them (no per-sub-tile registers held across the claim).
// (Inlined: out of line, A/B round 5, the fused binned pass took 1.07 ms against 0.86.)
// The kernel's TraceArgs (its first argument) read again from the kernel-argument segment where they are used:
// scalar loads the compiler cannot hoist out of a loop (held in SGPRs across the shading loop's iterations they
// spilled into VGPR lanes, and the shading's VGPRs to scratch)
__device__ __forceinline__ const TraceArgs& kernel_trace_args() {
    auto p = (const __attribute__((address_space(4))) TraceArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const TraceArgs*)p;
}
template <bool COUNT, bool CERT, uint32_t NT, bool REC, class KeyAt>
__device__ __forceinline__ void pb_shade_tile(const TraceArgs& a, uint32_t rows, KeyAt&& key_at, RayQ* __restrict__ q,
                                              uint32_t* __restrict__ qcount, int emit, uint32_t* __restrict__ redo,
                                              uint32_t* __restrict__ redo_count, uint32_t* s_cnt, uint64_t* s_mask,
                                              uint32_t& s_base) {
    const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
    const uint32_t X0 = blockIdx.x * PB_TILE, C0 = blockIdx.y * PB_TILE;
    constexpr uint32_t NST = (PB_TILE / 8) * (PB_TILE / 8) / (NT / 64);   // sub-tiles per wave
    constexpr uint32_t NSUB = (PB_TILE / 8) * (PB_TILE / 8);
    const float hw = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint((float)(a.W >> 1))));
    const float hh = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint((float)(a.H >> 1))));
    const auto pixel = [&](uint32_t i, uint32_t& x, uint32_t& crow) {
        const uint32_t st = w + i * (NT / 64);
        x = X0 + (st % (PB_TILE / 8)) * 8 + (lane & 7u);
        crow = C0 + (st / (PB_TILE / 8)) * 8 + (lane >> 3);
        return x < a.W && crow < rows;
    };
    // the live reflection rays: hit, and the hit material's shininess > 0
#pragma unroll 1
    for (uint32_t i = 0; i < NST; i++) {
        uint32_t x, crow;
        const bool valid = pixel(i, x, crow);
        const uint64_t key = valid ? key_at(crow, x) : NO_HIT;
        bool live = false, flag = false;
        if (CERT && key != NO_HIT) {   // the certificate: the leaf's box, the reference slab test at t
            const float4 b2 = a.leaf[4 * (size_t)(uint32_t)key + 2], b3 = a.leaf[4 * (size_t)(uint32_t)key + 3];
            const f3 o = mk(((float)x - hw) / 4.f, ((float)pb_image_row(a, crow) - hh) / 4.f, 0.f);
            const f3 d = mk(0.f, 0.f, 1.f);
            float tm;
            flag = !ray_box(o, mk(1.f / d.x, 1.f / d.y, 1.f / d.z), b2.z, b2.w, b3.x, b3.y, b3.z, b3.w, true,
                            key_t(key), tm);
        }
        if (emit && key != NO_HIT && !flag) {
            const uint32_t tri = __float_as_uint(a.leaf[4 * (size_t)(uint32_t)key + 2].y) & ~LEAF_BIT;
            const uint32_t mi = TCS == 4 ? __float_as_uint(a.tclip[TCS * (size_t)tri + 3].w) : a.matidx[tri];
            live = 0 < a.mats[mi].shininess / 1000.f * 1;
        }
        const uint64_t livem = __ballot(live), flagm = CERT ? __ballot(flag) : 0ull;
        const uint32_t st = w + i * (NT / 64);
        if (lane == 0) {
            s_cnt[st] = (uint32_t)__popcll(livem);
            s_mask[st] = livem;
            s_mask[NSUB + st] = flagm;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < NSUB; k++) {
            const uint32_t v = s_cnt[k];
            s_cnt[k] = run;
            run += v;
        }
        s_base = run && emit ? atomicAdd(qcount, run) : 0u;
    }
    __syncthreads();
    const uint32_t sbase = (uint32_t)__builtin_amdgcn_readfirstlane(s_base);
    uint32_t hits = 0, tex = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < NST; i++) {
        uint32_t x, crow;
        const bool valid = pixel(i, x, crow);
        const uint32_t st = w + i * (NT / 64);
        // (wave-uniform: into SGPRs, so the shading below keeps its VGPRs)
        const auto uni64 = [](uint64_t v) {
            return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v) |
                   (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32;
        };
        const uint64_t livem = uni64(s_mask[st]), flagm = CERT ? uni64(s_mask[NSUB + st]) : 0ull;
        const uint32_t qb = sbase + (uint32_t)__builtin_amdgcn_readfirstlane(s_cnt[st]);
        const bool flag = CERT && ((flagm >> lane) & 1u);
        if (CERT && flagm) {   // (rare) the re-trace list, one atomic per wave
            const uint32_t slot = wave_append(flag, redo_count);
            if (flag) redo[slot] = crow * a.W + x;
        }
        if (valid && !flag) {
            const TraceArgs& a = kernel_trace_args();   // (a is the kernel's first argument: k_primary_binned, k_pb_shade)
            const uint64_t key = key_at(crow, x);
            const f3 o = mk(((float)x - hw) / 4.f, ((float)pb_image_row(a, crow) - hh) / 4.f, 0.f);
            const bool phit = key != NO_HIT;
            uint32_t h1 = 0, t1 = 0;
            RayQ e;
            // (the live rays were counted above: this lane's queue entry is known before the shading)
            RayQ* dst = emit && ((livem >> lane) & 1u) ? q + qb + lane_rank(livem)
                                                        : nullptr;
            (void)primary_pixel<REC>(a, (size_t)crow * a.W + x, o, mk(0.f, 0.f, 1.f), phit, phit ? key_t(key) : 0.f,
                                     phit ? (uint32_t)key : 0u, h1, t1, e, dst);
            hits += h1;
            tex += t1;
        }
    }
    if (COUNT) {
        Counts c = {0, 0, 0, 0, 0};
        flush_counts<COUNT>(a, c, hits, tex, 2);
    }
}
// FUSE (the default; RTBVH_PB_FUSE=0 builds the separate k_pb_shade launch, A/B): the tile's shading (k_pb_shade's work, pb_shade_tile) at the end of the
// same workgroup, from the keys in LDS -- no keys round trip through HBM, one launch fewer, and a tile's
// dependent shading gathers run beside other tiles' rasterisation on the CU
#ifndef RTBVH_PB_FUSE
#define RTBVH_PB_FUSE 1
#endif
#ifndef RTBVH_PB_WAVES
#define RTBVH_PB_WAVES 8   // k_primary_binned's launch bounds: 8 waves per SIMD (64 VGPRs, some spilled) beat 6
                                   // and 5 -- round 5, primary pass 0.87-0.89 / 0.91-0.93 / 0.98 ms with 37 / 16 /
                                   // no VGPRs spilled.  Since then, by the compiler's resource remarks at 8 waves:
                                   // 5 spilled in the bench's instance (certified, no counts, no records, 256
                                   // threads a tile), 10-16 in the instances with counts or records
#endif
// RB: threads per tile -- PB_RASTER_BLOCK, or PB_RASTER_BLOCK_SMALL for a small pass traced one frame at a time
// (api.hip: a rank's ~1,000 tiles then all run at once, and more waves per tile shorten the longest tile)
template <bool COUNT, bool CERT = false, bool FUSE = false, bool REC = true, uint32_t RB = PB_RASTER_BLOCK>
__global__ __launch_bounds__(RB, RTBVH_PB_WAVES) void k_primary_binned(TraceArgs a, const uint32_t* __restrict__ off,
                                                             const uint4* __restrict__ bins, uint32_t cap,
                                                             uint32_t ntx, uint32_t rows,
                                                             unsigned long long* __restrict__ keys, RayQ* __restrict__ q,
                                                             uint32_t* __restrict__ qcount, int emit,
                                                             uint32_t* __restrict__ redo,
                                                             uint32_t* __restrict__ redo_count) {
    __shared__ unsigned long long s_key[PB_TILE * PB_KS];
    __shared__ float s_bmax[(PB_TILE / 8) * (PB_TILE / 8)];
    __shared__ uint32_t s_q[RB / 64][PB_QCAP];
    __shared__ uint32_t s_next;
    const uint32_t* s_t = reinterpret_cast<const uint32_t*>(s_key);   // [2 slot + 1]: a pixel's bound (t bits)
    const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
    const uint32_t tile = blockIdx.y * ntx + blockIdx.x;
    const uint32_t X0 = blockIdx.x * PB_TILE, C0 = blockIdx.y * PB_TILE;
    const uint32_t beg = off[tile * PB_NZ], end = off[(tile + 1) * PB_NZ];
    if (end > cap) return;   // bins overflowed: k_primary traces this tile (pb_gate)
#ifdef RTBVH_PB_PROF
    uint64_t pt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pt_last = clock64();
#endif
    // keys of the pixels outside the frame (or the rank's rows) start at t = 0: no entry covers them,
    // and they never raise a block's largest bound
    for (uint32_t i = threadIdx.x; i < PB_TILE * PB_KS; i += RB)
        s_key[i] = X0 + i % PB_KS < a.W && C0 + i / PB_KS < rows ? NO_HIT : 0ull;
    if (threadIdx.x < (PB_TILE / 8) * (PB_TILE / 8)) s_bmax[threadIdx.x] = INFINITY;
    if (threadIdx.x == 0) s_next = 0;
    __syncthreads();
    const float hw = (float)(a.W >> 1), hh = (float)(a.H >> 1);
    const f3 d = mk(0.f, 0.f, 1.f);
    const f3 inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
    uint32_t* sq = s_q[w];
    Counts c = {0, 0, 0, 0, 0};
    const uint32_t nbatch = (end - beg + 63) / 64;
    const auto claim = [&]() {
        uint32_t b = 0;
        if (lane == 0) b = atomicAdd(&s_next, 1u);
        return (uint32_t)__builtin_amdgcn_readfirstlane(b);
    };
    const auto fetch = [&](uint32_t b) {
        const uint32_t e = beg + b * 64 + lane;
        return b < nbatch && e < end ? bins[e] : make_uint4(0, 0, 0, INVALID);
    };
    uint32_t bn = claim();
    uint4 fn = fetch(bn);
    PB_T(7);
    while (bn < nbatch) {
        const uint4 f = fn;
        bn = claim();
        fn = fetch(bn);   // the next batch's entries, in flight during this one
        const bool ve = f.w != INVALID;
        const uint32_t j = f.w & ~LEAF_BIT;
        const bool gen = ve && (f.w & LEAF_BIT) != 0;
        // the entry's rectangle in tile coordinates (it overlaps the tile by construction)
        const int rx0 = max((int)(f.x & 0xFFFFu), (int)X0) - (int)X0, rx1 = min((int)(f.x >> 16), (int)X0 + 31) - (int)X0;
        const int ry0 = max((int)(f.y & 0xFFFFu), (int)C0) - (int)C0, ry1 = min((int)(f.y >> 16), (int)C0 + 31) - (int)C0;
        const float zmin = __uint_as_float(f.z);
        PB_T(0);
        // 1: coarse
        bool surv = false;
        if (ve) {
            float m = -INFINITY;
            for (int by = ry0 >> 3; by <= ry1 >> 3; by++)
                for (int bx = rx0 >> 3; bx <= rx1 >> 3; bx++) m = fmaxf(m, s_bmax[by * (PB_TILE / 8) + bx]);
            surv = gen || zmin <= m;
        }
        if (COUNT) {
            const uint32_t nv = (uint32_t)__popcll(__ballot(ve)), ns = (uint32_t)__popcll(__ballot(surv));
            if (lane == 0) { c.wint += nv; c.wleaf += ns; }
        }
        // 2: the survivors' triangles
        float4 r0 = make_float4(0, 0, 0, 0), r1 = r0, r2 = r0;
        if (surv) {
            const float4* r = a.leaf + 4 * (size_t)j;
            r0 = r[0]; r1 = r[1]; r2 = r[2];
        }
        PB_T(1);
        // 4: the queued tests, every lane one (entry lane k, pixel pi)
        uint32_t qn = 0;
        const auto flush = [&]() {
            PB_T(3);
            for (uint32_t q0 = 0; q0 < (RTBVH_PB_PROBE == 2 ? 0u : qn); q0 += 64) {
                const bool act = q0 + lane < qn;
                const uint32_t v = act ? sq[q0 + lane] : 0u;
                const int k = (int)(v >> 10);
                const uint32_t pi = v & 1023u;
#define BP(x) __uint_as_float((uint32_t)__shfl((int)__float_as_uint(x), k, 64))
                const f3 p0 = mk(BP(r0.x), BP(r0.y), BP(r0.z)), e1 = mk(BP(r0.w), BP(r1.x), BP(r1.y));
                const f3 e2 = mk(BP(r1.z), BP(r1.w), BP(r2.x));
                const float kz = BP(zmin);
#undef BP
                const uint32_t kw = (uint32_t)__shfl((int)f.w, k, 64);
                const uint32_t kj = kw & ~LEAF_BIT;
                const bool kg = (kw & LEAF_BIT) != 0;
                const uint32_t px = pi % PB_TILE, py = pi / PB_TILE;
                const f3 o = mk(((float)(X0 + px) - hw) / 4.f, ((float)pb_image_row(a, C0 + (act ? py : 0u)) - hh) / 4.f,
                                0.f);
                bool in = false;
                if (act) {
                    if (kg) {   // the general slab test on the leaf's box, no pruning (traverse_packet4's leaf step)
                        const float4 b2 = a.leaf[4 * (size_t)kj + 2], b3 = a.leaf[4 * (size_t)kj + 3];
                        float tt;
                        in = ray_box_xy(o, inv, f2v{b2.z, b2.w}, f2v{b3.y, b3.z}, b3.x, b3.w, false, 0.f, tt);
                    } else {
                        in = kz <= __uint_as_float(s_t[2 * pb_slot(pi) + 1]);
                    }
                }
                if (COUNT) c.leaf += in;
                const float t = ray_triangle_flat(o, d, p0, e1, e2, in);
                if (t != -1.f) atomicMin(&s_key[pb_slot(pi)], (unsigned long long)__float_as_uint(t) << 32 | kj);
            }
            qn = 0;
            PB_T(4);
        };
        // 3: fine, survivor by survivor
        for (uint64_t todo = RTBVH_PB_PROBE == 1 ? 0ull : __ballot(surv); todo; todo &= todo - 1) {
            const int k = __ffsll((unsigned long long)todo) - 1;
            const bool sg = __builtin_amdgcn_readlane((int)gen, k) != 0;
            const int sx0 = __builtin_amdgcn_readlane(rx0, k), sx1 = __builtin_amdgcn_readlane(rx1, k);
            const int sy0 = __builtin_amdgcn_readlane(ry0, k), sy1 = __builtin_amdgcn_readlane(ry1, k);
            const float sz = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(zmin), k));
            const int lw = sx1 - sx0 + 1;
            const int cs = lw <= 8 ? 3 : lw <= 16 ? 4 : 5;   // lanes as 8x8, 16x4 or 32x2 pixels
            const int col = (int)(lane & ((1u << cs) - 1)), px = sx0 + col;
            for (int y0 = sy0; y0 <= sy1; y0 += 64 >> cs) {
                const int y = y0 + (int)(lane >> cs);
                const bool ok = col < lw && y <= sy1;
                const uint32_t pi = (uint32_t)(y * (int)PB_TILE + px);
                const bool need = ok && (sg || sz <= __uint_as_float(s_t[2 * pb_slot(pi) + 1]));
                const uint64_t nm = __ballot(need);
                if (qn + (uint32_t)__popcll(nm) > PB_QCAP) flush();
                if (need) sq[qn + lane_rank(nm)] = (uint32_t)k << 10 | pi;
                qn += (uint32_t)__popcll(nm);
            }
        }
        flush();
        PB_T(3);
        // the block maxima from the keys (pixels outside the frame hold t = 0): lane l reads column
        // l % 32 of rows l / 32, + 2, + 4, ... (two whole rows per read: 2-way bank conflicts at most),
        // one running maximum per block row, then the maxima of the 8 lanes of a block column and of
        // the two half-waves
        float m[PB_TILE / 8] = {0.f, 0.f, 0.f, 0.f};
        const uint32_t* bt = s_t + 2 * ((lane / 32) * PB_KS + lane % 32) + 1;
#pragma unroll
        for (uint32_t r = 0; r < PB_TILE / 2; r++) m[r / 4] = fmaxf(m[r / 4], __uint_as_float(bt[2 * (2 * r * PB_KS)]));
#pragma unroll
        for (uint32_t by = 0; by < PB_TILE / 8; by++) {
            m[by] = fmaxf(m[by], __shfl_xor(m[by], 1, 64));
            m[by] = fmaxf(m[by], __shfl_xor(m[by], 2, 64));
            m[by] = fmaxf(m[by], __shfl_xor(m[by], 4, 64));
            m[by] = fmaxf(m[by], __shfl_xor(m[by], 32, 64));
        }
        if (lane < PB_TILE && (lane & 7u) == 0) {
#pragma unroll
            for (uint32_t by = 0; by < PB_TILE / 8; by++) s_bmax[by * (PB_TILE / 8) + lane / 8] = m[by];
        }
        PB_T(5);
    }
    __syncthreads();
    if (FUSE) {
        __shared__ uint32_t s_cnt[(PB_TILE / 8) * (PB_TILE / 8)];
        __shared__ uint64_t s_mask[2 * (PB_TILE / 8) * (PB_TILE / 8)];
        __shared__ uint32_t s_base;
        pb_shade_tile<COUNT, CERT, RB, REC>(
            a, rows, [&](uint32_t crow, uint32_t x) { return s_key[(crow - C0) * PB_KS + (x - X0)]; }, q, qcount, emit,
            redo, redo_count, s_cnt, s_mask, s_base);
    } else {
        // the tile's keys, row segments of 32 pixels
        for (uint32_t i = threadIdx.x; i < PB_TILE * PB_TILE; i += RB) {
            const uint32_t px = i % PB_TILE, py = i / PB_TILE;
            if (X0 + px < a.W && C0 + py < rows) keys[(size_t)(C0 + py) * a.W + X0 + px] = s_key[py * PB_KS + px];
        }
    }
#ifdef RTBVH_PB_PROF
    PB_T(6);
    if (lane == 0)
        for (int i = 0; i < 8; i++) atomicAdd(&a.counters[32 + i], (unsigned long long)pt[i]);
#endif
    flush_counts<COUNT, true>(a, c, 0, 0, 2);
}

// k_primary's outputs from the binned pass's keys, one 32 x 32 tile per block (a wave takes its
// 8 x 8 sub-tiles w, w + 4, ...).  The reflection rays go to the bounce queue with ONE atomic per
// block: its live rays are counted first (hit and shininess > 0, RayTraceLaunch.hlsl:48 and
// RayTraceReflection.hlsl:17-18), the block's base claimed, then every pixel shaded and its ray
// written at base + its rank.  (One atomic per wave -- k_primary's wave_append -- is 130K claims on
// one counter per C5 frame, ~1.2 ms at the ~100 claims per us one address takes.)  Tiles whose bins
// overflowed return (k_primary traced them).
// (a 1024-thread block, one pixel per thread: 256 threads with four pixels each held 86 VGPRs,
// 5 waves per SIMD, for the shading's dependent gathers)
#ifndef RTBVH_PB_SHADE_BLOCK
#define RTBVH_PB_SHADE_BLOCK 1024
#endif
constexpr uint32_t PB_SHADE_BLOCK = RTBVH_PB_SHADE_BLOCK;
template <bool COUNT, bool CERT>
__global__ __launch_bounds__(PB_SHADE_BLOCK, 8) void k_pb_shade(TraceArgs a, const uint32_t* __restrict__ off, uint32_t cap,
                                                    uint32_t ntx, uint32_t rows,
                                                    const unsigned long long* __restrict__ keys, RayQ* __restrict__ q,
                                                    uint32_t* __restrict__ qcount, int emit,
                                                    uint32_t* __restrict__ redo, uint32_t* __restrict__ redo_count) {
    __shared__ uint32_t s_cnt[(PB_TILE / 8) * (PB_TILE / 8)];
    __shared__ uint64_t s_mask[2 * (PB_TILE / 8) * (PB_TILE / 8)];
    __shared__ uint32_t s_base;
    const uint32_t tile = blockIdx.y * ntx + blockIdx.x;
    if (off[(tile + 1) * PB_NZ] > cap) return;
    pb_shade_tile<COUNT, CERT, PB_SHADE_BLOCK, true>(
        a, rows, [&](uint32_t crow, uint32_t x) { return keys[(size_t)crow * a.W + x]; }, q, qcount, emit, redo,
        redo_count, s_cnt, s_mask, s_base);
}

// The reference-order re-trace of the pixels a certified primary pass flagged (redo: compact pixel
// indices crow * W + x): the exact findCollision DFS per pixel (traverse), then k_primary's outputs
// (primary_pixel) and the bounce queue.  A fixed grid over the count on the device.
template <bool COUNT>
__global__ __launch_bounds__(BLOCK) void k_primary_redo(TraceArgs a, const uint32_t* __restrict__ redo,
                                                        const uint32_t* __restrict__ redo_count, RayQ* __restrict__ q,
                                                        uint32_t* __restrict__ qcount, int emit) {
    const uint32_t n = *redo_count;
    Counts c = {0, 0, 0, 0, 0};
    uint32_t hits = 0, tex = 0;
    const float hw = (float)(a.W >> 1), hh = (float)(a.H >> 1);
    const f3 d = mk(0.f, 0.f, 1.f);
    const f3 inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
    for (uint32_t base = blockIdx.x * BLOCK; base < n; base += gridDim.x * BLOCK) {
        const uint32_t i = base + threadIdx.x;
        bool live = false;
        RayQ e;
        if (i < n) {
            const uint32_t p = redo[i], crow = p / a.W, x = p % a.W;
            const f3 o = mk(((float)x - hw) / 4.f, ((float)pb_image_row(a, crow) - hh) / 4.f, 0.f);
            float best;
            uint32_t bl, h1 = 0, t1 = 0;
            const bool h = traverse_ref<COUNT>(a, o, d, inv, best, bl, c);
            live = primary_pixel(a, p, o, d, h, best, bl, h1, t1, e);
            hits += h1;
            tex += t1;
        }
        const uint32_t slot = wave_append(emit && live, qcount);
        if (emit && live) q[slot] = e;
    }
    flush_counts<COUNT>(a, c, hits, tex, 2);
}

// RayTraceReflection.hlsl:6-62 over the compacted queue of live rays (in `perm`
// order when the queue was sorted for coherence), one ray per lane
template <bool COUNT, bool NEAREST, bool LIM>
__global__ __launch_bounds__(BLOCK, 8) void k_bounce(TraceArgs a, const RayQ* __restrict__ qin,
                                                     const uint32_t* __restrict__ qin_count,
                                                     const uint32_t* __restrict__ perm, RayQ* __restrict__ qout,
                                                     uint32_t* __restrict__ qout_count, int emit) {
    __shared__ uint32_t s_lst[LANE_LSB == 0 ? 1 : LANE_LSB * BLOCK];
    const uint32_t n = *qin_count;
    Counts c = {0, 0, 0, 0, 0};
    uint32_t hits = 0, tex = 0;
    for (uint32_t base = blockIdx.x * BLOCK; base < n; base += gridDim.x * BLOCK) {
        const uint32_t i = base + threadIdx.x;
        bool live = false;
        RayQ e;
        if (i < n) {
            e = qin[perm ? perm[i] : i];
            f3 o, d, inv;
            load_ray(&e, o, d, inv);
            float best;
            uint32_t bl;
            float4 col = a.color[e.idx];
            float intensity = e.intensity;
            const int lim = LIM ? a.stack_limit : STACK_SIZE;
#ifdef RTBVH_BOUNCE_PROBE   // cost probes (A/B builds, wrong frames): 1 no walk (every ray misses), 2 no shading
            const bool th = RTBVH_BOUNCE_PROBE == 1 ? false
                                                    : traverse<COUNT, NEAREST, LANE_LSB>(RecordTree{a.inner}, a.leaf, a.T, o,
                                                          d, inv, lim, best, bl, c, s_lst + threadIdx.x);
            if (RTBVH_BOUNCE_PROBE == 2 && th) {
                hits++;
                col = make_float4(best, (float)bl, 0.f, 1.f);
            } else if (th) {
#else
            if (traverse<COUNT, NEAREST, LANE_LSB>(RecordTree{a.inner}, a.leaf, a.T, o, d, inv, lim, best, bl, c,
                                                   s_lst + threadIdx.x)) {
#endif
                hits++;
                const HitInfo h = shade_hit(a, bl, o, d, best);
                tex += h.textured;
                col = make_float4(lerpf(col.x, h.color.x, intensity), lerpf(col.y, h.color.y, intensity),
                                  lerpf(col.z, h.color.z, intensity), lerpf(col.w, h.color.w, intensity));
                intensity *= h.shininess / 1000.f * 1;
                const f3 ro = add(h.hitp, mul(h.nrm, .0001f));   // RAY_OFFSET .0001
                const f3 rd = normalize(reflect(d, h.nrm));
                e.intensity = intensity;
                e.ox = ro.x; e.oy = ro.y; e.oz = ro.z;
                e.dx = rd.x; e.dy = rd.y; e.dz = rd.z;
                live = 0 < intensity;
            } else {
                col = make_float4(lerpf(col.x, .5f, intensity), lerpf(col.y, .5f, intensity),
                                  lerpf(col.z, .5f, intensity), lerpf(col.w, 1.f, intensity));
                intensity = 0.f;
            }
            a.color[e.idx] = col;
            if (a.intensity) a.intensity[e.idx] = intensity;
        }
        const uint32_t slot = wave_append(emit && live, qout_count);
        if (emit && live) qout[slot] = e;
    }
    flush_counts<COUNT>(a, c, hits, tex, 5);
}

// ---- bounce pass split in two: persistent traversal with lane refill + shading ----
// The one-ray-per-lane bounce kernel keeps a wave until its slowest ray is done:
// PMC on C5 showed ~12 of 64 lanes active per traversal step (1.6e8 wave loads for
// 4.7e8 lane visits).  Here each lane that finishes its ray takes the next one from
// the queue (one atomic per wave per refill, Aila & Laine's dynamic fetch), so the
// wave stays full; the finished ray's (t, leaf) goes to a hit record, and the
// shading runs afterwards as a plain one-thread-per-ray kernel (k_bounce_shade).
// Per-lane traversal state and visit order are exactly those of traverse().
// A wave refills when at least REFILL_MIN lanes are idle.  A/B on C5 (bounce pass):
// 4 -> 15.6 ms, 8 -> 9.2, 16 -> 5.5, 24 -> 4.13, 32 -> 3.87, 40 -> 3.84, 48 -> 3.90,
// 64 -> 5.36 (the single work counter's atomic contention below 32).  Round 2's walk, bounce stage
// with shading: 8 -> 2.67 ms, 16 -> 2.57, 24 -> 2.59, 32 -> 2.62.
// Work counters: the queue is cut into NEXT_SEGS contiguous segments, each with its own
// counter on its own 128-B line.  Workgroup b runs on XCD b % 8 (round-robin dispatch); its
// waves claim from the segments of their XCD first (starting at one picked by b / 8), then from
// the other XCDs' in turn.  A single counter serialised the claims of all 8192 waves (~88 per
// us), which is what kept REFILL_MIN from going lower; and an XCD's waves now walk rays of
// neighbouring queue positions (neighbouring pixels), whose upper-tree nodes its L2 shares.
#ifndef RTBVH_REFILL_MIN
#define RTBVH_REFILL_MIN 16
#endif
constexpr uint32_t REFILL_MIN = RTBVH_REFILL_MIN;
constexpr uint32_t XCDS = 8;
constexpr uint32_t SEGS_PER_XCD = NEXT_SEGS >= XCDS ? NEXT_SEGS / XCDS : 1;
__device__ __forceinline__ uint32_t claim_segment(uint32_t k) {   // the wave's k-th segment
    if (NEXT_SEGS < XCDS) return k;
    const uint32_t xcd = blockIdx.x % XCDS, sub = (blockIdx.x / XCDS) % SEGS_PER_XCD;
    const uint32_t g = (xcd + k / SEGS_PER_XCD) % XCDS;
    return g * SEGS_PER_XCD + (sub + k) % SEGS_PER_XCD;
}
// segment seg of a queue of n rays: positions [s0, s0 + len)
__device__ __forceinline__ void segment_bounds(uint32_t n, uint32_t seg, uint32_t& s0, uint32_t& len) {
    s0 = (uint32_t)((uint64_t)n * seg / NEXT_SEGS);
    len = (uint32_t)((uint64_t)n * (seg + 1) / NEXT_SEGS) - s0;
}
// The refill of a persistent walk (all lanes converged; has: this lane holds a ray).  Once REFILL_MIN lanes are
// idle the wave claims that many positions of its current segment with one atomic, and start(p) hands queue
// position p to each idle lane that got one.  Every refill either hands out rays or moves on to the next segment
// (the last one sets `drained`), so a wave with no ray left comes back here until the queue is drained.
struct Refill {
    bool drained = false;
    uint32_t kseg = 0;   // segments claimed from so far (wave-uniform)
};
template <class Start>
__device__ __forceinline__ void refill_claim(Refill& rf, uint32_t* __restrict__ next, uint32_t n, bool has,
                                             Start&& start) {
    const uint64_t idle = __ballot(!has);
    const uint32_t nidle = (uint32_t)__popcll(idle);
    if (!rf.drained && (nidle >= REFILL_MIN || nidle == 64)) {
        const uint32_t seg = claim_segment(rf.kseg);
        uint32_t s0, len;
        segment_bounds(n, seg, s0, len);
        uint32_t base = 0;
        if (lane_id() == 0) base = atomicAdd(next + NEXT_STRIDE * seg, nidle);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base + nidle >= len && ++rf.kseg == NEXT_SEGS) rf.drained = true;   // segment (and the last) used up
        if (!has) {
            const uint32_t p = base + lane_rank(idle);
            if (p < len) start(s0 + p);
        }
    }
}

__device__ __forceinline__ void sort2(float& ta, uint32_t& ia, float& tb, uint32_t& ib) {
    const bool sw = tb < ta;
    const float t = sw ? tb : ta;
    const uint32_t i = sw ? ib : ia;
    tb = sw ? ta : tb;
    ib = sw ? ia : ib;
    ta = t;
    ia = i;
}

// A 16-bit key for an entry distance t that never exceeds it: the upper half of max(t, 0)
// (fmaxf drops NaN).  Positive t is truncated (rounded down); t <= 0 becomes 0, which is below
// every best distance (a hit's t > EPSILON), as t is: an entry is dropped on pop only when the
// exact test would drop it too.  One v_max_f32; the store takes the high half (the first
// form rounded negative t away from zero: six VALU and two SALU per push).
__device__ __forceinline__ uint16_t bf16_down(float t) { return (uint16_t)(__float_as_uint(fmaxf(t, 0.f)) >> 16); }
__device__ __forceinline__ float bf16_up(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// Walk modes of k_bounce_trav: 0 reference order, 1 nearest-first (binary records), 2 the
// 4-wide nearest-first walk on the quantized nodes (qn, rtbvh_device.h QNode: one 64-B node
// per 4-wide step; a node without a finite grid falls back to its exact record pair).
// Binary modes keep the stack entries [0, SB) in LDS, [entry][lane] (a wave's lanes hit
// 64 distinct banks whatever their depths), and only deeper entries in scratch: the
// all-scratch stack of 8192 resident waves (17 KB each) does not fit in L2 and PMC
// showed ~3.6 GB of stack write-back per C5 bounce pass.  The 4-wide walk keeps
// (node, entry distance) entries [0, SW) in LDS as a node id and the distance as a bf16
// rounded toward -inf (6 B each; the pop's prune test on the rounded-down distance keeps
// every entry the exact test keeps), deeper entries as full pairs in scratch.
constexpr int SB = 16;   // 16 x 4 B x 256 lanes = 16 KB per block
// the binary modes' stack (a Stack of the shared step): `col`: this lane's LDS column, entry k at col[k * BLOCK];
// `deep`: the kernel's scratch array of the entries [SB, STACK_SIZE)
struct BlockStack {
    uint32_t *col, *deep;
    __device__ __forceinline__ void store(int k, uint32_t v) {
        if (k < SB) col[k * BLOCK] = v;
        else deep[k - SB] = v;
    }
    __device__ __forceinline__ uint32_t load(int k) const { return k < SB ? col[k * BLOCK] : deep[k - SB]; }
};
// 13 x 6 B x 256 lanes = 19.5 KB per block: 8 blocks per CU in 160 KB.  A/B (C5 bounce stage):
// 8 entries 2.75-2.77 ms (deeper entries go to scratch), 12 2.50-2.55, 13 2.47-2.52, 14 2.51-2.53
// (7 blocks per CU)
#ifndef RTBVH_SW
#define RTBVH_SW 13
#endif
constexpr int SW = RTBVH_SW;
static_assert(SW * 6 * 256 * 8 <= 160 * 1024, "the 4-wide bounce walk's LDS stack: 8 blocks per CU");

// ---- the slack test of a quantized node --------------------------------------------------
// The exact form (RTBVH_QBOX below) decodes each corner, org + q * scl, and runs the reference
// slab test on it: 6 decodes + 12 slab operations per box.  Here the slab is evaluated in the
// node's grid, t(q) = q * b + a with b = scl * inv (exact: a power of two times inv) and
// a = (org - o) * inv, shared by the node's four boxes; and the ray's sign picks each axis's
// near and far corner word once per node, so a box costs 6 cvt + 6 fma + max3 + min3.
// Conservative against the reference test on the EXACT box: for every corner x the box
// contains and its decoded corner D (D <= x on the near side), the reference's
// RN(RN(x - o) * inv) and t(q) both lie within 8u * M * |inv| of (org + q scl - o) * inv
// (u = 2^-24, M = |org| + |o| + 256 scl: the roundings of the decode, the subtraction, the
// products and the fma), so the near distances are taken E = 2^-20 * M * |inv| (16u) low and
// the far ones E high.  Every box the exact test hits is hit, at an entry distance <= the
// exact one: the walk reaches every leaf the exact walk reaches and prunes only what it would.
// Finite for |o| <= 2^90, |inv| <= 2^20 (qnode_fast_ray) and corners within 2^100 (a QNode
// with larger ones keeps the exact record pair, build.hip quantize_axis); other rays take the
// exact decode.
__device__ __forceinline__ bool qnode_fast_ray(f3 o, f3 inv) {
    const float mi = fmaxf(fmaxf(fabsf(inv.x), fabsf(inv.y)), fabsf(inv.z));
    const float mo = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
    return mi <= 0x1p20f && mo <= 0x1p90f;   // NaN: false
}
struct QAxis { uint32_t nw, fw; float b, an, af; };
// CERT (the certified walk): the near side is widened by the margin rr as well, in
// position (rr * |inv| in distance): the entry of the box grown by rr on every side (margin.h).
template <bool CERT = false>
__device__ __forceinline__ QAxis qaxis(float org, float scl, uint32_t lw, uint32_t hw, float o, float inv,
                                       float rr = 0.f) {
    QAxis r;
    const bool neg = inv < 0.f;
    r.nw = neg ? hw : lw;
    r.fw = neg ? lw : hw;
    const float m = fmaf(scl, 256.f, fabsf(org) + fabsf(o));
    const float e = m * fabsf(inv);
    const float a = (org - o) * inv;
    if (CERT) r.an = fmaf(-fmaf(m, 0x1p-20f, rr), fabsf(inv), a);
    else r.an = fmaf(e, -0x1p-20f, a);
    r.af = fmaf(e, 0x1p-20f, a);
    r.b = scl * inv;
    return r;
}
__device__ __forceinline__ float qt(uint32_t w, int c, float b, float a) {
    return fmaf((float)((w >> (8 * c)) & 255u), b, a);
}
__device__ __forceinline__ bool qbox_fast(const QAxis& x, const QAxis& y, const QAxis& z, int c, bool hit, float best,
                                          float& tmin) {
    const float mn = fmaxf(fmaxf(qt(x.nw, c, x.b, x.an), qt(y.nw, c, y.b, y.an)), qt(z.nw, c, z.b, z.an));
    const float mx = fminf(fminf(qt(x.fw, c, x.b, x.af), qt(y.fw, c, y.b, y.af)), qt(z.fw, c, z.b, z.af));
    tmin = mn;
    return 0 <= mx && mn <= mx && (!hit || mn <= best);
}

// The certified walk's box test: qbox_fast, and the box's stack key, capped at its node's margin range tcn
// (margin.h: past it the node's margin says nothing, so the box is never pruned by distance -- kept while
// min(key, tcn) <= best, the pop's test too).  After the first bound the key is the entry of the box grown
// by the node's margin rho_n(best) (rr, qaxis<true>).  Before it (best +inf: nothing pruned, rr = 0) it is
// the entry of the box grown by rho_n(t_e), t_e its margin-free entry: pops compare a key with later,
// finite bounds kb, and for kb <= t_e, rho_n(kb) <= rho_n(t_e), so the key is at most the entry of the box
// grown by rho_n(kb) -- a box the certified walk must visit (that entry <= kb) keeps key <= kb; for
// kb > t_e the key (<= t_e) is kept anyway, the margin-free entry being below the bound.  The grown entry
// is the max over axes of near - rho |1/d| (branch-free: rho = 0 after the first bound).
__device__ __forceinline__ bool qbox_fast_cert(const QAxis& x, const QAxis& y, const QAxis& z, int c, float best,
                                               const MtNodeK& nk, const MtNodeRho& nr, f3 ainv, float tcn,
                                               float& key) {
    const float nx = qt(x.nw, c, x.b, x.an), ny = qt(y.nw, c, y.b, y.an), nz = qt(z.nw, c, z.b, z.an);
    const float mn = fmaxf(fmaxf(nx, ny), nz);
    const float mx = fminf(fminf(qt(x.fw, c, x.b, x.af), qt(y.fw, c, y.b, y.af)), qt(z.fw, c, z.b, z.af));
    const float rb = best == __builtin_inff() ? mt_node_eval(nr, fmaxf(mn, 0.f)) : 0.f;
    // (the looser bound mn - rho max|1/d|, 2 VALU instead of 5, A/B round 5: 5.9 ms against 2.5 -- the walk
    // keeps far more entries before its first bound)
    key = fminf(fmaxf(fmaxf(fmaf(-rb, ainv.x, nx), fmaf(-rb, ainv.y, ny)), fmaf(-rb, ainv.z, nz)), tcn);
    return 0 <= mx && mn <= mx && key <= best;
}
// GUARD false: no walk-length guard (a clz64 tree has no cycles; the census of COUNT keeps it).
// CERT (MODE 2 only): the certified walk.  Every box test's entry distance is taken on the
// box grown by its node's margin rho_n(best) (margin.h: no hit the triangle test accepts at t <= best lies
// outside that box; rho_n from the largest edge bound of the leaves below the node, carried by its QNode),
// and a box is not pruned by distance at all while best is past its node's margin range: so the walk sees
// EVERY leaf whose triangle could be accepted at t <= best, and its (t, leaf) minimum is the minimum over
// all triangles the reference could test.  A ray the bound does not cover -- a slack-test-free ray
// (qnode_fast_ray), |d| off unit, a node without a grid, a stack overflow -- is flagged in its hit record
// (HIT_FLAG) for the reference-order re-trace (k_bounce_redo).
// The deferred rays of a certified bounce pass (the rays its margin does not cover: |1/d| > 2^20, |o| > 2^90,
// |d| off unit).  The walk lists them at claim time in the pass's defer list -- entry k at defer[k] with
// DEFER_VALID set, k from the counter next[DEFER_COUNT] -- and writes a "deferred" hit record (t = -inf, flagged:
// k_bounce_shade skips it).  Drained waves claim entries through next[DEFER_CLAIM] and walk them in the
// reference order; k_bounce_redo takes the rest.  Readers clear the entries they take.
#ifndef RTBVH_DEFER_INWALK
#define RTBVH_DEFER_INWALK 1   // (0, A/B: every deferred ray to k_bounce_redo)
#endif
// a deferred ray's reference-order walk: its hit record, "exact" (t negated; a miss -inf with id INVALID)
template <bool COUNT>
__device__ __forceinline__ float2 defer_walk(const Inner* __restrict__ inner, const uint4* __restrict__ topo,
                                             const float* __restrict__ nbox, const float4* __restrict__ leaf,
                                             uint32_t T, const RayQ* e, Counts& c) {
    f3 o, d, inv;
    load_ray(e, o, d, inv);
    float best;
    uint32_t bl;
    const bool h = traverse_ref<COUNT>(nbox != nullptr, inner, topo, nbox, leaf, T, o, d, inv, best, bl, c);
    const uint32_t tri = h ? __float_as_uint(leaf[4 * (size_t)bl + 2].y) & ~LEAF_BIT : INVALID;
    return make_float2(h ? -best : -__builtin_inff(), __uint_as_float(tri));
}

// One wave takes deferred rays -- up to 64 at a time, lane k the k-th -- and walks each in the reference order,
// until the list holds none it has not taken
template <bool COUNT>
__device__ __forceinline__ void defer_walk_all(uint32_t* __restrict__ next, uint32_t* __restrict__ defer,
                                               const Inner* __restrict__ inner, const uint4* __restrict__ topo,
                                               const float* __restrict__ nbox, const float4* __restrict__ leaf,
                                               uint32_t T, const RayQ* __restrict__ qin, float2* __restrict__ hitrec,
                                               Counts& c, bool wt) {
    const uint32_t lane = threadIdx.x & 63u;
    for (;;) {
        uint32_t base = 0, m = 0;
        if (lane == 0) {
            uint32_t v = __hip_atomic_load(next + DEFER_CLAIM, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (;;) {
                const uint32_t nd = __hip_atomic_load(next + DEFER_COUNT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v >= nd) break;
                const uint32_t want = min(nd - v, 64u);
                if (__hip_atomic_compare_exchange_strong(next + DEFER_CLAIM, &v, v + want, __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    base = v;
                    m = want;
                    break;
                }
            }
        }
        base = __builtin_amdgcn_readfirstlane(base);
        m = __builtin_amdgcn_readfirstlane(m);
        if (m == 0) return;
        if (lane < m) {
            // (the appending lane stores its entry right after its count add: wait for it)
            uint32_t e;
            do {
                e = __hip_atomic_load(defer + base + lane, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            } while (!(e & DEFER_VALID));
            defer[base + lane] = 0u;   // (the list is clean for the next pass)
            const float2 hv = defer_walk<COUNT>(inner, topo, nbox, leaf, T, qin + (e & ~DEFER_VALID), c);
            if (wt) st_hitrec(hitrec + (e & ~DEFER_VALID), hv);
            else hitrec[e & ~DEFER_VALID] = hv;
        }
    }
}
// the deferral workers: wave 0 of the first DEFER_WORKERS workgroups (one per XCD) walks the deferred rays as they
// come, from the start of the pass -- beside the walk, not after it -- and leaves once every queue segment is
// claimed and the list is empty (a ray deferred after that goes to the drained waves or k_bounce_redo)
#ifndef RTBVH_DEFER_WORKERS
#define RTBVH_DEFER_WORKERS 8
#endif
constexpr uint32_t DEFER_WORKERS = RTBVH_DEFER_WORKERS;

// Early shading (RTBVH_EARLY_SHADE, certified passes): the walk's launch carries shading workgroups after its
// persistent ones.  They are dispatched as the walk's workgroups retire -- in the walk's tail -- and each takes 1024
// queue positions in order: a ray whose hit record is final (the pass's records start "not written yet", k_hit_init)
// is claimed by a compare-and-swap to "shaded" and shaded there (bounce_shade_ray, k_bounce_shade's work); the
// pass's k_bounce_shade shades the rest.  So the shading of most rays runs beside the walk's last rays.
#ifndef RTBVH_EARLY_SHADE
#define RTBVH_EARLY_SHADE 1
#endif
#ifndef RTBVH_ESHADE_RAYS
#define RTBVH_ESHADE_RAYS 1024
#endif
constexpr uint32_t ESHADE_RAYS = RTBVH_ESHADE_RAYS;   // queue positions per shading workgroup
// hit-record words of a certified pass with early shading (RTBVH_EARLY_SHADE): not written yet, and shaded already
constexpr uint32_t HIT_NOT_READY = 0xFFFFFFFFu, HIT_SHADED = 0xFFFFFFFEu;   // (x words: NaN patterns no walk writes)
// RayTraceReflection.hlsl:19-60 for one queued ray e from its closest hit (tri at t; tri INVALID: a
// miss): colour, intensity, the reflectRay record, and the next ray in e (returns whether it is live)
__device__ __forceinline__ bool bounce_apply(const TraceArgs& a, RayQ& e, uint32_t tri, float t, uint32_t& hits,
                                             uint32_t& tex) {
    f3 o, d, inv;
    load_ray(&e, o, d, inv);
    float4 col = a.color[e.idx];
    float intensity = e.intensity;
    bool live = false;
    if (tri != INVALID) {
        hits = 1;
        const HitInfo h = shade_hit_tri(a, tri, o, d, t);
        tex = h.textured;
        col = make_float4(lerpf(col.x, h.color.x, intensity), lerpf(col.y, h.color.y, intensity),
                          lerpf(col.z, h.color.z, intensity), lerpf(col.w, h.color.w, intensity));
        intensity *= h.shininess / 1000.f * 1;
        const f3 ro = add(h.hitp, mul(h.nrm, .0001f));   // RAY_OFFSET .0001
        const f3 rd = normalize(reflect(d, h.nrm));
        e.intensity = intensity;
        e.ox = ro.x; e.oy = ro.y; e.oz = ro.z;
        e.dx = rd.x; e.dy = rd.y; e.dz = rd.z;
        live = 0 < intensity;
        if (a.refl_rec) put_record(a.refl_rec, e.idx, intensity, true, ro, rd, col);   // :42-46
    } else {
        col = make_float4(lerpf(col.x, .5f, intensity), lerpf(col.y, .5f, intensity),
                          lerpf(col.z, .5f, intensity), lerpf(col.w, 1.f, intensity));
        intensity = 0.f;
        if (a.refl_rec) {   // :50-55: the ray stays, intensity 0, colour blended
            float* r = a.refl_rec + 14 * (size_t)e.idx;
            r[0] = 0.f;
            r[10] = col.x; r[11] = col.y; r[12] = col.z; r[13] = col.w;
        }
    }
    a.color[e.idx] = col;
    if (a.intensity) a.intensity[e.idx] = intensity;
    return live;
}

// The certificate of a certified walk's hit: the reference's findCollision
// (RayTraceTraversal.hlsl:106-193) reaches leaf x -- and, the walk having seen every triangle that could
// be accepted at t <= its best, returns x -- when x's own box passes the reference slab test with the
// bound t (every box above contains it: the slab test is monotone in the box, so they pass too, at every
// bound the reference holds, all >= t).  The box is the leaf's: min / max of its clip-space vertices
// (build.hip leaf_record_words, MortonCodes.hlsl:87-96), from the triangle's record.
__device__ __forceinline__ void leaf_clip_box(const float4* __restrict__ tclip, uint32_t tri, f3& lo, f3& hi) {
    const float4* P = tclip + TCS * (size_t)tri;
    const float4 a0 = P[0], a1 = P[1], a2 = P[2];
    const f3 v0 = mk(a0.x, a0.y, a0.z), v1 = mk(a1.x, a1.y, a1.z), v2 = mk(a2.x, a2.y, a2.z);
    lo = vmin(vmin(v0, v1), v2);
    hi = vmax(vmax(v0, v1), v2);
}
__device__ __forceinline__ bool leaf_certified(const TraceArgs& a, uint32_t tri, f3 o, f3 inv, float t) {
    f3 lo, hi;
    leaf_clip_box(a.tclip, tri, lo, hi);
    float tm;
    return ray_box(o, inv, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, true, t, tm);
}

// RayTraceReflection.hlsl:19-60 for queued ray i from its hit record h2 (valid: i is a ray to shade now).  CERT: a ray
// whose walk flagged it or whose hit fails the certificate is flagged (the caller lists it for the re-trace) instead
template <bool CERT>
__device__ __forceinline__ void bounce_shade_ray(const TraceArgs& a, const RayQ* __restrict__ qin, uint32_t i, float2 h2,
                                                 bool valid, RayQ& e, bool& live, bool& flagged, uint32_t& hits,
                                                 uint32_t& tex) {
    live = false;
    flagged = false;
    if (!valid) return;
    e = qin[i];
    uint32_t tri = __float_as_uint(h2.y);
    bool skip = false;
    if (CERT) {
        flagged = hit_flagged(tri);
        tri = (tri & LEAF_BIT) ? INVALID : tri & ~HIT_FLAG;
        if (signbit(h2.x)) {   // the walk's deferred rays (trace.hip DEFER_*): walked in the reference order
            skip = flagged;    //   by the walk's drained waves (exact: shaded as is), or by k_bounce_redo
            flagged = false;
            h2.x = -h2.x;
        } else if (!flagged && tri != INVALID) {
            f3 o, d, inv;
            load_ray(&e, o, d, inv);
            flagged = !leaf_certified(a, tri, o, inv, h2.x);
        }
    }
    if (!flagged && !skip) live = bounce_apply(a, e, tri, h2.x, hits, tex);
}
// ... and its outputs (all lanes of the wave call this): a flagged ray appended to the re-trace list, a live next
// ray to the next queue; hits, tex: the caller's running counts.  k_bounce_shade's work per ray, and the walk's
// early-shading workgroups'.  Inlined: the early-shading role's shading spills 13 VGPRs in its own blocks (the
// walk's loop has none: its scratch accesses are the deep stack's, as in the plain instance); as an out-of-line
// call it made the one-frame walk 2.70 -> 3.16 ms (r06_hab3)
template <bool CERT>
__device__ __forceinline__ void bounce_shade_emit(const TraceArgs& a, const RayQ* qin, uint32_t i, float2 h2, bool valid,
                                                  RayQ* qout, uint32_t* qout_count, int emit, uint32_t* redo,
                                                  uint32_t* redo_count, uint32_t& hits, uint32_t& tex) {
    RayQ e;
    bool live, flagged;
    uint32_t h1 = 0, t1 = 0;   // (bounce_apply sets them: one ray's)
    bounce_shade_ray<CERT>(a, qin, i, h2, valid, e, live, flagged, h1, t1);
    hits += h1;
    tex += t1;
    if (CERT) {
        const uint32_t rs = wave_append(flagged, redo_count);
        if (flagged) redo[rs] = i;
    }
    const uint32_t qs = wave_append(emit && live, qout_count);
    if (emit && live) qout[qs] = e;
}
// ES: the instance with early shading (a frame traced one at a time); the walk without it (frames in flight) is its
// own instance without the shading role's code (bounce_shade_emit, inlined: see there).
template <bool COUNT, int MODE, bool LIM, bool GUARD, bool CERT = false, bool ES = false>
__global__ __launch_bounds__(BLOCK, BOUNCE_WAVES) void k_bounce_trav(const Inner* __restrict__ inner,
                                                          const QNode* __restrict__ qn,
                                                          const float4* __restrict__ leaf, uint32_t T,
                                                          const RayQ* __restrict__ qin,
                                                          const uint32_t* __restrict__ qin_count,
                                                          const uint32_t* __restrict__ perm,
                                                          float2* __restrict__ hitrec, uint32_t* __restrict__ next,
                                                          unsigned long long* __restrict__ counters,
                                                          unsigned long long* __restrict__ overflow, int stack_limit,
                                                          uint32_t* __restrict__ defer, const uint4* __restrict__ topo,
                                                          const float* __restrict__ nbox, uint32_t nwalk, TraceArgs ta,
                                                          RayQ* __restrict__ qout, uint32_t* __restrict__ qout_count,
                                                          int emit, uint32_t* __restrict__ redo,
                                                          uint32_t* __restrict__ redo_count) {
    constexpr bool NEAREST = MODE >= 1, WIDE = MODE == 2;
    static_assert(!CERT || (WIDE && !LIM), "the certified walk is the 4-wide one, without a stack limit");
    const int limit = LIM ? stack_limit : WIDE ? STACK4B : STACK_SIZE;
    const uint32_t n = *qin_count;
    if (n == 0) return;
    const uint32_t lane = lane_id();
    Counts c = {0, 0, 0, 0, 0};
    // (early shading on: the hit records are written through to memory, st_hitrec)
    constexpr bool wt = CERT && ES && RTBVH_EARLY_SHADE;   // (the ES instance is launched with shading workgroups)
    if (CERT && ES && RTBVH_EARLY_SHADE && blockIdx.x >= nwalk) {   // a shading workgroup (early shading, above)
        const uint32_t b0 = (blockIdx.x - nwalk) * ESHADE_RAYS;
        uint32_t hits = 0, tex = 0;
        for (uint32_t base = b0; base < b0 + ESHADE_RAYS && base < n; base += BLOCK) {   // (uniform)
            const uint32_t i = base + threadIdx.x;
            bool valid = false;
            float2 h2 = make_float2(0.f, 0.f);
            if (i < n) {
                unsigned long long* hp = reinterpret_cast<unsigned long long*>(hitrec + i);
                const unsigned long long v = __hip_atomic_load(hp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t xb = (uint32_t)v, yb = (uint32_t)(v >> 32);
                // final: written, not taken, and not a deferred ray's "deferred" record (its walk writes it again)
                const bool ready = xb != HIT_NOT_READY && xb != HIT_SHADED &&
                                   !(xb == 0xFF800000u && yb == (INVALID ^ HIT_FLAG));
                if (ready) {
                    unsigned long long exp = v;
                    valid = __hip_atomic_compare_exchange_strong(
                        hp, &exp, (unsigned long long)HIT_SHADED | (unsigned long long)yb << 32, __ATOMIC_RELAXED,
                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                h2 = make_float2(__uint_as_float(xb), __uint_as_float(yb));
            }
            bounce_shade_emit<true>(ta, qin, i, h2, valid, qout, qout_count, emit, redo, redo_count, hits, tex);
        }
        if (COUNT) flush_counts<COUNT>(ta, c, hits, tex, 5);
        return;
    }
#ifdef RTBVH_TAIL_PROBE   // (A/B probe builds: each wave's end of walk, 100-us buckets from its start, into counters[32..63])
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
#endif
    if (CERT && DEFER_WORKERS && blockIdx.x < DEFER_WORKERS && gridDim.x > 2 * DEFER_WORKERS && threadIdx.x < 64) {
        for (;;) {
            defer_walk_all<COUNT>(next, defer, inner, topo, nbox, leaf, T, qin, hitrec, c, wt);
            // every segment claimed (lane k: segment k's counter past its length): no ray left to defer but
            // those being claimed right now
            bool used = true;
            for (uint32_t seg = lane; seg < NEXT_SEGS; seg += 64) {
                uint32_t s0, len;
                segment_bounds(n, seg, s0, len);
                used = used && __hip_atomic_load(next + NEXT_STRIDE * seg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= len;
            }
            if (__ballot(!used) == 0) break;
            __builtin_amdgcn_s_sleep(64);
        }
        defer_walk_all<COUNT>(next, defer, inner, topo, nbox, leaf, T, qin, hitrec, c, wt);
        if (COUNT) {
            unsigned long long v[2] = {c.internal, c.leaf};
            wave_sum(v);
            if (lane == 0) {
                atomicAdd(&counters[5], v[0]);
                atomicAdd(&counters[6], v[1]);
            }
        }
        return;
    }
    bool has = false, qfast = false;
    uint32_t r = 0;
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // the ray's walk; the 4-wide walk uses its node, sp and guard
    uint32_t& node = w.node;
    int& sp = w.sp;
    uint32_t& guard = w.guard;
    uint32_t btri = 0;       // triangle of the best hit (leaf record word 9): the hit record's id
    uint64_t key = NO_HIT;   // WIDE: the lexicographic (t, leaf) minimum (hit / best / bl of the binary walks)
    f3 o = mk(0.f, 0.f, 0.f), d = o, inv = o;
    // CERT: the per-node margin's coefficients (margin.h rho_n; each QNode carries its node's edge bound
    // and margin range) and the ray's flag
    const MtNodeK nk = mt_node_consts();
    bool flg = false;
    __shared__ uint32_t s_stk[WIDE ? 1 : SB][WIDE ? 1 : BLOCK];   // (none for WIDE: its LDS is the 6-B stack)
    uint32_t stack[WIDE ? 1 : STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    const uint32_t tid = threadIdx.x;
    BlockStack st{&s_stk[0][0] + (WIDE ? 0u : tid), stack};
    // WIDE: the 4-wide walk's stack and node test (wpush, qchildren), and below its step
#define RTBVH_WIDE_PART 1
#include "wide_walk.inc"
    Refill rf;
    unsigned long long wsteps = 0, mixed = 0, active_lanes = 0;
    while (true) {
        refill_claim(rf, next, n, has, [&](uint32_t p) {   // this lane takes the p-th ray of the queue
            r = perm ? perm[p] : p;
            load_ray(qin + r, o, d, inv);
            qfast = WIDE && qnode_fast_ray(o, inv);
            has = true;
            w = walk_start(root_slot(T), T);
            key = NO_HIT;
            if (CERT) {   // a ray the margin does not cover is deferred (DEFER_* below)
                flg = !(qfast && dot(d, d) <= MT_DD);
                if (flg) {
                    // the "deferred" record first, then the entry with release order: a wave that takes
                    // the entry (acquire) writes the walk's record after this one, never under it
                    const float2 mk_def = make_float2(-__builtin_inff(), __uint_as_float(INVALID ^ HIT_FLAG));
                    if (wt) st_hitrec(hitrec + r, mk_def);
                    else hitrec[r] = mk_def;
                    const uint32_t k = atomicAdd(next + DEFER_COUNT, 1u);
                    __hip_atomic_store(defer + k, r | DEFER_VALID, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    has = false;
                    flg = false;
                }
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (COUNT) {   // wave-level divergence census (stats trav_*; all lanes converged here)
            const uint64_t act = __ballot(has);
            const uint64_t lf = __ballot(has && (node & LEAF_BIT) != 0);
            wsteps++;
            active_lanes += (uint32_t)__popcll(act);
            mixed += (lf != 0 && lf != act);
        }
        if (!has) continue;
        bool done = false;
        if (WIDE) {
#ifdef RTBVH_DEBUG_PIXEL   // (scripts/debug_walk.py: one ray's walk, step by step, from the COUNT kernel)
            const bool wide_dbg = COUNT && qin[r].idx == (uint32_t)RTBVH_DEBUG_PIXEL;
#endif
#define RTBVH_WIDE_PART 2
#include "wide_walk.inc"
        } else {
            // binary walks: one fetch for every active lane, leaf or internal, before the branch: a
            // wave holding both kinds would otherwise wait for two dependent round trips (leaf records
            // and child-pair records are both 64-B aligned records)
            const bool isleaf = (node & LEAF_BIT) != 0;
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(inner + node);
            v4f q0 = rr[0], q1 = rr[1], q2 = rr[2], q3 = rr[3];
            pin(q0); pin(q1); pin(q2); pin(q3);
            if (GUARD && --guard == 0) {
                c.overflow++;
                done = true;
            } else {
                if (isleaf) {
                    if (walk_leaf<COUNT>(w, st, WalkRule<NEAREST>{}, c, o, d, node & ~LEAF_BIT, mk(q0.x, q0.y, q0.z),
                                         mk(q0.w, q1.x, q1.y), mk(q1.z, q1.w, q2.x)))
                        btri = __float_as_uint(q2.y) & ~LEAF_BIT;
                } else {
                    const uint32_t own = __float_as_uint(q3.z);
                    walk_node<COUNT>(w, st, WalkRule<NEAREST>{}, c, o, inv, limit,
                                     record_children(q0, q1, q2, child_slot(__float_as_uint(q3.x), own, 0),
                                                     child_slot(__float_as_uint(q3.y), own, 1)));
                }
                done = sp == -1;
            }
        }
        if (done) {
            // (t, triangle) of the hit, INVALID for a miss: the shading reads no leaf record
            if (WIDE) {
                uint32_t id = key != NO_HIT ? btri : INVALID;
                if (CERT && flg) id ^= HIT_FLAG;   // (a hit: bit 30 set; a miss: bit 30 cleared)
                if (CERT && wt) st_hitrec(hitrec + r, make_float2(key_t(key), __uint_as_float(id)));
                else hitrec[r] = make_float2(key_t(key), __uint_as_float(id));
            }
            else hitrec[r] = make_float2(w.best, __uint_as_float(w.hit ? btri : INVALID));
            has = false;
            if (COUNT && GUARD) {   // walk length census (stats trav_max_steps / trav_steps_log2)
                const uint32_t steps = 2 * T + 2 - guard;
                atomicAdd(&counters[32 + (31 - __clz(steps | 1u))], 1ull);
                atomicMax(&counters[13], (unsigned long long)steps);
                atomicMax(&counters[20], (unsigned long long)steps << 32 | qin[r].idx);   // (the longest: its pixel)
            }
        }
    }
#ifdef RTBVH_TAIL_PROBE
    if (lane == 0 && !COUNT) {
        const uint64_t dt = __builtin_amdgcn_s_memrealtime() - t_start;   // 100 MHz: 10000 ticks = 100 us
        atomicAdd(&counters[32 + min(31u, (uint32_t)(dt / 10000u))], 1ull);
    }
#endif
    if (CERT && RTBVH_DEFER_INWALK) {
        // The deferred rays (the slack test cannot take them) the workers above have not taken yet: once its part
        // of the queue is drained, the wave walks them in the reference order; the hit record says "exact" (t
        // negated), so k_bounce_shade shades it without a certificate.  A deferred ray no wave takes here
        // (appended after the waves looked) is re-traced by k_bounce_redo.
        defer_walk_all<COUNT>(next, defer, inner, topo, nbox, leaf, T, qin, hitrec, c, wt);
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[3] = {c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT) {
                atomicAdd(&counters[5], v[0]);
                atomicAdd(&counters[6], v[1]);
                atomicAdd(&counters[10], wsteps);
                atomicAdd(&counters[11], mixed);
                atomicAdd(&counters[12], active_lanes);
            }
            if (v[2]) {
                atomicAdd(&counters[8], v[2]);
                atomicAdd(overflow, v[2]);
            }
        }
    }
}

template <bool COUNT, bool CERT>
__global__ __launch_bounds__(BLOCK) void k_bounce_shade(TraceArgs a, const RayQ* __restrict__ qin,
                                                        const uint32_t* __restrict__ qin_count,
                                                        const float2* __restrict__ hitrec, RayQ* __restrict__ qout,
                                                        uint32_t* __restrict__ qout_count, int emit,
                                                        uint32_t* __restrict__ redo, uint32_t* __restrict__ redo_count) {
    const uint32_t n = *qin_count;
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (blockIdx.x * BLOCK >= n) return;   // whole block past the queue (wave_append below needs all lanes)
    uint32_t hits = 0, tex = 0;
    float2 h2 = make_float2(0.f, 0.f);
    if (i < n) h2 = hitrec[i];
    // (a ray the walk's early shading took is done: RTBVH_EARLY_SHADE)
    bounce_shade_emit<CERT>(a, qin, i, h2, i < n && !(CERT && __float_as_uint(h2.x) == HIT_SHADED), qout, qout_count, emit,
                            redo, redo_count, hits, tex);
    if (COUNT) {
        Counts c = {0, 0, 0, 0, 0};
        flush_counts<COUNT>(a, c, hits, tex, 5);
    }
}
// (early shading: every hit record of the pass "not written yet" before the walk)
__global__ __launch_bounds__(BLOCK) void k_hit_init(float2* __restrict__ hitrec, const uint32_t* __restrict__ qin_count) {
    const uint32_t n = *qin_count;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK)
        hitrec[i] = make_float2(__uint_as_float(HIT_NOT_READY), __uint_as_float(HIT_NOT_READY));
}

// The reference-order re-trace of the rays a certified bounce pass flagged (redo: queue indices): the
// exact findCollision DFS (traverse, reference order), then the shading as k_bounce_shade.  A fixed grid
// over the count on the device (a captured frame replays it as it is).
// Then the walk's deferred rays no drained wave claimed (trace.hip DEFER_*: entries [next[DEFER_CLAIM],
// next[DEFER_COUNT]) of the defer list, cleared as they are read) come first in the index space.
template <bool COUNT>
__global__ __launch_bounds__(BLOCK) void k_bounce_redo(TraceArgs a, const RayQ* __restrict__ qin,
                                                       const uint32_t* __restrict__ redo,
                                                       const uint32_t* __restrict__ redo_count,
                                                       RayQ* __restrict__ qout, uint32_t* __restrict__ qout_count,
                                                       int emit, uint32_t* __restrict__ defer,
                                                       const uint32_t* __restrict__ dnext) {
    const uint32_t d0 = defer ? min(dnext[DEFER_CLAIM], dnext[DEFER_COUNT]) : 0u;
    const uint32_t nd = defer ? dnext[DEFER_COUNT] - d0 : 0u;
    const uint32_t n = nd + *redo_count;
    Counts c = {0, 0, 0, 0, 0};
    uint32_t hits = 0, tex = 0;
    for (uint32_t base = blockIdx.x * BLOCK; base < n; base += gridDim.x * BLOCK) {
        const uint32_t i = base + threadIdx.x;
        bool live = false;
        RayQ e;
        if (i < n) {
            uint32_t r;
            if (i < nd) {
                r = defer[d0 + i] & ~DEFER_VALID;
                defer[d0 + i] = 0u;
            } else {
                r = redo[i - nd];
            }
            e = qin[r];
            f3 o, d, inv;
            load_ray(&e, o, d, inv);
            float best;
            uint32_t bl;
            const bool h = traverse_ref<COUNT>(a, o, d, inv, best, bl, c);
            const uint32_t tri = h ? __float_as_uint(a.leaf[4 * (size_t)bl + 2].y) & ~LEAF_BIT : INVALID;
            uint32_t h1 = 0, t1 = 0;
            live = bounce_apply(a, e, tri, best, h1, t1);
            hits += h1;
            tex += t1;
        }
        const uint32_t slot = wave_append(emit && live, qout_count);
        if (emit && live) qout[slot] = e;
    }
    flush_counts<COUNT>(a, c, hits, tex, 5);
}

// bounce-ray coherence sort key (results do not depend on the order): direction
// octant in bits 27..29, 9-bit-per-axis Morton code of the origin inside the scene
// box in bits 0..26.  Entries past the live count get the largest key and sort last.
__device__ __forceinline__ uint32_t spread9(uint32_t v) {
    v &= 0x1FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ __forceinline__ uint32_t q9(float x, float lo, float hi) {
    float t = (x - lo) / (hi - lo) * 512.f;
    t = fminf(fmaxf(t, 0.f), 511.f);
    return (uint32_t)t;
}
__global__ __launch_bounds__(BLOCK) void k_bounce_keys(const RayQ* __restrict__ q, const uint32_t* __restrict__ count,
                                                       const float* __restrict__ box, uint32_t P,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    uint32_t key = 0xFFFFFFFFu;
    if (i < *count) {
        const RayQ e = q[i];
        const uint32_t oct = (e.dx < 0.f) | ((e.dy < 0.f) << 1) | ((e.dz < 0.f) << 2);
        const uint32_t m = spread9(q9(e.ox, box[0], box[3])) << 2 | spread9(q9(e.oy, box[1], box[4])) << 1 |
                           spread9(q9(e.oz, box[2], box[5]));
        key = oct << 27 | m;
    }
    keys[i] = key;
    vals[i] = i;
}

// RayTraceBVHPS.hlsl:13-16 + the R8G8B8A8_UNORM target: screen row y <- framebuffer row H-1-y
__device__ __forceinline__ uint32_t unorm8(float c) { return (uint32_t)floorf(sat(c) * 255.f + .5f); }
__global__ __launch_bounds__(BLOCK) void k_present(const float4* __restrict__ color, uint32_t W, uint32_t H,
                                                   uint32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (size_t)W * H) return;
    const uint32_t y = (uint32_t)(i / W), x = (uint32_t)(i % W);
    const float4 c = color[(size_t)(H - 1 - y) * W + x];
    out[i] = unorm8(c.x) | unorm8(c.y) << 8 | unorm8(c.z) << 16 | unorm8(c.w) << 24;
}

// frame row y of a W x H frame traced as 8-row bands dealt over nranks: band b = y / 8 is
// rank r's p-th band, so it sits at row p * 8 + y % 8 of that rank's compact buffer, buffers
// stacked stride_rows apart (tiles.py layout).  Round-robin (slots null): r = b % nranks,
// p = b / nranks; a weighted deal (rtbvh_deal_bands): slots[b] = r << 24 | p.
__global__ __launch_bounds__(BLOCK) void k_assemble(const float4* __restrict__ bands,
                                                    const uint32_t* __restrict__ slots, uint32_t stride_rows,
                                                    uint32_t W, uint32_t H, uint32_t nranks,
                                                    float4* __restrict__ frame) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (size_t)W * H) return;
    const uint32_t y = (uint32_t)(i / W), x = (uint32_t)(i % W);
    const uint32_t b = y >> 3, sl = slots ? slots[b] : (b % nranks) << 24 | (b / nranks);
    const uint32_t r = sl >> 24, k = (sl & 0xFFFFFFu) * 8 + (y & 7u);
    frame[i] = bands[((size_t)r * stride_rows + k) * W + x];
}

// frames compared pixel for pixel (rtbvh_compare_frames): *diff += pixels whose 16 bytes differ
__global__ __launch_bounds__(BLOCK) void k_count_diff(const uint4* __restrict__ a, const uint4* __restrict__ b,
                                                      size_t n, unsigned long long* __restrict__ diff) {
    unsigned long long cnt = 0;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) {
        const uint4 x = a[i], y = b[i];
        cnt += (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
    }
    cnt = wave_sum(cnt);
    if (lane_id() == 0 && cnt) atomicAdd(diff, cnt);
}

// ---- instance selection on the host ------------------------------------------------------------
// Run-time bools as compile-time constants: with_bools(f, b0, b1, ...) calls f(std::bool_constant<b0>{},
// std::bool_constant<b1>{}, ...), so a generic lambda names the kernel instance `k<B0, B1>` of its arguments.
// Only the instances such a lambda names exist: a combination no context asks for is excluded by the
// constants written beside the arguments.
template <class F> void with_bools(F&& f) { f(); }
template <class F, class... Bs> void with_bools(F&& f, bool b, Bs... rest) {
    if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// ---- ray queries (rtbvh_query_async): caller rays in, (t, u, v, triangle) out ------------------------
// findCollision for rays the caller chose, in the space the BVH was built in.  One ray per lane on the shared
// per-lane step (Walk, walk_leaf, walk_node) with k_bounce_trav's binary modes' stack (BlockStack) and fetch
// placement (one 64-B fetch a step, leaf or node), the same claims (refill_claim: per-wave segment claims
// on per-XCD counters, a refill once REFILL_MIN lanes are idle): caller rays are incoherent, and any-hit walks
// end at very different lengths.  A ray is two float4 loads, a hit one 16-B store at the ray's own index.
// t_max and ANY enter through the walk's rule alone (QueryRule).  A zero or non-finite direction or origin needs
// no special case: the arithmetic makes the ray a miss.
// NB: on the topology and the node boxes (NodeBoxTree's fetches), for a build that wrote no records.
// Every instance keeps the walk-length guard and reads the stack limit at run time (compiling them out where no
// context needs them, as k_bounce_trav's GUARD and LIM do, measured 12.13 -> 12.06 ms at C5: less than the
// figure moves between runs, so not worth twice the instances).
// (u, v) of the winning triangle are recomputed once at the end, not carried through the walk.
__device__ __forceinline__ void ray_triangle_uv(f3 o, f3 d, f3 p0, f3 e1, f3 e2, float& u, float& v) {
    const f3 tmp = cross(d, e2);
    const float idx = 1.f / dot(e1, tmp);
    const f3 rt = sub(o, p0);
    u = dot(rt, tmp) * idx;
    v = dot(d, cross(rt, e1)) * idx;
}
template <bool ANY, bool COUNT, bool NB>
__global__ __launch_bounds__(BLOCK, BOUNCE_WAVES) void k_query(QueryArgs a) {
    // (a certified query's re-trace: the list's length is on the device, the grid sized for a.n rays; the workgroups
    // past the list leave at once -- any workgroup claims from every segment)
    const uint32_t n = a.n_dev ? *a.n_dev : a.n, T = a.T;
    if (a.n_dev && blockIdx.x * BLOCK >= n) return;
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    Counts c = {0, 0, 0, 0, 0};
    uint32_t nrays = 0, nhits = 0;
    bool has = false;
    uint32_t r = 0;
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};
    QueryRule<ANY> rule{0.f};
    f3 o = mk(0.f, 0.f, 0.f), d = o, inv = o;
    __shared__ uint32_t s_stk[SB][BLOCK];
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, n, has, [&](uint32_t p) {   // this lane takes the p-th ray of the walk order
            r = a.perm ? a.perm[p] : p;
            const float4 q0 = a.rays[2 * (size_t)r], q1 = a.rays[2 * (size_t)r + 1];
            o = mk(q0.x, q0.y, q0.z);
            rule.tmax = q0.w;
            d = mk(q1.x, q1.y, q1.z);
            inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
            has = true;
            w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (!has) continue;
        bool done = false;
        const bool isleaf = (w.node & LEAF_BIT) != 0;
        // one fetch for every active lane, leaf or node, before the branch (k_bounce_trav); NB: a node's
        // children from the topology, then their boxes
        v4f q0, q1, q2;
        uint32_t cl = 0, cr = 0;
        if (!NB || isleaf) {
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(a.inner + w.node);
            q0 = rr[0]; q1 = rr[1]; q2 = rr[2];
            v4f q3 = rr[3];
            pin(q0); pin(q1); pin(q2); pin(q3);
            if (!NB && !isleaf) {
                const uint32_t own = __float_as_uint(q3.z);
                cl = child_slot(__float_as_uint(q3.x), own, 0);
                cr = child_slot(__float_as_uint(q3.y), own, 1);
            }
        } else {
            const ChildPair ch = nbt.children(w.node);
            cl = ch.cl;
            cr = ch.cr;
            q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
            q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
            q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
        }
        if (--w.guard == 0) {
            c.overflow++;
            done = true;
        } else if (isleaf) {
            const bool acc = walk_leaf<COUNT>(w, st, rule, c, o, d, w.node & ~LEAF_BIT, mk(q0.x, q0.y, q0.z),
                                              mk(q0.w, q1.x, q1.y), mk(q1.z, q1.w, q2.x));
            done = (ANY && acc) || w.sp == -1;
        } else {
            walk_node<COUNT>(w, st, rule, c, o, inv, limit, record_children(q0, q1, q2, cl, cr));
            done = w.sp == -1;
        }
        if (done) {
            // (u, v) of the winning triangle, recomputed once from its leaf record.  (Fetching the record with the
            // wave's next common fetch instead -- the ray taking one more step at its leaf -- gained nothing: C5,
            // closest-hit 12.06 -> 12.32 ms)
            float4 h = make_float4(-1.f, 0.f, 0.f, __uint_as_float(INVALID));
            if (w.hit) {
                const float4* lr = leaf + 4 * (size_t)w.bl;
                const float4 la = lr[0], lb = lr[1], lc = lr[2];
                float u, v;
                ray_triangle_uv(o, d, mk(la.x, la.y, la.z), mk(la.w, lb.x, lb.y), mk(lb.z, lb.w, lc.x), u, v);
                h = make_float4(w.best, u, v, __uint_as_float(__float_as_uint(lc.y) & ~LEAF_BIT));
            }
            a.hits[r] = h;
            has = false;
            if (COUNT) {
                nrays++;
                nhits += w.hit;
            }
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[5] = {nrays, nhits, c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int k = 0; k < 4; k++) atomicAdd(&a.counts[k], v[k]);
            if (v[4]) atomicAdd(a.overflow, v[4]);
        }
    }
}

// ---- certified ray queries (RTBVH_QUERY_CERTIFIED): the 4-wide certified walk for caller rays ---------------
// k_bounce_trav's certified walk (wide_walk.inc, CERT: the QNodes, boxes grown by the margin, the u64 (t, leaf)
// key) with k_query's rays, claims and hits.  DESIGN.md 5b has the argument; in short:
//  - a ray the margin does not cover -- !(qnode_fast_ray && d.d <= MT_DD), NaN inputs included -- never steps: it is
//    listed for the re-trace at its claim;
//  - t_max is the walk's initial bound: the key starts at (t_max, 0xFFFFFFFF), so a triangle at t <= t_max wins
//    (its leaf index is below the sentinel), one beyond never does, and a final key with the sentinel is a miss;
//    +inf gives NO_HIT, the bounce walk's start.  !(t_max > EPSILON) (NaN included) accepts no triangle: a miss
//    without a walk;
//  - ANY: the walk ends at the first accepted triangle;
//  - the certificate: the winning triangle's own leaf box (leaf_clip_box, leaf_certified's source) passes the
//    reference's box test -- with the bound t for a closest hit, the any-hit rule with t_max for ANY;
//  - a ray without a certificate or flagged by the step (a node without a grid, a stack overflow) is listed too.
// A wave appends its rays to the list with one atomic, at the top of its next iteration (an all-uncovered batch
// would otherwise make one same-address atomic a ray).
// The list (a.redo, its length a.redo_n) is re-traced by k_query over it as its perm (launch_query_certified): the
// plain mode's answer by construction.  The step's own overflow count is dropped: the re-trace reports the ray's.
// No walk-length guard (a clz64 tree) and no stack limit: api.hip takes k_query for every ray otherwise.
// COUNT: the walk counts a.walk[0..2] (certified, redone, uncovered), and a.counts from the rays answered here.
template <bool ANY, bool COUNT>
__global__ __launch_bounds__(BLOCK, BOUNCE_WAVES) void k_query_wide(QueryArgs a) {
    const uint32_t n = a.n, T = a.T;
    const uint32_t lane = lane_id(), tid = threadIdx.x;
    const float4* __restrict__ leaf = a.leaf;
    Counts c = {0, 0, 0, 0, 0};
    uint32_t nhits = 0, ncert = 0, nunc = 0, nlisted = 0;   // per lane; nlisted: the wave's listed rays
    bool has = false, flg = false;
    uint32_t r = 0, node = INVALID, guard = 0, btri = 0;
    int sp = 0;
    uint64_t key = NO_HIT;
    float tmax = 0.f;
    f3 o = mk(0.f, 0.f, 0.f), d = o, inv = o;
    const MtNodeK nk = mt_node_consts();
    // the walk's names (wide_walk.inc): the certified walk, no guard (a clz64 tree), the whole stack, covered rays
    constexpr bool WIDE = true, CERT = true, GUARD = false;
    const Inner* __restrict__ inner = a.inner;
    const QNode* __restrict__ qn = a.qnode;
    const int limit = STACK4B;
    const bool qfast = true;
#define RTBVH_WIDE_PART 1
#include "wide_walk.inc"
    const float4 miss = make_float4(-1.f, 0.f, 0.f, __uint_as_float(INVALID));
    Refill rf;
    bool pend = false;   // this lane's ray r (ended, or claimed uncovered: the lane holds none) goes to the re-trace list
    while (true) {
        {   // (all lanes converged) the rays the last iteration found for the list: one atomic a wave
            const uint32_t slot = wave_append(pend, a.redo_n);
            if (pend) a.redo[slot] = r;
            if (COUNT) nlisted += (uint32_t)__popcll(__ballot(pend));   // (wave-uniform)
            pend = false;
        }
        refill_claim(rf, a.next, n, has, [&](uint32_t p) {   // this lane takes the p-th ray of the walk order
            r = a.perm ? a.perm[p] : p;
            const float4 q0 = a.rays[2 * (size_t)r], q1 = a.rays[2 * (size_t)r + 1];
            o = mk(q0.x, q0.y, q0.z);
            tmax = q0.w;
            d = mk(q1.x, q1.y, q1.z);
            inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
            if (!(qnode_fast_ray(o, inv) && dot(d, d) <= MT_DD)) {   // not covered by the margin (NaN: here too)
                pend = true;
                if (COUNT) nunc++;
            } else if (!(tmax > EPSILON)) {   // no triangle is accepted at t <= t_max (every accepted t > EPSILON)
                a.hits[r] = miss;
                if (COUNT) ncert++;
            } else {
                has = true;
                flg = false;
                node = root_slot(T);
                sp = 0;
                key = (uint64_t)__float_as_uint(tmax) << 32 | 0xFFFFFFFFull;
            }
        });
        if (__ballot(has || pend) == 0 && rf.drained) break;   // (a pending ray is listed at the top)
        if (!has) continue;
        bool done = false;
        {
#ifdef RTBVH_DEBUG_PIXEL
            const bool wide_dbg = false;
#endif
#define RTBVH_WIDE_PART 2
#include "wide_walk.inc"
        }
        const bool hit = (uint32_t)key != 0xFFFFFFFFu;
        if (ANY && hit) done = true;
        if (done) {
            bool redo = flg;
            float4 h = miss;
            if (!redo && hit) {
                const float t = key_t(key);
                f3 lo, hi;
                leaf_clip_box(a.tclip, btri, lo, hi);
                float tm;
                const bool ok = ANY ? ray_box(o, inv, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, false, 0.f, tm) && !(tm > tmax)
                                    : ray_box(o, inv, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, true, t, tm);
                if (ok) {   // (u, v) recomputed from the winning leaf's record, as k_query does
                    const float4* lr = leaf + 4 * (size_t)(uint32_t)key;
                    const float4 la = lr[0], lb = lr[1], lc = lr[2];
                    float u, v;
                    ray_triangle_uv(o, d, mk(la.x, la.y, la.z), mk(la.w, lb.x, lb.y), mk(lb.z, lb.w, lc.x), u, v);
                    h = make_float4(t, u, v, __uint_as_float(btri));
                } else {
                    redo = true;
                }
            }
            if (redo) {
                pend = true;
            } else {
                a.hits[r] = h;
                if (COUNT) {
                    ncert++;
                    nhits += hit;
                }
            }
            has = false;
        }
    }
    if (COUNT) {
        unsigned long long v[5] = {ncert, nhits, c.internal, c.leaf, nunc};
        wave_sum(v);
        if (lane == 0) {   // (redone: the listed rays that were not uncovered)
            for (int k = 0; k < 4; k++) atomicAdd(&a.counts[k], v[k]);
            atomicAdd(&a.walk[0], v[0]);
            atomicAdd(&a.walk[1], (unsigned long long)nlisted - v[4]);
            atomicAdd(&a.walk[2], v[4]);
        }
    }
}

// the coherence key of caller rays: k_bounce_keys' (octant, origin Morton) over the root box
__global__ __launch_bounds__(BLOCK) void k_query_keys(const float4* __restrict__ rays, uint32_t n,
                                                      const float* __restrict__ box, uint32_t* __restrict__ keys,
                                                      uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 q0 = rays[2 * (size_t)i], q1 = rays[2 * (size_t)i + 1];
    const uint32_t oct = (q1.x < 0.f) | ((q1.y < 0.f) << 1) | ((q1.z < 0.f) << 2);
    const uint32_t m = spread9(q9(q0.x, box[0], box[3])) << 2 | spread9(q9(q0.y, box[1], box[4])) << 1 |
                       spread9(q9(q0.z, box[2], box[5]));
    keys[i] = oct << 27 | m;
    vals[i] = i;
}

// ---- closest-point queries (rtbvh_nearest_async): caller points in, (point, dist2, u, v, triangle) out ---------
// For each point the lexicographic minimum of (dist2, triangle id) over the triangles with dist2 <= max_dist2, in
// the space the BVH was built in.  include/rtbvh.h has the formulas; DESIGN.md 5d why the walk returns the
// brute-force answer bit for bit: the closest point is clamped into the leaf's own box, so -- every operation of
// the distance rounding monotonically -- a triangle's dist2 is never below the box distance of any box that
// contains its leaf box, and a walk that enters a box iff its distance is <= the bound (non-strict: ties are
// visited for the id tie-break) reaches every triangle that can win, whatever order it visits in.
// One point per lane on k_query's frame: the same claims, stack, one 64-B fetch a step before the leaf / node
// branch, walk-length guard and run-time stack limit.  The best is a u64 key (dist2 bits << 32 | id) started at
// (max_dist2 bits, 0xFFFFFFFF): dist2 >= +0, so the bits order as the floats, a NaN dist2 is above every key,
// dist2 == max_dist2 is accepted and a final sentinel id means no result.  (point, u, v) of the winner are
// recomputed once at the end from its leaf record (bl: its sorted leaf index).
// Plain fp32 as specified: no fma, no fast intrinsics; the one division of a triangle is the IEEE quotient.
__device__ __forceinline__ float box_dist2(f3 p, f3 lo, f3 hi) {
    const float dx = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.f);
    const float dy = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.f);
    const float dz = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.f);
    return (dx * dx + dy * dy) + dz * dz;
}
// The closest point of the triangle (a, e1, e2) to p, clamped into [lo, hi]: the Voronoi regions in the header's
// order (the first that matches), as selects around ONE division -- each region's quotient is that division of its
// own numerator and denominator, so the floats are the branchy form's.
__device__ __forceinline__ float triangle_dist2(f3 p, f3 a, f3 e1, f3 e2, f3 lo, f3 hi, float& u, float& v, f3& q) {
    const f3 ap = sub(p, a);
    const float d1 = dot(e1, ap), d2 = dot(e2, ap);
    const float e11 = dot(e1, e1), e12 = dot(e1, e2), e22 = dot(e2, e2);
    const float d3 = d1 - e11, d4 = d2 - e12, d5 = d1 - e12, d6 = d2 - e22;
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    const bool r0 = d1 <= 0.f && d2 <= 0.f;                   // vertex 0
    const bool r1 = d3 >= 0.f && d4 <= d3;                    // vertex 1
    const bool r2 = d6 >= 0.f && d5 <= d6;                    // vertex 2
    const bool r3 = vc <= 0.f && d1 >= 0.f && d3 <= 0.f;      // edge 0-1
    const bool r4 = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;      // edge 0-2
    const bool r5 = va <= 0.f && d43 >= 0.f && d56 >= 0.f;    // edge 1-2
    const float num = r3 ? d1 : r4 ? d2 : r5 ? d43 : 1.f;
    const float den = r3 ? d1 - d3 : r4 ? d2 - d6 : r5 ? d43 + d56 : (va + vb) + vc;
    const float w = num / den;
    if (r0) { u = 0.f; v = 0.f; }
    else if (r1) { u = 1.f; v = 0.f; }
    else if (r2) { u = 0.f; v = 1.f; }
    else if (r3) { u = w; v = 0.f; }
    else if (r4) { u = 0.f; v = w; }
    else if (r5) { u = 1.f - w; v = w; }
    else { u = vb * w; v = vc * w; }
    if (u != u) u = 0.f;   // a degenerate triangle: vertex 0 stands for it
    if (v != v) v = 0.f;
    q = add(add(a, mul(e1, u)), mul(e2, v));
    q = mk(fmaxf(lo.x, fminf(hi.x, q.x)), fmaxf(lo.y, fminf(hi.y, q.y)), fmaxf(lo.z, fminf(hi.z, q.z)));
    const f3 e = sub(p, q);
    return dot(e, e);
}
// 8 waves per SIMD, as k_query: every instance fits the 64 registers without a spill
template <bool COUNT, bool NB>
__global__ __launch_bounds__(BLOCK, BOUNCE_WAVES) void k_nearest(NearestArgs a) {
    const uint32_t n = a.n, T = a.T;
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    Counts c = {0, 0, 0, 0, 0};
    uint32_t npoints = 0, nfound = 0;
    bool has = false;
    uint32_t r = 0;
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // (bl: the best triangle's sorted leaf index; hit, best unused)
    uint64_t key = 0;
    f3 p = mk(0.f, 0.f, 0.f);
    __shared__ uint32_t s_stk[SB][BLOCK];
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    const float4 none0 = make_float4(0.f, 0.f, 0.f, -1.f), none1 = make_float4(0.f, 0.f, __uint_as_float(INVALID), 0.f);
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, n, has, [&](uint32_t k) {   // this lane takes the k-th point of the walk order
            r = a.perm ? a.perm[k] : k;
            const float4 pt = a.points[r];
            p = mk(pt.x, pt.y, pt.z);
            const float bound = pt.w + 0.f;   // (-0 -> +0: the key's bits order as the floats)
            if (COUNT) npoints++;
            const bool finite = fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY;
            if (!(bound >= 0.f) || !finite) {   // no walk: no result
                a.out[2 * (size_t)r] = none0;
                a.out[2 * (size_t)r + 1] = none1;
            } else {
                has = true;
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
                key = (uint64_t)__float_as_uint(bound) << 32 | 0xFFFFFFFFull;
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (!has) continue;
        bool done = false;
        const bool isleaf = (w.node & LEAF_BIT) != 0;
        // one fetch for every active lane, leaf or node, before the branch (k_query); NB: a node's children from
        // the topology, then their boxes
        v4f q0, q1, q2, q3;
        uint32_t cl = 0, cr = 0;
        if (!NB || isleaf) {
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(a.inner + w.node);
            q0 = rr[0]; q1 = rr[1]; q2 = rr[2]; q3 = rr[3];
            pin(q0); pin(q1); pin(q2); pin(q3);
            if (!NB && !isleaf) {
                const uint32_t own = __float_as_uint(q3.z);
                cl = child_slot(__float_as_uint(q3.x), own, 0);
                cr = child_slot(__float_as_uint(q3.y), own, 1);
            }
        } else {
            const ChildPair ch = nbt.children(w.node);
            cl = ch.cl;
            cr = ch.cr;
            q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
            q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
            q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
            q3 = v4f{0.f, 0.f, 0.f, 0.f};
        }
        const float bound = key_t(key);
        if (--w.guard == 0) {
            c.overflow++;
            done = true;
        } else if (isleaf) {
            if (COUNT) c.leaf++;
            // the leaf's own box first (words 10..15): a triangle's dist2 is never below it
            const f3 lo = mk(q2.z, q2.w, q3.x), hi = mk(q3.y, q3.z, q3.w);
            if (box_dist2(p, lo, hi) <= bound) {
                float u, v;
                f3 q;
                const float d = triangle_dist2(p, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), mk(q1.z, q1.w, q2.x), lo,
                                               hi, u, v, q);
                const uint64_t cand = (uint64_t)__float_as_uint(d) << 32 | (__float_as_uint(q2.y) & ~LEAF_BIT);
                if (cand < key) {
                    key = cand;
                    w.bl = w.node & ~LEAF_BIT;
                }
            }
            walk_pop(w, st);
            done = w.sp == -1;
        } else {
            if (COUNT) c.internal++;
            const float bdl = box_dist2(p, mk(q0.x, q0.y, q2.x), mk(q0.z, q0.w, q2.y));
            const float bdr = box_dist2(p, mk(q1.x, q1.y, q2.z), mk(q1.z, q1.w, q2.w));
            const bool lh = bdl <= bound, rh = bdr <= bound;
            if (!lh && !rh) {
                walk_pop(w, st);
            } else if (lh && rh && w.sp + 1 >= limit) {   // the stack limit: both children lost, counted
                c.overflow++;
                walk_pop(w, st);
            } else {
                const bool swap = lh && rh && bdr < bdl;   // the nearer child first
                if (lh && rh) {
                    st.store(w.sp, w.top);   // push the other
                    w.sp++;
                    w.top = swap ? cl : cr;
                }
                w.node = swap ? cr : (lh ? cl : cr);
            }
            done = w.sp == -1;
        }
        if (done) {
            float4 o0 = none0, o1 = none1;
            if ((uint32_t)key != 0xFFFFFFFFu) {   // the winner's (point, u, v), recomputed from its leaf record
                const float4* lr = leaf + 4 * (size_t)w.bl;
                const float4 la = lr[0], lb = lr[1], lc = lr[2], ld = lr[3];
                float u, v;
                f3 q;
                const float d = triangle_dist2(p, mk(la.x, la.y, la.z), mk(la.w, lb.x, lb.y), mk(lb.z, lb.w, lc.x),
                                               mk(lc.z, lc.w, ld.x), mk(ld.y, ld.z, ld.w), u, v, q);
                o0 = make_float4(q.x, q.y, q.z, d);
                o1 = make_float4(u, v, __uint_as_float((uint32_t)key), 0.f);
            }
            a.out[2 * (size_t)r] = o0;
            a.out[2 * (size_t)r + 1] = o1;
            has = false;
            if (COUNT) nfound += (uint32_t)key != 0xFFFFFFFFu;
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[5] = {npoints, nfound, c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int k = 0; k < 4; k++) atomicAdd(&a.counts[k], v[k]);
            if (v[4]) atomicAdd(a.overflow, v[4]);
        }
    }
}

// RTBVH_NEAREST_SORT's key: the 30-bit Morton code of the point in the root box
__global__ __launch_bounds__(BLOCK) void k_nearest_keys(const float4* __restrict__ points, uint32_t n,
                                                        const float* __restrict__ box, uint32_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 p = points[i];
    keys[i] = spread9(q9(p.x, box[0], box[3])) << 2 | spread9(q9(p.y, box[1], box[4])) << 1 |
              spread9(q9(p.z, box[2], box[5]));
    vals[i] = i;
}

// ---- radius queries (rtbvh_within_async): caller points in, every (triangle, dist2) with dist2 <= max_dist2 out --
// k_nearest's frame and its two distances, unchanged; the bound is the point's max_dist2 for the whole walk, so
// DESIGN.md 5d's lemma gives the exact set (5e): a member's dist2 is never below the box distance of a box around
// its leaf, and every box with distance <= bound is entered.  Nothing is gained from the nearer child first, so
// the walk is left-first, which meets the leaves in the build's sort order: that is the order of a point's list.
// FILL = false counts a point's members and stores the count at offsets[r + 1] (the scan makes offsets of them);
// FILL = true stores the members at offsets[r] + i while that is below min(offsets[r + 1], capacity): whatever the
// offsets hold, no store leaves the point's segment or the first `capacity` pairs.
// Every instance fits 64 registers without a spill at 8 waves per SIMD.
template <bool FILL, bool COUNT, bool NB>
__global__ __launch_bounds__(BLOCK, BOUNCE_WAVES) void k_within(WithinArgs a) {
    const uint32_t n = a.n, T = a.T;
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    Counts c = {0, 0, 0, 0, 0};
    uint32_t npoints = 0;
    unsigned long long npairs = 0;
    bool has = false;
    uint32_t r = 0, cnt = 0;
    unsigned long long pos = 0, end = 0;   // FILL: the next pair's index and the end of the point's segment
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // (hit, best, bl unused)
    float bound = 0.f;
    f3 p = mk(0.f, 0.f, 0.f);
    __shared__ uint32_t s_stk[SB][BLOCK];
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, n, has, [&](uint32_t k) {   // this lane takes the k-th point of the walk order
            r = a.perm ? a.perm[k] : k;
            const float4 pt = a.points[r];
            p = mk(pt.x, pt.y, pt.z);
            bound = pt.w + 0.f;   // (-0 -> +0)
            if (COUNT && a.count_pairs) npoints++;
            const bool finite = fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY;
            if (!(bound >= 0.f) || !finite) {   // no walk: an empty list
                if (!FILL) a.offsets[(size_t)r + 1] = 0;
            } else {
                has = true;
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
                cnt = 0;
                if (FILL) {
                    pos = a.offsets[r];
                    const unsigned long long e = a.offsets[(size_t)r + 1];
                    end = e < a.capacity ? e : a.capacity;
                }
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (!has) continue;
        bool done = false;
        const bool isleaf = (w.node & LEAF_BIT) != 0;
        // one fetch for every active lane, leaf or node, before the branch (k_nearest)
        v4f q0, q1, q2, q3;
        uint32_t cl = 0, cr = 0;
        if (!NB || isleaf) {
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(a.inner + w.node);
            q0 = rr[0]; q1 = rr[1]; q2 = rr[2]; q3 = rr[3];
            pin(q0); pin(q1); pin(q2); pin(q3);
            if (!NB && !isleaf) {
                const uint32_t own = __float_as_uint(q3.z);
                cl = child_slot(__float_as_uint(q3.x), own, 0);
                cr = child_slot(__float_as_uint(q3.y), own, 1);
            }
        } else {
            const ChildPair ch = nbt.children(w.node);
            cl = ch.cl;
            cr = ch.cr;
            q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
            q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
            q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
            q3 = v4f{0.f, 0.f, 0.f, 0.f};
        }
        if (--w.guard == 0) {
            c.overflow++;
            done = true;
        } else if (isleaf) {
            if (COUNT) c.leaf++;
            const f3 lo = mk(q2.z, q2.w, q3.x), hi = mk(q3.y, q3.z, q3.w);   // the leaf's own box first
            if (box_dist2(p, lo, hi) <= bound) {
                float u, v;
                f3 q;
                const float d = triangle_dist2(p, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), mk(q1.z, q1.w, q2.x), lo,
                                               hi, u, v, q);
                if (d <= bound) {   // (false for a NaN dist2)
                    if (!FILL || COUNT) cnt++;
                    if (FILL && pos < end) {
                        a.pairs[pos] = make_uint2(__float_as_uint(q2.y) & ~LEAF_BIT, __float_as_uint(d));
                        pos++;
                    }
                }
            }
            walk_pop(w, st);
            done = w.sp == -1;
        } else {
            if (COUNT) c.internal++;
            const float bdl = box_dist2(p, mk(q0.x, q0.y, q2.x), mk(q0.z, q0.w, q2.y));
            const float bdr = box_dist2(p, mk(q1.x, q1.y, q2.z), mk(q1.z, q1.w, q2.w));
            const bool lh = bdl <= bound, rh = bdr <= bound;
            if (!lh && !rh) {
                walk_pop(w, st);
            } else if (lh && rh && w.sp + 1 >= limit) {   // the stack limit: both children lost, counted
                c.overflow++;
                walk_pop(w, st);
            } else {
                if (lh && rh) {   // left first: push the right child
                    st.store(w.sp, w.top);
                    w.sp++;
                    w.top = cr;
                }
                w.node = lh ? cl : cr;
            }
            done = w.sp == -1;
        }
        if (done) {
            if (!FILL) a.offsets[(size_t)r + 1] = cnt;
            if (COUNT && a.count_pairs) npairs += cnt;
            has = false;
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[5] = {npoints, npairs, c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int k = 0; k < 4; k++) atomicAdd(&a.counts[k], v[k]);
            if (v[4]) atomicAdd(a.overflow, v[4]);
        }
    }
}

// ---- k-nearest queries (rtbvh_knn_async): caller points in, the k smallest (dist2, triangle) within max_dist2 out --
// k_nearest's frame with a list in place of the single key.  Each lane keeps k u64 keys (dist2 bits << 32 | id) in
// ascending order, all started at k_nearest's sentinel (max_dist2 bits, 0xFFFFFFFF): the bound is max_dist2 until the
// list is full, dist2 == max_dist2 is accepted, a NaN dist2 is above every key, and the slots never filled still hold
// the sentinel at the end.  `worst` caches slot k - 1; a candidate below it is inserted by shifting the larger keys
// one slot up (the old worst falls out), and a box -- a child's, or a leaf's own -- is entered iff its distance is <=
// the worst key's dist2, non-strict, the nearer child first.  DESIGN.md 5h: 5d's lemma with the bound read as the
// worst key's dist2, which only falls, so a member of the final list was never pruned.
// The list lives in LDS beside the stack, [slot][lane]: 8 B a lane in one 2 KB row a slot, so a wave's lanes are on
// distinct banks whatever slot each one touches.  CAP (the slots allocated: 4, 8, 16 or 32) is the smallest tier
// that holds k, so a small k does not pay the LDS of 32; the loops run to k.  knn_blocks(CAP) blocks fit a CU's
// 160 KB, which is also what the launch bound asks for: the registers follow the occupancy the LDS allows.
// The insertion is bound by LDS latency, not traffic: it fetches ROUND keys together and then decides, which took 29%
// off k = 32 against a key a round.  (In scratch at 8 waves per SIMD, or unordered with a tracked worst slot and a
// final sort, the walk was slower: DESIGN.md 5h, profiles/knn_ab.json.)
constexpr int knn_blocks(int cap) {   // blocks (= waves per SIMD) of 16 KB of stack and cap * 2 KB of list in 160 KB
    const int b = 160 / (16 + 2 * cap);
    return b < (int)BOUNCE_WAVES ? b : (int)BOUNCE_WAVES;
}
struct KnnList {
    unsigned long long* col;   // this lane's LDS column, slot j at col[j * BLOCK]
    __device__ __forceinline__ void store(int j, uint64_t v) { col[j * BLOCK] = v; }
    __device__ __forceinline__ uint64_t load(int j) const { return col[j * BLOCK]; }
};
template <int CAP, bool COUNT, bool NB>
__global__ __launch_bounds__(BLOCK, knn_blocks(CAP)) void k_knn(KnnArgs a) {
    const uint32_t n = a.n, T = a.T;
    const int k = (int)a.k;   // 1 .. CAP
    constexpr int ROUND = CAP >= 16 ? 8 : 4;   // keys an insertion fetches together
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    Counts c = {0, 0, 0, 0, 0};
    uint32_t npoints = 0, nfound = 0;
    bool has = false;
    uint32_t r = 0;
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // (hit, best, bl unused)
    uint64_t worst = 0;   // the list's slot k - 1
    f3 p = mk(0.f, 0.f, 0.f);
    __shared__ uint32_t s_stk[SB][BLOCK];
    __shared__ unsigned long long s_lst[CAP][BLOCK];
    KnnList lst{&s_lst[0][threadIdx.x]};
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    const uint2 none = make_uint2(INVALID, __float_as_uint(-1.f));
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, n, has, [&](uint32_t i) {   // this lane takes the i-th point of the walk order
            r = a.perm ? a.perm[i] : i;
            const float4 pt = a.points[r];
            p = mk(pt.x, pt.y, pt.z);
            const float bound = pt.w + 0.f;   // (-0 -> +0: the key's bits order as the floats)
            if (COUNT) npoints++;
            const bool finite = fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY;
            if (!(bound >= 0.f) || !finite) {   // no walk: every slot none
                for (int j = 0; j < k; j++) a.pairs[(size_t)r * k + j] = none;
            } else {
                has = true;
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
                worst = (uint64_t)__float_as_uint(bound) << 32 | 0xFFFFFFFFull;
                for (int j = 0; j < k; j++) lst.store(j, worst);
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (!has) continue;
        bool done = false;
        const bool isleaf = (w.node & LEAF_BIT) != 0;
        // one fetch for every active lane, leaf or node, before the branch (k_nearest)
        v4f q0, q1, q2, q3;
        uint32_t cl = 0, cr = 0;
        if (!NB || isleaf) {
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(a.inner + w.node);
            q0 = rr[0]; q1 = rr[1]; q2 = rr[2]; q3 = rr[3];
            pin(q0); pin(q1); pin(q2); pin(q3);
            if (!NB && !isleaf) {
                const uint32_t own = __float_as_uint(q3.z);
                cl = child_slot(__float_as_uint(q3.x), own, 0);
                cr = child_slot(__float_as_uint(q3.y), own, 1);
            }
        } else {
            const ChildPair ch = nbt.children(w.node);
            cl = ch.cl;
            cr = ch.cr;
            q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
            q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
            q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
            q3 = v4f{0.f, 0.f, 0.f, 0.f};
        }
        const float bound = key_t(worst);
        if (--w.guard == 0) {
            c.overflow++;
            done = true;
        } else if (isleaf) {
            if (COUNT) c.leaf++;
            const f3 lo = mk(q2.z, q2.w, q3.x), hi = mk(q3.y, q3.z, q3.w);   // the leaf's own box first
            if (box_dist2(p, lo, hi) <= bound) {
                float u, v;
                f3 q;
                const float d = triangle_dist2(p, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), mk(q1.z, q1.w, q2.x), lo,
                                               hi, u, v, q);
                const uint64_t cand = (uint64_t)__float_as_uint(d) << 32 | (__float_as_uint(q2.y) & ~LEAF_BIT);
                if (cand < worst) {   // into its place: the keys above it move one slot up, the worst falls out
                    // ROUND keys a round, fetched together: one LDS latency a round, not one a key
                    int j = k - 1;
                    uint64_t top = cand;   // slot k - 1 afterwards: the candidate, or what slot k - 2 held
                    for (bool go = j > 0, first = true; go; first = false) {
                        uint64_t b[ROUND];
#pragma unroll
                        for (int i = 0; i < ROUND; i++) b[i] = lst.load(j - 1 - i > 0 ? j - 1 - i : 0);
                        if (first && !(b[0] < cand)) top = b[0];
#pragma unroll
                        for (int i = 0; i < ROUND; i++)   // (step i: j is the round's first j minus i, b[i] slot j - 1)
                            if (go) {
                                if (b[i] < cand) {
                                    go = false;
                                } else {
                                    lst.store(j, b[i]);
                                    go = --j > 0;
                                }
                            }
                    }
                    lst.store(j, cand);
                    worst = top;
                }
            }
            walk_pop(w, st);
            done = w.sp == -1;
        } else {
            if (COUNT) c.internal++;
            const float bdl = box_dist2(p, mk(q0.x, q0.y, q2.x), mk(q0.z, q0.w, q2.y));
            const float bdr = box_dist2(p, mk(q1.x, q1.y, q2.z), mk(q1.z, q1.w, q2.w));
            const bool lh = bdl <= bound, rh = bdr <= bound;
            if (!lh && !rh) {
                walk_pop(w, st);
            } else if (lh && rh && w.sp + 1 >= limit) {   // the stack limit: both children lost, counted
                c.overflow++;
                walk_pop(w, st);
            } else {
                const bool swap = lh && rh && bdr < bdl;   // the nearer child first
                if (lh && rh) {
                    st.store(w.sp, w.top);   // push the other
                    w.sp++;
                    w.top = swap ? cl : cr;
                }
                w.node = swap ? cr : (lh ? cl : cr);
            }
            done = w.sp == -1;
        }
        if (done) {   // the list is in order: the sentinels, all at its end, become "none"
            for (int j = 0; j < k; j++) {
                const uint64_t key = lst.load(j);
                const bool found = (uint32_t)key != 0xFFFFFFFFu;
                a.pairs[(size_t)r * k + j] = found ? make_uint2((uint32_t)key, (uint32_t)(key >> 32)) : none;
                if (COUNT) nfound += found;
            }
            has = false;
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[5] = {npoints, nfound, c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int i = 0; i < 4; i++) atomicAdd(&a.counts[i], v[i]);
            if (v[4]) atomicAdd(a.overflow, v[4]);
        }
    }
}

// ---- all-hits ray queries (rtbvh_allhits_async): caller rays in, every (t, u, v, triangle) with t <= t_max out ----
// k_within's frame and CSR protocol with k_query's rays.  The bound never shrinks: a child is entered iff its box
// passes the any-hit rule query_box<true> with the ray's t_max, left first, and a leaf's triangle is a member iff
// ray_triangle accepts it at t <= t_max.  The slab test is monotone in the box, so every box around a member's
// leaf box passes when the leaf box does: the walk lists the brute-force set, in the build's sort
// order.  A leaf's own box is tested at its parent (the same floats); a one-triangle tree has no parent, so the
// box is tested at the leaf there.
// rayTriangleCollision with (u, v) kept: ray_triangle's operations in ray_triangle's order
__device__ __forceinline__ float ray_triangle_tuv(f3 o, f3 d, f3 p0, f3 e1, f3 e2, float& u, float& v) {
    f3 tmp = cross(d, e2);
    const float dx = dot(e1, tmp);
    if (fabsf(dx) < EPSILON) return -1.f;
    const float idx = 1.f / dx;
    const f3 rt = sub(o, p0);
    u = dot(rt, tmp) * idx;
    if (u < .0f || 1.f < u) return -1.f;
    tmp = cross(rt, e1);
    v = dot(d, tmp) * idx;
    if (v < .0f || 1.f < u + v) return -1.f;
    const float t = dot(e2, tmp) * idx;
    if (EPSILON < t) return t;
    return -1.f;
}
// FILL = false counts a ray's members and stores the count at offsets[r + 1]; FILL = true stores the members at
// offsets[r] + i while that is below min(offsets[r + 1], capacity), one 16-B store each: whatever the offsets hold,
// no store leaves the ray's segment or the first `capacity` hits.
template <bool FILL, bool COUNT, bool NB>
__global__ __launch_bounds__(BLOCK, BOUNCE_WAVES) void k_allhits(AllhitsArgs a) {
    const uint32_t n = a.n, T = a.T;
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    Counts c = {0, 0, 0, 0, 0};
    uint32_t nrays = 0;
    unsigned long long nhits = 0;
    bool has = false;
    uint32_t r = 0, cnt = 0;
    unsigned long long pos = 0, end = 0;   // FILL: the next hit's index and the end of the ray's segment
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // (hit, best, bl unused)
    float tmax = 0.f;
    f3 o = mk(0.f, 0.f, 0.f), d = o, inv = o;
    __shared__ uint32_t s_stk[SB][BLOCK];
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, n, has, [&](uint32_t p) {   // this lane takes the p-th ray of the walk order
            r = a.perm ? a.perm[p] : p;
            const float4 q0 = a.rays[2 * (size_t)r], q1 = a.rays[2 * (size_t)r + 1];
            o = mk(q0.x, q0.y, q0.z);
            tmax = q0.w;
            d = mk(q1.x, q1.y, q1.z);
            inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
            if (COUNT && a.count_hits) nrays++;
            const bool finite = fabsf(o.x) < INFINITY && fabsf(o.y) < INFINITY && fabsf(o.z) < INFINITY &&
                                fabsf(d.x) < INFINITY && fabsf(d.y) < INFINITY && fabsf(d.z) < INFINITY;
            const bool zero = d.x == 0.f && d.y == 0.f && d.z == 0.f;
            if (!finite || zero || !(tmax > 0.f)) {   // no walk: an empty list
                if (!FILL) a.offsets[(size_t)r + 1] = 0;
                else if (a.written) a.written[r] = 0;
            } else {
                has = true;
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
                cnt = 0;
                if (FILL) {
                    pos = a.offsets[r];
                    const unsigned long long e = a.offsets[(size_t)r + 1];
                    end = e < a.capacity ? e : a.capacity;
                }
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (!has) continue;
        bool done = false;
        const bool isleaf = (w.node & LEAF_BIT) != 0;
        // one fetch for every active lane, leaf or node, before the branch (k_query)
        v4f q0, q1, q2, q3;
        uint32_t cl = 0, cr = 0;
        if (!NB || isleaf) {
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(a.inner + w.node);
            q0 = rr[0]; q1 = rr[1]; q2 = rr[2]; q3 = rr[3];
            pin(q0); pin(q1); pin(q2); pin(q3);
            if (!NB && !isleaf) {
                const uint32_t own = __float_as_uint(q3.z);
                cl = child_slot(__float_as_uint(q3.x), own, 0);
                cr = child_slot(__float_as_uint(q3.y), own, 1);
            }
        } else {
            const ChildPair ch = nbt.children(w.node);
            cl = ch.cl;
            cr = ch.cr;
            q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
            q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
            q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
            q3 = v4f{0.f, 0.f, 0.f, 0.f};
        }
        float mn;
        if (--w.guard == 0) {
            c.overflow++;
            done = true;
        } else if (isleaf) {
            if (COUNT) c.leaf++;
            // (T == 1: the root is the leaf, and no parent tested its box -- words 10..15 of the record)
            if (T > 1 || query_box<true>(o, inv, f2v{q2.z, q2.w}, f2v{q3.y, q3.z}, q3.x, q3.w, false, 0.f, tmax, mn)) {
                float u = 0.f, v = 0.f;
                const float t = ray_triangle_tuv(o, d, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y),
                                                 mk(q1.z, q1.w, q2.x), u, v);
                if (t != -1.f && t <= tmax) {
                    if (!FILL || COUNT) cnt++;
                    if (FILL && pos < end) {
                        a.hits[pos] = make_float4(t, u, v, __uint_as_float(__float_as_uint(q2.y) & ~LEAF_BIT));
                        pos++;
                    }
                }
            }
            walk_pop(w, st);
            done = w.sp == -1;
        } else {
            if (COUNT) c.internal++;
            const bool lh = query_box<true>(o, inv, q0.xy, q0.zw, q2.x, q2.y, false, 0.f, tmax, mn);
            const bool rh = query_box<true>(o, inv, q1.xy, q1.zw, q2.z, q2.w, false, 0.f, tmax, mn);
            if (!lh && !rh) {
                walk_pop(w, st);
            } else if (lh && rh && w.sp + 1 >= limit) {   // the stack limit: both children lost, counted
                c.overflow++;
                walk_pop(w, st);
            } else {
                if (lh && rh) {   // left first: push the right child
                    st.store(w.sp, w.top);
                    w.sp++;
                    w.top = cr;
                }
                w.node = lh ? cl : cr;
            }
            done = w.sp == -1;
        }
        if (done) {
            if (!FILL) a.offsets[(size_t)r + 1] = cnt;
            else if (a.written) a.written[r] = (uint32_t)(pos - a.offsets[r]);   // (pos started there)
            if (COUNT && a.count_hits) nhits += cnt;
            has = false;
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[5] = {nrays, nhits, c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int k = 0; k < 4; k++) atomicAdd(&a.counts[k], v[k]);
            if (v[4]) atomicAdd(a.overflow, v[4]);
        }
    }
}

// ---- first-k ray queries (rtbvh_khits_async): caller rays in, each ray's k members with the smallest keys out ----
// k_knn's frame with k_allhits' rays.  A member is k_allhits' (the leaf's own box passes the any-hit rule with t_max,
// ray_triangle_tuv accepts at t <= t_max); its key is (tk bits << 32 | id) with tk = fmaxf(t, mn), mn the slab entry
// of its own leaf box: t is often a few ulps below mn, and with the box in the key no box around the leaf box starts
// above tk (the slab test is monotone in the box).  Each lane keeps k keys in ascending order, all
// started at the sentinel (t_max bits, 0xFFFFFFFF); `worst` caches slot k - 1, and a box -- a child's, or a leaf's
// own, tested at the leaf with the current bound -- is entered iff it passes the first two slab conditions and
// !(mn > the worst key's tk), the nearer child first by mn, left on a tie.  The bound only falls and is never below
// the final worst key's tk, so no member of the final list is pruned.
// The list lives in LDS beside the stack as k_knn's, [slot][lane]: an 8-B key column and a 4-B column with the
// leaf's slot in the leaf records, so the finished list's (t, u, v) are recomputed by the same ray_triangle_tuv on the
// same inputs -- the same bits -- instead of carried.  CAP (4, 8 or 16 slots) is the smallest tier that holds k;
// khits_blocks(CAP) blocks fit a CU's 160 KB and the launch bound asks for as many.
constexpr int khits_blocks(int cap) {   // blocks of 16 KB of stack and cap * 3 KB of list in 160 KB
    const int b = 160 / (16 + 3 * cap);
    return b < (int)BOUNCE_WAVES ? b : (int)BOUNCE_WAVES;
}
struct KhitsList {
    unsigned long long* key;   // this lane's LDS columns, slot j at [j * BLOCK]
    uint32_t* leaf;
    __device__ __forceinline__ void store(int j, uint64_t v, uint32_t l) {
        key[j * BLOCK] = v;
        leaf[j * BLOCK] = l;
    }
    __device__ __forceinline__ uint64_t load(int j) const { return key[j * BLOCK]; }
    __device__ __forceinline__ uint32_t load_leaf(int j) const { return leaf[j * BLOCK]; }
};
template <int CAP, bool COUNT, bool NB>
__global__ __launch_bounds__(BLOCK, khits_blocks(CAP)) void k_khits(KhitsArgs a) {
    const uint32_t n = a.n, T = a.T;
    const int k = (int)a.k;   // 1 .. CAP
    constexpr int ROUND = CAP >= 16 ? 8 : 4;   // keys an insertion fetches together
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    Counts c = {0, 0, 0, 0, 0};
    uint32_t nrays = 0, nfound = 0;
    bool has = false;
    uint32_t r = 0;
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // (hit, best, bl unused)
    uint64_t worst = 0;   // the list's slot k - 1
    float tmax = 0.f;
    f3 o = mk(0.f, 0.f, 0.f), d = o, inv = o;
    __shared__ uint32_t s_stk[SB][BLOCK];
    __shared__ unsigned long long s_key[CAP][BLOCK];
    __shared__ uint32_t s_leaf[CAP][BLOCK];
    KhitsList lst{&s_key[0][threadIdx.x], &s_leaf[0][threadIdx.x]};
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    const float4 none = make_float4(-1.f, 0.f, 0.f, __uint_as_float(INVALID));
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, n, has, [&](uint32_t p) {   // this lane takes the p-th ray of the walk order
            r = a.perm ? a.perm[p] : p;
            const float4 q0 = a.rays[2 * (size_t)r], q1 = a.rays[2 * (size_t)r + 1];
            o = mk(q0.x, q0.y, q0.z);
            tmax = q0.w;
            d = mk(q1.x, q1.y, q1.z);
            inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
            if (COUNT) nrays++;
            const bool finite = fabsf(o.x) < INFINITY && fabsf(o.y) < INFINITY && fabsf(o.z) < INFINITY &&
                                fabsf(d.x) < INFINITY && fabsf(d.y) < INFINITY && fabsf(d.z) < INFINITY;
            const bool zero = d.x == 0.f && d.y == 0.f && d.z == 0.f;
            if (!finite || zero || !(tmax > 0.f)) {   // no walk: every slot a miss
                for (int j = 0; j < k; j++) a.hits[(size_t)r * k + j] = none;
            } else {
                has = true;
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
                worst = (uint64_t)__float_as_uint(tmax) << 32 | 0xFFFFFFFFull;
                for (int j = 0; j < k; j++) lst.store(j, worst, 0u);
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (!has) continue;
        bool done = false;
        const bool isleaf = (w.node & LEAF_BIT) != 0;
        // one fetch for every active lane, leaf or node, before the branch (k_query)
        v4f q0, q1, q2, q3;
        uint32_t cl = 0, cr = 0;
        if (!NB || isleaf) {
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(a.inner + w.node);
            q0 = rr[0]; q1 = rr[1]; q2 = rr[2]; q3 = rr[3];
            pin(q0); pin(q1); pin(q2); pin(q3);
            if (!NB && !isleaf) {
                const uint32_t own = __float_as_uint(q3.z);
                cl = child_slot(__float_as_uint(q3.x), own, 0);
                cr = child_slot(__float_as_uint(q3.y), own, 1);
            }
        } else {
            const ChildPair ch = nbt.children(w.node);
            cl = ch.cl;
            cr = ch.cr;
            q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
            q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
            q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
            q3 = v4f{0.f, 0.f, 0.f, 0.f};
        }
        const float bound = key_t(worst);   // t_max until the list is full
        if (--w.guard == 0) {
            c.overflow++;
            done = true;
        } else if (isleaf) {
            if (COUNT) c.leaf++;
            float mn;   // the leaf's own box first, with the current bound (words 10..15 of the record)
            if (query_box<true>(o, inv, f2v{q2.z, q2.w}, f2v{q3.y, q3.z}, q3.x, q3.w, false, 0.f, bound, mn)) {
                float u = 0.f, v = 0.f;
                const float t = ray_triangle_tuv(o, d, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y),
                                                 mk(q1.z, q1.w, q2.x), u, v);
                const uint64_t cand = (uint64_t)__float_as_uint(fmaxf(t, mn)) << 32 | (__float_as_uint(q2.y) & ~LEAF_BIT);
                if (t != -1.f && t <= tmax && cand < worst) {   // into its place: the keys above it move one slot up
                    const uint32_t here = w.node & ~LEAF_BIT;
                    int j = k - 1;
                    uint64_t top = cand;   // slot k - 1 afterwards: the candidate, or what slot k - 2 held
                    for (bool go = j > 0, first = true; go; first = false) {
                        uint64_t b[ROUND];
                        uint32_t bl[ROUND];
#pragma unroll
                        for (int i = 0; i < ROUND; i++) {
                            const int at = j - 1 - i > 0 ? j - 1 - i : 0;
                            b[i] = lst.load(at);
                            bl[i] = lst.load_leaf(at);
                        }
                        if (first && !(b[0] < cand)) top = b[0];
#pragma unroll
                        for (int i = 0; i < ROUND; i++)   // (step i: j is the round's first j minus i, b[i] slot j - 1)
                            if (go) {
                                if (b[i] < cand) {
                                    go = false;
                                } else {
                                    lst.store(j, b[i], bl[i]);
                                    go = --j > 0;
                                }
                            }
                    }
                    lst.store(j, cand, here);
                    worst = top;
                }
            }
            walk_pop(w, st);
            done = w.sp == -1;
        } else {
            if (COUNT) c.internal++;
            float ml, mr;
            const bool lh = query_box<true>(o, inv, q0.xy, q0.zw, q2.x, q2.y, false, 0.f, bound, ml);
            const bool rh = query_box<true>(o, inv, q1.xy, q1.zw, q2.z, q2.w, false, 0.f, bound, mr);
            if (!lh && !rh) {
                walk_pop(w, st);
            } else if (lh && rh && w.sp + 1 >= limit) {   // the stack limit: both children lost, counted
                c.overflow++;
                walk_pop(w, st);
            } else {
                const bool swap = lh && rh && mr < ml;   // the nearer child first, left on a tie
                if (lh && rh) {
                    st.store(w.sp, w.top);   // push the other
                    w.sp++;
                    w.top = swap ? cl : cr;
                }
                w.node = swap ? cr : (lh ? cl : cr);
            }
            done = w.sp == -1;
        }
        if (done) {   // the list is in order, the sentinels all at its end: the listed leaves' hits, then misses
            for (int j = 0; j < k; j++) {
                const uint64_t key = lst.load(j);
                const bool found = (uint32_t)key != 0xFFFFFFFFu;
                float4 h = none;
                if (found) {
                    const v4f* rr = reinterpret_cast<const v4f*>(leaf + 4 * (size_t)lst.load_leaf(j));
                    const v4f l0 = rr[0], l1 = rr[1], l2 = rr[2];
                    float u = 0.f, v = 0.f;
                    const float t = ray_triangle_tuv(o, d, mk(l0.x, l0.y, l0.z), mk(l0.w, l1.x, l1.y),
                                                     mk(l1.z, l1.w, l2.x), u, v);
                    h = make_float4(t, u, v, __uint_as_float((uint32_t)key));
                }
                a.hits[(size_t)r * k + j] = h;
                if (COUNT) nfound += found;
            }
            has = false;
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[5] = {nrays, nfound, c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int i = 0; i < 4; i++) atomicAdd(&a.counts[i], v[i]);
            if (v[4]) atomicAdd(a.overflow, v[4]);
        }
    }
}

// ---- RTBVH_ALLHITS_BY_T: each ray's stored hits ordered by (t, tri), in place ---------------------------------
// t > EPSILON > 0, so the floats order as their bits and (t, tri) is the u64 key t bits << 32 | tri: a total order
// (a ray's list holds a triangle once).  A hit moves as one 16-B word.
__device__ __forceinline__ uint64_t hit_key(float4 h) {
    return (uint64_t)__float_as_uint(h.x) << 32 | __float_as_uint(h.w);
}
// One lane per ray: a list of up to ALLHITS_LANE_MAX hits is insertion-sorted where it lies (mostly already in
// order or nearly so, and L1-resident); the rays with longer lists are appended to `list`, one atomic a wave.
__global__ __launch_bounds__(BLOCK) void k_allhits_order_lane(float4* __restrict__ hits,
                                                              const unsigned long long* __restrict__ offsets,
                                                              const uint32_t* __restrict__ written, uint32_t n,
                                                              uint32_t* __restrict__ list, uint32_t* list_n) {
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t len = r < n ? written[r] : 0;
    const bool lng = len > ALLHITS_LANE_MAX;
    const uint32_t slot = wave_append(lng, list_n);   // (all lanes converged)
    if (lng) list[slot] = r;
    if (lng || len < 2) return;
    float4* h = hits + offsets[r];
    for (uint32_t i = 1; i < len; i++) {
        const float4 x = h[i];
        const uint64_t kx = hit_key(x);
        uint32_t j = i;
        while (j > 0) {
            const float4 y = h[j - 1];
            if (hit_key(y) <= kx) break;
            h[j] = y;
            j--;
        }
        if (j != i) h[j] = x;
    }
}
// The bitonic network with every comparator ascending (a stage's first step pairs i with its mirror in the 2k
// block, the others i with i + j), by one workgroup over a[0, len), len of any size: the network is that of the
// next power of two with +inf behind the list -- a comparator never moves its larger element down, so those stay
// where they are and a pair that reaches past the list is skipped.  `a`: LDS or global memory (the workgroup's
// own stores, ordered by the barrier).
template <class Ptr> __device__ __forceinline__ void order_pair(Ptr a, uint32_t i, uint32_t l) {
    const float4 x = a[i], y = a[l];
    if (hit_key(y) < hit_key(x)) {
        a[i] = y;
        a[l] = x;
    }
}
// stage k's first step: i in the lower half of its k-block, and its mirror
template <class Ptr> __device__ __forceinline__ void order_mirror(Ptr a, uint32_t len, uint32_t k, uint32_t tid) {
    const uint32_t hb = k >> 1;
    for (uint32_t p = tid;; p += BLOCK) {
        const uint32_t base = (p & ~(hb - 1)) << 1, off = p & (hb - 1);
        const uint32_t i = base | off, l = base + (k - 1 - off);
        if (i >= len) break;   // (i grows with p)
        if (l < len) order_pair(a, i, l);
    }
    __syncthreads();
}
// the steps at the distances j_first, j_first / 2, ... down to j_last: index i with bit j clear, and i + j
template <class Ptr>
__device__ __forceinline__ void order_steps(Ptr a, uint32_t len, uint32_t j_first, uint32_t j_last, uint32_t tid) {
    for (uint32_t j = j_first; j >= j_last && j >= 1; j >>= 1) {
        for (uint32_t p = tid;; p += BLOCK) {
            const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
            if (i >= len) break;
            if (l < len) order_pair(a, i, l);
        }
        __syncthreads();
    }
}
template <class Ptr> __device__ __forceinline__ void order_network(Ptr a, uint32_t len, uint32_t tid) {
    for (uint32_t k = 2; (k >> 1) < len; k <<= 1) {   // (len < 2^30: a list holds a triangle once)
        order_mirror(a, len, k, tid);
        order_steps(a, len, k >> 2, 1, tid);
    }
}
// One workgroup per listed ray.  A list of up to C = ALLHITS_LDS_MAX hits is sorted in LDS.  A longer one chunk by
// chunk: the stages up to C are each chunk's own sort (C divides a chunk's start, so the network's blocks are the
// chunks); of a later stage the steps at distances >= C run on global memory and the rest, again chunk-local, in
// LDS -- 2 + log2(P / C) (3 + log2(P / C)) / 2 passes over the list instead of one per step.
__global__ __launch_bounds__(BLOCK) void k_allhits_order_block(float4* hits, const unsigned long long* __restrict__ offsets,
                                                               const uint32_t* __restrict__ written,
                                                               const uint32_t* __restrict__ list,
                                                               const uint32_t* __restrict__ list_n) {
    constexpr uint32_t C = ALLHITS_LDS_MAX;
    static_assert((C & (C - 1)) == 0 && C >= 2, "the LDS chunk: a power of two");
    __shared__ float4 s_h[C];
    const uint32_t m = *list_n, tid = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < m; i += gridDim.x) {
        const uint32_t r = list[i], len = written[r];
        float4* g = hits + offsets[r];
        uint32_t k = C;   // k = C: the chunks' own sorts; then the stages 2C, 4C, ... while half a stage is inside the list
        do {
            if (k > C) {
                order_mirror(g, len, k, tid);
                order_steps(g, len, k >> 2, C, tid);
            }
            for (uint32_t c0 = 0; c0 < len; c0 += C) {
                const uint32_t n = len - c0 < C ? len - c0 : C;
                for (uint32_t e = tid; e < n; e += BLOCK) s_h[e] = g[c0 + e];
                __syncthreads();
                if (k == C) order_network(&s_h[0], n, tid);
                else order_steps(&s_h[0], n, C >> 1, 1, tid);
                for (uint32_t e = tid; e < n; e += BLOCK) g[c0 + e] = s_h[e];
                __syncthreads();   // (the next loads overwrite s_h; the next global step reads g)
            }
            k <<= 1;
        } while ((k >> 1) < len);
    }
}

// ---- box-overlap queries (rtbvh_overlap_async): caller boxes in, every triangle that meets the box out ----------
// k_within's frame and CSR protocol with a triangle id per entry.  The node test (B) is comparisons only:
// qlo <= hi && lo <= qhi on every axis, closed, false for a NaN.  It is monotone in the tree's box, so entering a
// child iff its box passes reaches every member with no margin; the walk is left-first, which is the
// order of a box's list.  A leaf tests its record's own box, then, under TRI, the triangle-box separating axes (T)
// of include/rtbvh.h, operation for operation, fp32 without contraction.
// (T): true iff one of the plane's axis and the nine edge axes separates the triangle {a, a + e1, a + e2} from the
// box [qlo, qhi].  A NaN compares false everywhere: it does not separate.
__device__ __forceinline__ bool tri_box_separated(f3 qlo, f3 qhi, f3 a, f3 e1, f3 e2) {
    const f3 c = mk((qlo.x + qhi.x) * 0.5f, (qlo.y + qhi.y) * 0.5f, (qlo.z + qhi.z) * 0.5f);
    const f3 h = mk((qhi.x - qlo.x) * 0.5f, (qhi.y - qlo.y) * 0.5f, (qhi.z - qlo.z) * 0.5f);
    const f3 v0 = mk(a.x - c.x, a.y - c.y, a.z - c.z);
    const f3 v1 = mk(v0.x + e1.x, v0.y + e1.y, v0.z + e1.z);
    const f3 v2 = mk(v0.x + e2.x, v0.y + e2.y, v0.z + e2.z);
    const f3 nn = mk(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
    const float d = (nn.x * v0.x + nn.y * v0.y) + nn.z * v0.z;
    const float r = (h.x * fabsf(nn.x) + h.y * fabsf(nn.y)) + h.z * fabsf(nn.z);
    if (d > r || d < -r) return true;
    bool sep = false;
#pragma unroll
    for (int k = 0; k < 3; k++) {   // unrolled: kept as a loop (unroll 1) it takes 15 registers more, to select f
        const f3 f = k == 0 ? e1 : k == 1 ? mk(e2.x - e1.x, e2.y - e1.y, e2.z - e1.z) : e2;
        const f3 g = mk(fabsf(f.x), fabsf(f.y), fabsf(f.z));
        float p0 = v0.z * f.y - v0.y * f.z, p1 = v1.z * f.y - v1.y * f.z, p2 = v2.z * f.y - v2.y * f.z;   // x
        float rr = h.y * g.z + h.z * g.y;
        sep |= fminf(fminf(p0, p1), p2) > rr || fmaxf(fmaxf(p0, p1), p2) < -rr;
        p0 = v0.x * f.z - v0.z * f.x, p1 = v1.x * f.z - v1.z * f.x, p2 = v2.x * f.z - v2.z * f.x;           // y
        rr = h.x * g.z + h.z * g.x;
        sep |= fminf(fminf(p0, p1), p2) > rr || fmaxf(fmaxf(p0, p1), p2) < -rr;
        p0 = v0.y * f.x - v0.x * f.y, p1 = v1.y * f.x - v1.x * f.y, p2 = v2.y * f.x - v2.x * f.y;           // z
        rr = h.x * g.y + h.y * g.x;
        sep |= fminf(fminf(p0, p1), p2) > rr || fmaxf(fmaxf(p0, p1), p2) < -rr;
    }
    return sep;
}

// (B) on a box given as its corners
__device__ __forceinline__ bool boxes_meet(f3 qlo, f3 qhi, f3 lo, f3 hi) {
    return qlo.x <= hi.x && lo.x <= qhi.x && qlo.y <= hi.y && lo.y <= qhi.y && qlo.z <= hi.z && lo.z <= qhi.z;
}

// FILL = false counts a box's members and stores the count at offsets[r + 1]; FILL = true stores the ids at
// offsets[r] + i while that is below min(offsets[r + 1], capacity), as k_within its pairs: whatever the offsets
// hold, no store leaves the box's segment or the first `capacity` ids.
// Every instance fits 64 registers without a spill at 8 waves per SIMD.
template <bool FILL, bool COUNT, bool NB, bool TRI>
__global__ __launch_bounds__(BLOCK, BOUNCE_WAVES) void k_overlap(OverlapArgs a) {
    const uint32_t n = a.n, T = a.T;
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    Counts c = {0, 0, 0, 0, 0};
    uint32_t nboxes = 0;
    unsigned long long nids = 0;
    bool has = false;
    uint32_t r = 0, cnt = 0;
    unsigned long long pos = 0, end = 0;   // FILL: the next id's index and the end of the box's segment
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // (hit, best, bl unused)
    f3 qlo = mk(0.f, 0.f, 0.f), qhi = mk(0.f, 0.f, 0.f);
    __shared__ uint32_t s_stk[SB][BLOCK];
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, n, has, [&](uint32_t k) {   // this lane takes the k-th box of the walk order
            r = a.perm ? a.perm[k] : k;
            const float4 b0 = a.boxes[2 * (size_t)r], b1 = a.boxes[2 * (size_t)r + 1];
            qlo = mk(b0.x, b0.y, b0.z);
            qhi = mk(b1.x, b1.y, b1.z);
            if (COUNT && a.count_ids) nboxes++;
            const bool finite = fabsf(qlo.x) < INFINITY && fabsf(qlo.y) < INFINITY && fabsf(qlo.z) < INFINITY &&
                                fabsf(qhi.x) < INFINITY && fabsf(qhi.y) < INFINITY && fabsf(qhi.z) < INFINITY;
            if (!finite || !(qlo.x <= qhi.x && qlo.y <= qhi.y && qlo.z <= qhi.z)) {   // no walk: an empty list
                if (!FILL) a.offsets[(size_t)r + 1] = 0;
            } else {
                has = true;
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
                cnt = 0;
                if (FILL) {
                    pos = a.offsets[r];
                    const unsigned long long e = a.offsets[(size_t)r + 1];
                    end = e < a.capacity ? e : a.capacity;
                }
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (!has) continue;
        bool done = false;
        const bool isleaf = (w.node & LEAF_BIT) != 0;
        // one fetch for every active lane, leaf or node, before the branch (k_nearest)
        v4f q0, q1, q2, q3;
        uint32_t cl = 0, cr = 0;
        if (!NB || isleaf) {
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(a.inner + w.node);
            q0 = rr[0]; q1 = rr[1]; q2 = rr[2]; q3 = rr[3];
            pin(q0); pin(q1); pin(q2); pin(q3);
            if (!NB && !isleaf) {
                const uint32_t own = __float_as_uint(q3.z);
                cl = child_slot(__float_as_uint(q3.x), own, 0);
                cr = child_slot(__float_as_uint(q3.y), own, 1);
            }
        } else {
            const ChildPair ch = nbt.children(w.node);
            cl = ch.cl;
            cr = ch.cr;
            q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
            q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
            q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
            q3 = v4f{0.f, 0.f, 0.f, 0.f};
        }
        if (--w.guard == 0) {
            c.overflow++;
            done = true;
        } else if (isleaf) {
            if (COUNT) c.leaf++;
            bool in = boxes_meet(qlo, qhi, mk(q2.z, q2.w, q3.x), mk(q3.y, q3.z, q3.w));   // the leaf's own box first
            if (TRI && in)
                in = !tri_box_separated(qlo, qhi, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), mk(q1.z, q1.w, q2.x));
            if (in) {
                if (!FILL || COUNT) cnt++;
                if (FILL && pos < end) {
                    a.ids[pos] = __float_as_uint(q2.y) & ~LEAF_BIT;
                    pos++;
                }
            }
            walk_pop(w, st);
            done = w.sp == -1;
        } else {
            if (COUNT) c.internal++;
            const bool lh = boxes_meet(qlo, qhi, mk(q0.x, q0.y, q2.x), mk(q0.z, q0.w, q2.y));
            const bool rh = boxes_meet(qlo, qhi, mk(q1.x, q1.y, q2.z), mk(q1.z, q1.w, q2.w));
            if (!lh && !rh) {
                walk_pop(w, st);
            } else if (lh && rh && w.sp + 1 >= limit) {   // the stack limit: both children lost, counted
                c.overflow++;
                walk_pop(w, st);
            } else {
                if (lh && rh) {   // left first: push the right child
                    st.store(w.sp, w.top);
                    w.sp++;
                    w.top = cr;
                }
                w.node = lh ? cl : cr;
            }
            done = w.sp == -1;
        }
        if (done) {
            if (!FILL) a.offsets[(size_t)r + 1] = cnt;
            if (COUNT && a.count_ids) nids += cnt;
            has = false;
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[5] = {nboxes, nids, c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int k = 0; k < 4; k++) atomicAdd(&a.counts[k], v[k]);
            if (v[4]) atomicAdd(a.overflow, v[4]);
        }
    }
}

// RTBVH_OVERLAP_SORT's key: the 30-bit Morton code of the box's centre in the root box (k_nearest_keys' code)
__global__ __launch_bounds__(BLOCK) void k_overlap_keys(const float4* __restrict__ boxes, uint32_t n,
                                                        const float* __restrict__ box, uint32_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 lo = boxes[2 * (size_t)i], hi = boxes[2 * (size_t)i + 1];
    keys[i] = spread9(q9((lo.x + hi.x) * 0.5f, box[0], box[3])) << 2 |
              spread9(q9((lo.y + hi.y) * 0.5f, box[1], box[4])) << 1 | spread9(q9((lo.z + hi.z) * 0.5f, box[2], box[5]));
    vals[i] = i;
}

// ---- region queries (rtbvh_region_async): up to six planes in, every triangle within them out -------------------
// k_overlap's frame and CSR protocol with a plane set for the query.  The value of plane {n, d} at x is
// s = ((t_x + t_y) + t_z) + d with t_k = n_k == 0 ? +0 : n_k * x_k, fp32 without contraction; m and M of a box are s
// at its near and far corners (include/rtbvh.h).  Rounded products and sums are monotone, so m(node) <= m(leaf) <=
// s(v) <= M(leaf) <= M(node) for nested boxes and a vertex inside them:
//  * prune: a child is entered iff m <= 0 on every plane, which every box above a (B) member passes;
//  * accept: an internal child with M <= 0 on every plane holds members only, so its leaf range topo[child].zw is
//    taken whole -- counted in one step, copied by the wave in the fill pass -- while no leaf box holds a NaN
//    (*leaf_nan, k_leaf_nan: node boxes drop NaNs, so an all-NaN triangle can sit inside an accepted box).
// Both passes walk alike (the stack limit loses the same subtrees in both).  The walk is left-first and a list is in
// sort order, so an accepted right child behind an entered left one waits on the stack as an ordinary node: its
// children pass the accept when it is popped.  The root's own box is the root-box words: a region that holds it takes
// [0, T - 1] with no step at all, one that misses it has an empty list.
// The 24 plane floats stay in registers.  The launch bounds are chosen from the instances' register counts
// (DESIGN.md 5o): the instances without COUNT take 59-70 VGPRs and keep 7 waves per SIMD with no VGPR spilled (at 8,
// the fill instances spill 2-15 and the C5 fill pass took 1.4 times as long); the counting ones take up to 84 and
// keep 5.  Every instance also keeps 39-54 uniform values (pointer arguments, exec masks) in VGPR lanes, reloaded
// inside the loop by v_readlane: no memory traffic, counted in DESIGN.md 5o.
#ifndef RTBVH_REGION_WAVES   // (an A/B build sets another launch bound: EXTRA=-DRTBVH_REGION_WAVES=<n>)
#define RTBVH_REGION_WAVES 7
#endif
#ifndef RTBVH_REGION_COUNT_WAVES
#define RTBVH_REGION_COUNT_WAVES 5
#endif
constexpr uint32_t REGION_WAVES = RTBVH_REGION_WAVES, REGION_COUNT_WAVES = RTBVH_REGION_COUNT_WAVES;
// an accepted range of up to this many ids is copied by its own lane, a longer one by the whole wave (C5 boxes at
// ten displacements, whose ranges hold 3 ids on average: the fill pass 380 ms at 4, 388 at 0, 420 at 16;
// profiles/region_ab.json)
#ifndef RTBVH_REGION_LANE_COPY
#define RTBVH_REGION_LANE_COPY 4
#endif
constexpr uint32_t REGION_LANE_COPY = RTBVH_REGION_LANE_COPY;

__device__ __forceinline__ float plane_term(float n, float x) { return n == 0.f ? 0.f : n * x; }
__device__ __forceinline__ float plane_at(float nx, float ny, float nz, float d, f3 x) {
    return ((plane_term(nx, x.x) + plane_term(ny, x.y)) + plane_term(nz, x.z)) + d;
}
// enter: m <= 0 on every plane; inside: and M <= 0 on every plane.  A NaN fails either.
__device__ __forceinline__ void planes_box(const float (&pl)[24], f3 lo, f3 hi, bool& enter, bool& inside) {
    bool e = true, in = true;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const float nx = pl[4 * i], ny = pl[4 * i + 1], nz = pl[4 * i + 2], d = pl[4 * i + 3];
        const bool px = nx >= 0.f, py = ny >= 0.f, pz = nz >= 0.f;
        const float m = plane_at(nx, ny, nz, d, mk(px ? lo.x : hi.x, py ? lo.y : hi.y, pz ? lo.z : hi.z));
        const float M = plane_at(nx, ny, nz, d, mk(px ? hi.x : lo.x, py ? hi.y : lo.y, pz ? hi.z : lo.z));
        e &= m <= 0.f;
        in &= M <= 0.f;
    }
    enter = e;
    inside = e && in;
}
// (V): on every plane one of the vertices a, clamp(a + e1), clamp(a + e2) lies on the inner side
__device__ __forceinline__ bool planes_vertices(const float (&pl)[24], f3 a, f3 e1, f3 e2, f3 lo, f3 hi) {
    const f3 v1 = mk(fmaxf(lo.x, fminf(hi.x, a.x + e1.x)), fmaxf(lo.y, fminf(hi.y, a.y + e1.y)),
                     fmaxf(lo.z, fminf(hi.z, a.z + e1.z)));   // (k_clearance's clamp_box)
    const f3 v2 = mk(fmaxf(lo.x, fminf(hi.x, a.x + e2.x)), fmaxf(lo.y, fminf(hi.y, a.y + e2.y)),
                     fmaxf(lo.z, fminf(hi.z, a.z + e2.z)));
    bool in = true;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const float nx = pl[4 * i], ny = pl[4 * i + 1], nz = pl[4 * i + 2], d = pl[4 * i + 3];
        in &= plane_at(nx, ny, nz, d, a) <= 0.f || plane_at(nx, ny, nz, d, v1) <= 0.f ||
              plane_at(nx, ny, nz, d, v2) <= 0.f;
    }
    return in;
}

// FILL = false counts a region's members and stores the count at offsets[r + 1]; FILL = true stores the ids at
// offsets[r] + i while that is below min(offsets[r + 1], capacity), as k_overlap: whatever the offsets hold, no
// store -- a lane's own or the wave's range copy -- leaves the region's segment or the first `capacity` ids.
// SPLIT (k_region_piece): the queue holds the n << kshift piece slots k_region_expand filled instead of the n
// regions.  A lane takes one piece: a NODE piece starts the same step loop at its own node with an empty stack (the
// node's box is known to enter), a RANGE piece is the accept at the claim, an EMPTY slot is no work.  The sizes pass
// stores piece p's count at poff[p + 1]; the fill pass starts piece p of region r at offsets[r] + (poff[p] -
// poff[r << kshift]) and clamps every store like the plain walk.  msteps: the longest piece walk (COUNT).
template <bool FILL, bool COUNT, bool NB, bool TRI, bool SPLIT>
__device__ __forceinline__ void region_walk(const RegionArgs& a, const uint2* __restrict__ pieces,
                                            unsigned long long* __restrict__ poff, uint32_t kshift,
                                            unsigned long long* __restrict__ msteps) {
    const uint32_t n = SPLIT ? a.n << kshift : a.n, T = a.T;
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    const bool acc_on = a.accept && *a.leaf_nan == 0u;   // (one word for the whole grid)
    const f3 rootlo = mk(a.rootbox[0], a.rootbox[1], a.rootbox[2]), roothi = mk(a.rootbox[3], a.rootbox[4], a.rootbox[5]);
    Counts c = {0, 0, 0, 0, 0};
    uint32_t nregions = 0, nacc = 0;
    unsigned long long nids = 0, naccids = 0;
    bool has = false;
    uint32_t r = 0, cnt = 0;
    uint32_t slot = 0, psteps = 0, pmax = 0;   // SPLIT: the piece's slot; with COUNT its steps, and the most of any
    unsigned long long pos = 0, end = 0;   // FILL: the next id's index and the end of the region's segment
    uint32_t plo = 0, plen = 0;            // FILL: an accepted range still to copy, leaves [plo, plo + plen)
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // (hit, best, bl unused)
    float pl[24];
#pragma unroll
    for (int k = 0; k < 24; k++) pl[k] = 0.f;
    __shared__ uint32_t s_stk[SB][BLOCK];
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, n, has, [&](uint32_t k) {   // this lane takes the k-th region
            if (SPLIT) {   // ... the k-th piece slot
                slot = k;
                r = k >> kshift;
                const uint2 item = pieces[k];
                if (COUNT && a.count_ids && (k & ((1u << kshift) - 1u)) == 0) nregions++;   // (its region's first slot)
                if (item.y == 0u) {   // EMPTY
                    if (!FILL) poff[(size_t)k + 1] = 0;
                    return;
                }
                const float4* src = a.regions + 6 * (size_t)r;
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    const float4 p = src[i];
                    pl[4 * i] = p.x; pl[4 * i + 1] = p.y; pl[4 * i + 2] = p.z; pl[4 * i + 3] = p.w;
                }
                has = true;
                cnt = 0;
                if (COUNT) psteps = 0;
                if (FILL) {
                    pos = a.offsets[r] + (poff[k] - poff[(size_t)r << kshift]);
                    const unsigned long long e = a.offsets[(size_t)r + 1];
                    end = e < a.capacity ? e : a.capacity;
                }
                w = walk_start(item.x, T);   // a NODE piece: from its own node (LEAF_BIT | j: the leaf step alone)
                if (item.y != REGION_PIECE_NODE) {   // a RANGE piece: every leaf of [item.x, item.x + item.y), no step
                    w.sp = -1;
                    cnt = item.y;
                    if (FILL) {
                        plo = item.x;
                        plen = item.y;
                    }
                    if (COUNT) {
                        nacc++;
                        if (a.count_ids) naccids += item.y;
                    }
                }
                return;
            }
            r = k;
            const float4* src = a.regions + 6 * (size_t)r;
            bool finite = true;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const float4 p = src[i];
                pl[4 * i] = p.x; pl[4 * i + 1] = p.y; pl[4 * i + 2] = p.z; pl[4 * i + 3] = p.w;
                finite &= fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY &&
                          fabsf(p.w) < INFINITY;
            }
            if (COUNT && a.count_ids) nregions++;
            bool enter = false, inside = false;
            if (finite) {
                if (T == 1) enter = true;   // (the leaf test alone)
                else planes_box(pl, rootlo, roothi, enter, inside);
            }
            if (!enter) {   // no walk: an empty list
                if (!FILL) a.offsets[(size_t)r + 1] = 0;
            } else {
                has = true;
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
                cnt = 0;
                if (FILL) {
                    pos = a.offsets[r];
                    const unsigned long long e = a.offsets[(size_t)r + 1];
                    end = e < a.capacity ? e : a.capacity;
                }
                if (T > 1 && inside && acc_on) {   // the root accepted: every leaf, no step
                    w.sp = -1;
                    cnt = T;
                    if (FILL) {
                        plo = 0;
                        plen = T;
                    }
                    if (COUNT) {
                        nacc++;
                        if (a.count_ids) naccids += T;
                    }
                }
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        bool done = false;
        if (has && w.sp < 0) {
            done = true;   // (accepted at the claim)
        } else if (has) {
            const bool isleaf = (w.node & LEAF_BIT) != 0;
            // one fetch for every active lane, leaf or node, before the branch (k_nearest)
            v4f q0, q1, q2, q3;
            uint32_t cl = 0, cr = 0, lid = 0, rid = 0;   // the children as the walk keeps them, and as topo indexes them
            if (!NB || isleaf) {
                const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                       : reinterpret_cast<const v4f*>(a.inner + w.node);
                q0 = rr[0]; q1 = rr[1]; q2 = rr[2]; q3 = rr[3];
                pin(q0); pin(q1); pin(q2); pin(q3);
                if (!NB && !isleaf) {
                    const uint32_t own = __float_as_uint(q3.z);
                    lid = __float_as_uint(q3.x);
                    rid = __float_as_uint(q3.y);
                    cl = child_slot(lid, own, 0);
                    cr = child_slot(rid, own, 1);
                }
            } else {
                const ChildPair ch = nbt.children(w.node);
                cl = lid = ch.cl;
                cr = rid = ch.cr;
                q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
                q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
                q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
                q3 = v4f{0.f, 0.f, 0.f, 0.f};
            }
            if (SPLIT && COUNT) psteps++;
            if (--w.guard == 0) {
                c.overflow++;
                done = true;
            } else if (isleaf) {
                if (COUNT) c.leaf++;
                const f3 lo = mk(q2.z, q2.w, q3.x), hi = mk(q3.y, q3.z, q3.w);
                bool in, whole;
                planes_box(pl, lo, hi, in, whole);   // (B) on the leaf's own box
                if (TRI && in)
                    in = planes_vertices(pl, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), mk(q1.z, q1.w, q2.x), lo, hi);
                if (in) {
                    if (!FILL || COUNT) cnt++;
                    if (FILL && pos < end) {
                        a.ids[pos] = __float_as_uint(q2.y) & ~LEAF_BIT;
                        pos++;
                    }
                }
                walk_pop(w, st);
                done = w.sp == -1;
            } else {
                if (COUNT) c.internal++;
                bool lh, li, rh, ri;
                planes_box(pl, mk(q0.x, q0.y, q2.x), mk(q0.z, q0.w, q2.y), lh, li);
                planes_box(pl, mk(q1.x, q1.y, q2.z), mk(q1.z, q1.w, q2.w), rh, ri);
                const bool la = li && acc_on && !(cl & LEAF_BIT);
                const bool ra = ri && acc_on && !(cr & LEAF_BIT) && (la || !lh);   // (behind an entered left child: later)
                if (la || ra) {
                    uint32_t lo = 0, len = 0;
                    if (la) {
                        const uint4 t = a.topo[lid];
                        lo = t.z;
                        len = t.w - t.z + 1;
                    }
                    if (ra) {   // (behind an accepted left child its range follows the left one's)
                        const uint4 t = a.topo[rid];
                        if (!la) lo = t.z;
                        len += t.w - t.z + 1;
                    }
                    if (!FILL || COUNT) cnt += len;
                    if (COUNT) {
                        nacc += (la ? 1u : 0u) + (ra ? 1u : 0u);
                        if (a.count_ids) naccids += len;
                    }
                    if (FILL) {
                        plo = lo;
                        plen = len;
                    }
                }
                const bool le = lh && !la, re = rh && !ra;   // the children still to walk
                if (!le && !re) {
                    walk_pop(w, st);
                } else if (le && re && w.sp + 1 >= limit) {   // the stack limit: both children lost, counted
                    c.overflow++;
                    walk_pop(w, st);
                } else {
                    if (le && re) {   // left first: push the right child
                        st.store(w.sp, w.top);
                        w.sp++;
                        w.top = cr;
                    }
                    w.node = le ? cl : cr;
                }
                done = w.sp == -1;
            }
        }
        if (FILL) {   // every lane of the wave is here: the accepted ranges of this step, the ids from word 9
            if (plen > 0 && plen <= REGION_LANE_COPY) {
                for (uint32_t i = 0; i < plen && pos < end; i++, pos++)
                    a.ids[pos] = __float_as_uint(leaf[4 * (size_t)(plo + i) + 2].y) & ~LEAF_BIT;
                plen = 0;
            }
            uint64_t pm = __ballot(plen > 0);
            while (pm) {
                const uint32_t src = (uint32_t)__ffsll((unsigned long long)pm) - 1u;
                pm &= pm - 1;
                const uint32_t blo = __shfl(plo, (int)src, 64), blen = __shfl(plen, (int)src, 64);
                const unsigned long long bpos = __shfl(pos, (int)src, 64), bend = __shfl(end, (int)src, 64);
                const unsigned long long room = bpos < bend ? bend - bpos : 0ull;
                const uint32_t m = room < blen ? (uint32_t)room : blen;
                for (uint32_t i = lane; i < m; i += 64)
                    a.ids[bpos + i] = __float_as_uint(leaf[4 * (size_t)(blo + i) + 2].y) & ~LEAF_BIT;
                if (lane == src) {
                    pos += m;
                    plen = 0;
                }
            }
        }
        if (done) {
            if (!FILL) {
                if (SPLIT) poff[(size_t)slot + 1] = cnt;
                else a.offsets[(size_t)r + 1] = cnt;
            }
            if (COUNT && a.count_ids) nids += cnt;
            if (SPLIT && COUNT) pmax = psteps > pmax ? psteps : pmax;
            has = false;
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[7] = {nregions, nids, c.internal, c.leaf, nacc, naccids, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int k = 0; k < 6; k++) atomicAdd(&a.counts[k], v[k]);
            if (v[6]) atomicAdd(a.overflow, v[6]);
        }
    }
    if (SPLIT && COUNT) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = __shfl_xor(pmax, off, 64);
            pmax = o > pmax ? o : pmax;
        }
        if (lane == 0 && pmax) atomicMax(msteps, (unsigned long long)pmax);
    }
}
template <bool FILL, bool COUNT, bool NB, bool TRI>
__global__ __launch_bounds__(BLOCK, COUNT ? REGION_COUNT_WAVES : REGION_WAVES) void k_region(RegionArgs a) {
    region_walk<FILL, COUNT, NB, TRI, false>(a, nullptr, nullptr, 0u, nullptr);
}
template <bool FILL, bool COUNT, bool NB, bool TRI>
__global__ __launch_bounds__(BLOCK, COUNT ? REGION_COUNT_WAVES : REGION_WAVES) void k_region_piece(RegionSplitArgs sa) {
    region_walk<FILL, COUNT, NB, TRI, true>(sa.r, sa.pieces, sa.poff, sa.kshift, sa.split + 2);
}

// The expansion of a split region query: one wave a region, the ordered frontier in LDS as two lists of K pieces
// (16 B x K: 64 KB at K = 4096), read from one and written to the other each round.  A wave needs no barrier between
// its own rounds and no hand-off to another wave; the kernel boundary hands the pieces to k_region_piece.  A region
// holds at most K pieces whatever the wave count, so a workgroup of four waves would only share the same passes of 64
// items among them at the price of a barrier per pass.
// A round replaces the first K - len NODE pieces (each adds one piece net at most, so the list still fits) by the
// outcome of planes_box on their two children, left then right: dropped, RANGE (internal, inside, accepts on), or
// NODE (a leaf child: LEAF_BIT | j).  Ranks by ballot: the order of the list is the order of the leaves, whatever
// ran when.  It ends when no NODE is left, the list is full, or after REGION_SPLIT_ROUNDS rounds (a chain of one-leaf
// children adds one piece a round); k_region_piece walks the NODEs that remain.
template <bool NB>
__global__ __launch_bounds__(64) void k_region_expand(RegionSplitArgs sa, bool count) {
    extern __shared__ uint2 s_front[];
    const RegionArgs& a = sa.r;
    const uint32_t K = 1u << sa.kshift, r = blockIdx.x, lane = threadIdx.x, T = a.T;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    const bool acc_on = a.accept && *a.leaf_nan == 0u;
    uint2 *A = s_front, *B = s_front + K;
    float pl[24];
    bool finite = true;
    {
        const float4* src = a.regions + 6 * (size_t)r;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const float4 p = src[i];
            pl[4 * i] = p.x; pl[4 * i + 1] = p.y; pl[4 * i + 2] = p.z; pl[4 * i + 3] = p.w;
            finite &= fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY && fabsf(p.w) < INFINITY;
        }
    }
    uint32_t len = 0, tests = 0;   // (len: the same in every lane)
    {   // the root, as k_region's claim
        bool enter = false, inside = false;
        if (finite) {
            if (T == 1) enter = true;
            else planes_box(pl, mk(a.rootbox[0], a.rootbox[1], a.rootbox[2]), mk(a.rootbox[3], a.rootbox[4], a.rootbox[5]),
                            enter, inside);
        }
        if (enter) {
            len = 1;
            if (lane == 0)
                A[0] = T > 1 && inside && acc_on ? make_uint2(0u, T)
                                                 : make_uint2(NB ? nbt.root(T) : rec.root(T), REGION_PIECE_NODE);
        }
    }
    __syncthreads();
    for (uint32_t round = 0; round < REGION_SPLIT_ROUNDS && len > 0 && len < K; round++) {
        const uint32_t budget = K - len;
        uint32_t nnode = 0, nout = 0;
        for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t i = base + lane;
            const bool valid = i < len;
            const uint2 item = valid ? A[i] : make_uint2(0u, 0u);
            const bool isnode = valid && item.y == REGION_PIECE_NODE && !(item.x & LEAF_BIT);
            const uint64_t nm = __ballot(isnode);
            const bool expand = isnode && nnode + lane_rank(nm) < budget;
            nnode += (uint32_t)__popcll(nm);
            uint2 o0 = item, o1 = make_uint2(0u, 0u);
            uint32_t no = valid ? 1u : 0u;
            if (expand) {
                uint32_t cl, cr, lid, rid;
                f3 llo, lhi, rlo, rhi;
                if (!NB) {
                    const v4f* rr = reinterpret_cast<const v4f*>(a.inner + item.x);
                    const v4f q0 = rr[0], q1 = rr[1], q2 = rr[2], q3 = rr[3];
                    const uint32_t own = __float_as_uint(q3.z);
                    lid = __float_as_uint(q3.x);
                    rid = __float_as_uint(q3.y);
                    cl = child_slot(lid, own, 0);
                    cr = child_slot(rid, own, 1);
                    llo = mk(q0.x, q0.y, q2.x); lhi = mk(q0.z, q0.w, q2.y);
                    rlo = mk(q1.x, q1.y, q2.z); rhi = mk(q1.z, q1.w, q2.w);
                } else {
                    const ChildPair ch = nbt.children(item.x);
                    cl = lid = ch.cl;
                    cr = rid = ch.cr;
                    llo = mk(ch.llo.x, ch.llo.y, ch.lz0); lhi = mk(ch.lhi.x, ch.lhi.y, ch.lz1);
                    rlo = mk(ch.rlo.x, ch.rlo.y, ch.rz0); rhi = mk(ch.rhi.x, ch.rhi.y, ch.rz1);
                }
                tests++;
                bool lh, li, rh, ri;
                planes_box(pl, llo, lhi, lh, li);
                planes_box(pl, rlo, rhi, rh, ri);
                no = 0;
                if (lh) {
                    o0 = make_uint2(cl, REGION_PIECE_NODE);
                    if (li && acc_on && !(cl & LEAF_BIT)) {
                        const uint4 t = a.topo[lid];
                        o0 = make_uint2(t.z, t.w - t.z + 1);
                    }
                    no = 1;
                }
                if (rh) {
                    uint2 o = make_uint2(cr, REGION_PIECE_NODE);
                    if (ri && acc_on && !(cr & LEAF_BIT)) {
                        const uint4 t = a.topo[rid];
                        o = make_uint2(t.z, t.w - t.z + 1);
                    }
                    if (no) o1 = o;
                    else o0 = o;
                    no++;
                }
            }
            const uint64_t m1 = __ballot(no >= 1u), m2 = __ballot(no == 2u);
            const uint32_t at = nout + lane_rank(m1) + lane_rank(m2);   // (<= len + expanded <= K)
            if (no >= 1u) B[at] = o0;
            if (no == 2u) B[at + 1] = o1;
            nout += (uint32_t)__popcll(m1) + (uint32_t)__popcll(m2);
        }
        __syncthreads();
        uint2* t = A;
        A = B;
        B = t;
        len = nout;
        if (nnode == 0) break;   // (copied as it was: final)
    }
    uint2* out = sa.pieces + ((size_t)r << sa.kshift);
    for (uint32_t i = lane; i < K; i += 64) out[i] = i < len ? A[i] : make_uint2(0u, 0u);
    if (count) {
        const unsigned long long t = wave_sum((unsigned long long)tests);
        if (lane == 0) {
            if (len) atomicAdd(&sa.split[0], (unsigned long long)len);
            if (t) {
                atomicAdd(&sa.split[1], t);
                atomicAdd(&a.counts[2], t);
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_region_offsets(const unsigned long long* __restrict__ poff,
                                                          unsigned long long* __restrict__ offsets, uint32_t n,
                                                          uint32_t kshift) {
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r <= n) offsets[r] = poff[(size_t)r << kshift];
}

// *word = 1 if a leaf box (words 10..15 of a leaf record) holds a NaN; the caller zeroes it first
__global__ __launch_bounds__(BLOCK) void k_leaf_nan(const float4* __restrict__ leaf, uint32_t T, uint32_t* __restrict__ word) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= T) return;
    const float4 w2 = leaf[4 * (size_t)i + 2], w3 = leaf[4 * (size_t)i + 3];
    if (w2.z != w2.z || w2.w != w2.w || w3.x != w3.x || w3.y != w3.y || w3.z != w3.z || w3.w != w3.w) *word = 1u;
}

// ---- signed-distance queries (rtbvh_signed_async): caller points in, rtbvh_nearest's fields and crossing counts out --
// Two passes over the same walk order.  The closest-point pass is k_nearest itself, storing into the record: an
// rtbvh_signed is an rtbvh_nearest whose last word (0 there) holds the flags.  k_signed is the ray pass on the same
// frame: a lane owns one point and takes it through the ray phases j = 0 .. R - 1 (R = 1, or 3 with VOTE3), each a
// walk from the root that counts the triangles ray j crosses -- origin the point, direction the constant D_j,
// t_max = +inf.  A child is entered iff its box passes the any-hit rule query_box<true>, left first; the rule is
// monotone in the box, so every leaf whose own box passes is reached, and a leaf -- its box tested
// at its parent with the same floats, or here when the root is the leaf -- counts iff signed_cross holds.  A finished
// phase folds its count into `flags` (parity bit j + 1, the saturated byte j + 1); the last one adds `inside` and
// stores the word.  NEAR: the closest-point pass ran before and the nearest fields are left alone; otherwise
// (RTBVH_SIGNED_INSIDE_ONLY) this pass stores "no result" there.
// One fused kernel -- the closest-point walk as a phase 0 of the same lane -- gave the same bits and was 2.6-6.4%
// slower in eleven cases of sixteen, never more than 1.4% faster (profiles/signed_ab.json): the passes stay apart.
// The directions have no zero component and are exact in fp32; their inverses are the compile-time IEEE quotients.
__device__ __forceinline__ f3 signed_dir(uint32_t j) {
    return j == 0 ? mk(0.75f, 0.5f, 0.4375f) : j == 1 ? mk(-0.5f, 0.75f, -0.4375f) : mk(0.4375f, -0.5f, -0.75f);
}
__device__ __forceinline__ f3 signed_inv(uint32_t j) {
    return j == 0   ? mk(1.f / 0.75f, 1.f / 0.5f, 1.f / 0.4375f)
           : j == 1 ? mk(1.f / -0.5f, 1.f / 0.75f, 1.f / -0.4375f)
                    : mk(1.f / 0.4375f, 1.f / -0.5f, 1.f / -0.75f);
}
// rayTriangleCollision's arithmetic in its order, without its division and its EPSILON: u, v and t are compared as
// numerators against the determinant, made positive by an exact negation of all four.  A NaN fails a comparison.
// cross_line: the line through p along d meets the triangle's plane inside the triangle (edges included); det > 0 and
// N, the distance's numerator, go back to the caller, whose rule on N is its own (k_signed's ray, k_collide's segment).
__device__ __forceinline__ bool cross_line(f3 p, f3 d, f3 p0, f3 e1, f3 e2, float& det, float& N) {
    f3 tmp = cross(d, e2);
    det = dot(e1, tmp);
    const f3 rt = sub(p, p0);
    float U = dot(rt, tmp);
    tmp = cross(rt, e1);
    float V = dot(d, tmp);
    N = dot(e2, tmp);
    if (det < 0.f) {
        det = -det;
        U = -U;
        V = -V;
        N = -N;
    }
    return det > 0.f && U >= 0.f && V >= 0.f && U + V <= det;
}
__device__ __forceinline__ bool signed_cross(f3 p, f3 d, f3 p0, f3 e1, f3 e2) {
    float det, N;
    return cross_line(p, d, p0, e1, e2, det, N) && N > 0.f;
}
template <bool COUNT, bool NB, bool NEAR, bool VOTE3>
__global__ __launch_bounds__(BLOCK, BOUNCE_WAVES) void k_signed(SignedArgs a) {
    const uint32_t n = a.n, T = a.T;
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    constexpr uint32_t LAST = VOTE3 ? 2 : 0;
    Counts c = {0, 0, 0, 0, 0};
    uint32_t npoints = 0, ninside = 0;
    bool has = false;
    uint32_t r = 0;
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // (hit, best, bl unused)
    uint32_t j = 0, cnt = 0, flags = 0;            // the ray, its crossings so far, the finished rays' bits
    f3 p = mk(0.f, 0.f, 0.f);
    __shared__ uint32_t s_stk[SB][BLOCK];
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, n, has, [&](uint32_t k) {   // this lane takes the k-th point of the walk order
            r = a.perm ? a.perm[k] : k;
            const float4 pt = a.points[r];
            p = mk(pt.x, pt.y, pt.z);
            if (COUNT) npoints++;
            const bool finite = fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY;
            if (!NEAR) {   // no closest-point pass: no result, and flags = 0 until the last ray ends (or for good:
                           // a point that casts no ray).  With NEAR k_nearest stored the record, flags = 0 included.
                a.out[2 * (size_t)r] = make_float4(0.f, 0.f, 0.f, -1.f);
                a.out[2 * (size_t)r + 1] = make_float4(0.f, 0.f, __uint_as_float(INVALID), 0.f);
            }
            if (finite) {
                has = true;
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
                j = 0;
                cnt = 0;
                flags = 0;
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (!has) continue;
        bool done = false;   // this ray's walk is over
        const bool isleaf = (w.node & LEAF_BIT) != 0;
        // one fetch for every active lane, leaf or node, before the branch (k_nearest)
        v4f q0, q1, q2, q3;
        uint32_t cl = 0, cr = 0;
        if (!NB || isleaf) {
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(a.inner + w.node);
            q0 = rr[0]; q1 = rr[1]; q2 = rr[2]; q3 = rr[3];
            pin(q0); pin(q1); pin(q2); pin(q3);
            if (!NB && !isleaf) {
                const uint32_t own = __float_as_uint(q3.z);
                cl = child_slot(__float_as_uint(q3.x), own, 0);
                cr = child_slot(__float_as_uint(q3.y), own, 1);
            }
        } else {
            const ChildPair ch = nbt.children(w.node);
            cl = ch.cl;
            cr = ch.cr;
            q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
            q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
            q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
            q3 = v4f{0.f, 0.f, 0.f, 0.f};
        }
        const f3 inv = signed_inv(VOTE3 ? j : 0u);
        float mn;
        if (--w.guard == 0) {
            c.overflow++;
            done = true;
        } else if (isleaf) {
            if (COUNT) c.leaf++;
            // (T == 1: the root is the leaf, and no parent tested its box -- words 10..15 of the record)
            if (T > 1 || query_box<true>(p, inv, f2v{q2.z, q2.w}, f2v{q3.y, q3.z}, q3.x, q3.w, false, 0.f, INFINITY, mn))
                cnt += signed_cross(p, signed_dir(VOTE3 ? j : 0u), mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y),
                                    mk(q1.z, q1.w, q2.x));
            walk_pop(w, st);
            done = w.sp == -1;
        } else {
            if (COUNT) c.internal++;
            const bool lh = query_box<true>(p, inv, q0.xy, q0.zw, q2.x, q2.y, false, 0.f, INFINITY, mn);
            const bool rh = query_box<true>(p, inv, q1.xy, q1.zw, q2.z, q2.w, false, 0.f, INFINITY, mn);
            if (!lh && !rh) {
                walk_pop(w, st);
            } else if (lh && rh && w.sp + 1 >= limit) {   // the stack limit: both children lost, counted
                c.overflow++;
                walk_pop(w, st);
            } else {
                if (lh && rh) {   // left first: push the right child
                    st.store(w.sp, w.top);
                    w.sp++;
                    w.top = cr;
                }
                w.node = lh ? cl : cr;
            }
            done = w.sp == -1;
        }
        if (done) {
            flags |= (cnt & 1u) << (j + 1) | (cnt < 255u ? cnt : 255u) << (8 * (j + 1));
            if (j == LAST) {
                const uint32_t odd = flags >> 1 & 7u;
                const uint32_t inside = VOTE3 ? (uint32_t)(__popc(odd) >= 2) : odd & 1u;
                reinterpret_cast<uint32_t*>(a.out + 2 * (size_t)r + 1)[3] = flags | inside;
                if (COUNT) ninside += inside;
                has = false;
            } else {   // the next ray, from the root
                j++;
                cnt = 0;
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
            }
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[5] = {npoints, ninside, c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int k = 0; k < 4; k++) atomicAdd(&a.counts[k], v[k]);
            if (v[4]) atomicAdd(a.overflow, v[4]);
        }
    }
}

// ---- self-collision queries (rtbvh_collide_async): the crossing pairs of the mesh's own triangles ---------------
// k_overlap's frame and CSR protocol with the tree's own leaves for queries: the lane that claims k takes the leaf at
// sorted position k -- its box is the query box, the claims come in sort order, which is the coherent order -- and
// lists the leaves it is paired with under include/rtbvh.h's rules: the position filter (partner position > k: a
// pair is listed by its earlier triangle; SYM: != k, by both), (B) on the two leaf boxes, (N) no common vertex
// index -- one gather of the partner's three indices, only behind (B) -- and, under TRI, (X): one of the six
// segment-triangle tests holds, cross_line's arithmetic with both ends of the segment checked.  The node test is
// k_overlap's (B), so the walk reaches every member, left first: a list is in sort order.
// The half a triangle does not own is pruned by leaf range (!SYM).  Karras node i splits its range [lo, hi] at g:
// its left child is node or leaf g over [lo, g], its right one g + 1 over [g + 1, hi].  So the left child's range
// ends at its own id, which the step holds in either tree form, and it is skipped iff g <= k; the right child's
// range ends where its parent's does, past k by induction from the root's T - 1 (position T - 1 owns nothing and
// is not walked).  No fetch is added, and the lists are the same with and without: a skipped subtree holds
// positions <= k only, all of which the position filter drops.
__device__ __forceinline__ bool segment_cross(f3 p, f3 d, f3 p0, f3 e1, f3 e2) {
    float det, N;
    return cross_line(p, d, p0, e1, e2, det, N) && N >= 0.f && N <= det;
}
// the segments S0 = (a, e1), S1 = (a, e2), S2 = (fl(a + e1), fl(e2 - e1)) of one triangle against the other
__device__ __forceinline__ bool edges_cross(f3 a, f3 e1, f3 e2, f3 p0, f3 f1, f3 f2) {
    return segment_cross(a, e1, p0, f1, f2) || segment_cross(a, e2, p0, f1, f2) ||
           segment_cross(add(a, e1), sub(e2, e1), p0, f1, f2);
}
// Every instance fits 64 registers without a spill at 8 waves per SIMD, the TRI ones too: the six tests run one
// after the other on the 16 floats of the query and the 9 of the partner (DESIGN.md 5k has each instance's count).
template <bool FILL, bool COUNT, bool NB, bool TRI, bool SYM>
__global__ __launch_bounds__(BLOCK, BOUNCE_WAVES) void k_collide(CollideArgs a) {
    const uint32_t T = a.T;
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const uint32_t* __restrict__ idx = a.idx;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    Counts c = {0, 0, 0, 0, 0};
    uint32_t ntris = 0;
    unsigned long long nids = 0;
    bool has = false;
    uint32_t k = 0, id = 0, cnt = 0;          // the query leaf's position and triangle, its partners so far
    uint32_t i0 = 0, i1 = 0, i2 = 0;          // its vertex indices
    unsigned long long pos = 0, end = 0;      // FILL: the next id's index and the end of the triangle's segment
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // (hit, best, bl unused)
    f3 qlo = mk(0.f, 0.f, 0.f), qhi = mk(0.f, 0.f, 0.f);
    f3 qa = mk(0.f, 0.f, 0.f), qe1 = mk(0.f, 0.f, 0.f), qe2 = mk(0.f, 0.f, 0.f);
    __shared__ uint32_t s_stk[SB][BLOCK];
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, T, has, [&](uint32_t p) {   // this lane takes the leaf at sorted position p
            k = p;
            const float4* r = leaf + 4 * (size_t)p;
            const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
            id = __float_as_uint(r2.y) & ~LEAF_BIT;
            qlo = mk(r2.z, r2.w, r3.x);
            qhi = mk(r3.y, r3.z, r3.w);
            if (TRI) {
                qa = mk(r0.x, r0.y, r0.z);
                qe1 = mk(r0.w, r1.x, r1.y);
                qe2 = mk(r1.z, r1.w, r2.x);
            }
            if (COUNT && a.count_ids) ntris++;
            // no walk: a NaN in the leaf box fails (B) with every box; the last position owns no pair
            if (!(qlo.x <= qhi.x && qlo.y <= qhi.y && qlo.z <= qhi.z) || (!SYM && p + 1 == T)) {
                if (!FILL) a.offsets[(size_t)id + 1] = 0;
            } else {
                has = true;
                i0 = idx[3 * (size_t)id];
                i1 = idx[3 * (size_t)id + 1];
                i2 = idx[3 * (size_t)id + 2];
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
                cnt = 0;
                if (FILL) {
                    pos = a.offsets[id];
                    const unsigned long long e = a.offsets[(size_t)id + 1];
                    end = e < a.capacity ? e : a.capacity;
                }
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (!has) continue;
        bool done = false;
        const bool isleaf = (w.node & LEAF_BIT) != 0;
        // one fetch for every active lane, leaf or node, before the branch (k_nearest)
        v4f q0, q1, q2, q3;
        uint32_t cl = 0, cr = 0, gl = 0;   // gl: the left child's Karras id, where its leaf range ends
        if (!NB || isleaf) {
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(a.inner + w.node);
            q0 = rr[0]; q1 = rr[1]; q2 = rr[2]; q3 = rr[3];
            if (!NB && !isleaf) {
                const uint32_t own = __float_as_uint(q3.z);
                gl = __float_as_uint(q3.x) & ~LEAF_BIT;
                cl = child_slot(__float_as_uint(q3.x), own, 0);
                cr = child_slot(__float_as_uint(q3.y), own, 1);
            }
        } else {
            const ChildPair ch = nbt.children(w.node);
            cl = ch.cl;
            cr = ch.cr;
            gl = ch.cl & ~LEAF_BIT;
            q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
            q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
            q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
            q3 = v4f{0.f, 0.f, 0.f, 0.f};
        }
        if (--w.guard == 0) {
            c.overflow++;
            done = true;
        } else if (isleaf) {
            if (COUNT) c.leaf++;
            const uint32_t j = w.node & ~LEAF_BIT;
            const uint32_t y = __float_as_uint(q2.y) & ~LEAF_BIT;
            bool in = (SYM ? j != k : j > k) && boxes_meet(qlo, qhi, mk(q2.z, q2.w, q3.x), mk(q3.y, q3.z, q3.w));
            if (in) {   // (N): the partner's three indices
                const uint32_t y0 = idx[3 * (size_t)y], y1 = idx[3 * (size_t)y + 1], y2 = idx[3 * (size_t)y + 2];
                in = i0 != y0 && i0 != y1 && i0 != y2 && i1 != y0 && i1 != y1 && i1 != y2 && i2 != y0 && i2 != y1 &&
                     i2 != y2;
            }
            if (TRI && in) {
                const f3 p0 = mk(q0.x, q0.y, q0.z), f1 = mk(q0.w, q1.x, q1.y), f2 = mk(q1.z, q1.w, q2.x);
                in = edges_cross(qa, qe1, qe2, p0, f1, f2) || edges_cross(p0, f1, f2, qa, qe1, qe2);
            }
            if (in) {
                if (!FILL || COUNT) cnt++;
                if (FILL && pos < end) {
                    a.ids[pos] = y;
                    pos++;
                }
            }
            walk_pop(w, st);
            done = w.sp == -1;
        } else {
            if (COUNT) c.internal++;
            const bool lh = (SYM || gl > k) && boxes_meet(qlo, qhi, mk(q0.x, q0.y, q2.x), mk(q0.z, q0.w, q2.y));
            const bool rh = boxes_meet(qlo, qhi, mk(q1.x, q1.y, q2.z), mk(q1.z, q1.w, q2.w));
            if (!lh && !rh) {
                walk_pop(w, st);
            } else if (lh && rh && w.sp + 1 >= limit) {   // the stack limit: both children lost, counted
                c.overflow++;
                walk_pop(w, st);
            } else {
                if (lh && rh) {   // left first: push the right child
                    st.store(w.sp, w.top);
                    w.sp++;
                    w.top = cr;
                }
                w.node = lh ? cl : cr;
            }
            done = w.sp == -1;
        }
        if (done) {
            if (!FILL) a.offsets[(size_t)id + 1] = cnt;
            if (COUNT && a.count_ids) nids += cnt;
            has = false;
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[5] = {ntris, nids, c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int i = 0; i < 4; i++) atomicAdd(&a.counts[i], v[i]);
            if (v[4]) atomicAdd(a.overflow, v[4]);
        }
    }
}

// ---- triangle queries (rtbvh_cross_async, rtbvh_cross_first_async): what a caller's triangle crosses -------------
// k_overlap's frame and CSR protocol with a caller's triangle for the query: the claiming lane loads its three 16-B
// words and keeps what a leaf record would hold of it -- a, e1 = v1 - v0, e2 = v2 - v0 and the box [qlo, qhi] of the
// three vertices, 15 floats -- and lists the leaves that pass include/rtbvh.h's rules: (B) on the leaf's own box,
// then (X), k_collide's six segment-triangle tests through edges_cross.  The node test is k_overlap's (B), so the
// walk reaches every member, left first: a list is in sort order.
// PASS: CROSS_PASS_SIZES and CROSS_PASS_FILL are k_overlap's two passes.  CROSS_PASS_FIRST stores the first member
// met at first[r] and ends the walk there -- left first, that is the member at the lowest sort position, the head of
// the list -- and 0xFFFFFFFF when the walk ends without one.
// The four record loads are not pinned (k_collide's choice, not k_overlap's): every instance fits 64 registers
// without a spill at 8 waves per SIMD as it is, and pinned each of the twelve took the same registers (DESIGN.md 5l
// has each instance's count).
template <int PASS, bool COUNT, bool NB>
__global__ __launch_bounds__(BLOCK, BOUNCE_WAVES) void k_cross(CrossArgs a) {
    constexpr bool SIZES = PASS == CROSS_PASS_SIZES, FILL = PASS == CROSS_PASS_FILL, FIRST = PASS == CROSS_PASS_FIRST;
    const uint32_t n = a.n, T = a.T;
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    Counts c = {0, 0, 0, 0, 0};
    uint32_t nqueries = 0;
    unsigned long long nids = 0;
    bool has = false;
    uint32_t r = 0, cnt = 0;
    unsigned long long pos = 0, end = 0;   // FILL: the next id's index and the end of the query's segment
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // (hit, best, bl unused)
    f3 qlo = mk(0.f, 0.f, 0.f), qhi = mk(0.f, 0.f, 0.f);
    f3 qa = mk(0.f, 0.f, 0.f), qe1 = mk(0.f, 0.f, 0.f), qe2 = mk(0.f, 0.f, 0.f);
    __shared__ uint32_t s_stk[SB][BLOCK];
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, n, has, [&](uint32_t k) {   // this lane takes the k-th triangle of the walk order
            r = a.perm ? a.perm[k] : k;
            const float4 t0 = a.tris[3 * (size_t)r], t1 = a.tris[3 * (size_t)r + 1], t2 = a.tris[3 * (size_t)r + 2];
            const f3 v0 = mk(t0.x, t0.y, t0.z), v1 = mk(t1.x, t1.y, t1.z), v2 = mk(t2.x, t2.y, t2.z);
            if (COUNT && a.count_ids) nqueries++;
            const bool finite = fabsf(v0.x) < INFINITY && fabsf(v0.y) < INFINITY && fabsf(v0.z) < INFINITY &&
                                fabsf(v1.x) < INFINITY && fabsf(v1.y) < INFINITY && fabsf(v1.z) < INFINITY &&
                                fabsf(v2.x) < INFINITY && fabsf(v2.y) < INFINITY && fabsf(v2.z) < INFINITY;
            if (!finite) {   // no walk: an empty list
                if (SIZES) a.offsets[(size_t)r + 1] = 0;
                if (FIRST) a.first[r] = INVALID;
            } else {
                has = true;
                qa = v0;
                qe1 = sub(v1, v0);
                qe2 = sub(v2, v0);
                qlo = mk(fminf(fminf(v0.x, v1.x), v2.x), fminf(fminf(v0.y, v1.y), v2.y), fminf(fminf(v0.z, v1.z), v2.z));
                qhi = mk(fmaxf(fmaxf(v0.x, v1.x), v2.x), fmaxf(fmaxf(v0.y, v1.y), v2.y), fmaxf(fmaxf(v0.z, v1.z), v2.z));
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
                cnt = 0;
                if (FILL) {
                    pos = a.offsets[r];
                    const unsigned long long e = a.offsets[(size_t)r + 1];
                    end = e < a.capacity ? e : a.capacity;
                }
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (!has) continue;
        bool done = false;
        const bool isleaf = (w.node & LEAF_BIT) != 0;
        // one fetch for every active lane, leaf or node, before the branch (k_nearest)
        v4f q0, q1, q2, q3;
        uint32_t cl = 0, cr = 0;
        if (!NB || isleaf) {
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(a.inner + w.node);
            q0 = rr[0]; q1 = rr[1]; q2 = rr[2]; q3 = rr[3];
            if (!NB && !isleaf) {
                const uint32_t own = __float_as_uint(q3.z);
                cl = child_slot(__float_as_uint(q3.x), own, 0);
                cr = child_slot(__float_as_uint(q3.y), own, 1);
            }
        } else {
            const ChildPair ch = nbt.children(w.node);
            cl = ch.cl;
            cr = ch.cr;
            q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
            q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
            q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
            q3 = v4f{0.f, 0.f, 0.f, 0.f};
        }
        if (--w.guard == 0) {
            c.overflow++;
            done = true;
        } else if (isleaf) {
            if (COUNT) c.leaf++;
            bool in = boxes_meet(qlo, qhi, mk(q2.z, q2.w, q3.x), mk(q3.y, q3.z, q3.w));   // the leaf's own box first
            if (in) {
                const f3 p0 = mk(q0.x, q0.y, q0.z), f1 = mk(q0.w, q1.x, q1.y), f2 = mk(q1.z, q1.w, q2.x);
                in = edges_cross(qa, qe1, qe2, p0, f1, f2) || edges_cross(p0, f1, f2, qa, qe1, qe2);
            }
            if (in) {
                if (!FILL || COUNT) cnt++;
                if (FILL && pos < end) {
                    a.ids[pos] = __float_as_uint(q2.y) & ~LEAF_BIT;
                    pos++;
                }
                if (FIRST) a.first[r] = __float_as_uint(q2.y) & ~LEAF_BIT;
            }
            if (FIRST && in) {   // the head of the list: the walk ends here
                done = true;
            } else {
                walk_pop(w, st);
                done = w.sp == -1;
            }
        } else {
            if (COUNT) c.internal++;
            const bool lh = boxes_meet(qlo, qhi, mk(q0.x, q0.y, q2.x), mk(q0.z, q0.w, q2.y));
            const bool rh = boxes_meet(qlo, qhi, mk(q1.x, q1.y, q2.z), mk(q1.z, q1.w, q2.w));
            if (!lh && !rh) {
                walk_pop(w, st);
            } else if (lh && rh && w.sp + 1 >= limit) {   // the stack limit: both children lost, counted
                c.overflow++;
                walk_pop(w, st);
            } else {
                if (lh && rh) {   // left first: push the right child
                    st.store(w.sp, w.top);
                    w.sp++;
                    w.top = cr;
                }
                w.node = lh ? cl : cr;
            }
            done = w.sp == -1;
        }
        if (done) {
            if (SIZES) a.offsets[(size_t)r + 1] = cnt;
            if (FIRST && cnt == 0) a.first[r] = INVALID;
            if (COUNT && a.count_ids) nids += cnt;
            has = false;
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[5] = {nqueries, nids, c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int k = 0; k < 4; k++) atomicAdd(&a.counts[k], v[k]);
            if (v[4]) atomicAdd(a.overflow, v[4]);
        }
    }
}

// RTBVH_CROSS_SORT's key: the 30-bit Morton code, in the root box, of the centre of the query triangle's box
// (k_overlap_keys' code)
__global__ __launch_bounds__(BLOCK) void k_cross_keys(const float4* __restrict__ tris, uint32_t n,
                                                      const float* __restrict__ box, uint32_t* __restrict__ keys,
                                                      uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 v0 = tris[3 * (size_t)i], v1 = tris[3 * (size_t)i + 1], v2 = tris[3 * (size_t)i + 2];
    const f3 lo = mk(fminf(fminf(v0.x, v1.x), v2.x), fminf(fminf(v0.y, v1.y), v2.y), fminf(fminf(v0.z, v1.z), v2.z));
    const f3 hi = mk(fmaxf(fmaxf(v0.x, v1.x), v2.x), fmaxf(fmaxf(v0.y, v1.y), v2.y), fmaxf(fmaxf(v0.z, v1.z), v2.z));
    keys[i] = spread9(q9((lo.x + hi.x) * 0.5f, box[0], box[3])) << 2 |
              spread9(q9((lo.y + hi.y) * 0.5f, box[1], box[4])) << 1 | spread9(q9((lo.z + hi.z) * 0.5f, box[2], box[5]));
    vals[i] = i;
}

// ---- clearance queries (rtbvh_clearance_async): the nearest scene triangle to a caller's triangle ----------------
// For each query triangle the lexicographic minimum of (dist2, triangle id) over the scene triangles with dist2 <=
// max_dist2.  include/rtbvh.h has the formulas: the first smallest of fifteen candidate point pairs -- each vertex
// of one triangle against the other triangle through triangle_dist2, unchanged, and the nine segment pairs -- every
// point clamped into its own triangle's box, and +0 where k_cross's (B) and (X) hold.  DESIGN.md 5n has why the walk
// returns the brute-force answer bit for bit: with both points clamped, a pair's dist2 is never below the box-box
// distance of the query's box and any box that contains the leaf box, so a walk that enters a box iff that distance
// is <= the bound (non-strict: ties are visited for the id tie-break) reaches every triangle that can win.
// k_nearest's frame -- the claims, the stack, one 64-B fetch a step before the leaf / node branch, the guard and the
// run-time stack limit, the u64 best key, the winner's points recomputed at the end from its leaf record -- with
// k_cross's query load.  Plain fp32 as specified: no fma, no fast intrinsics, every division the IEEE quotient.
// The fifteen candidates run as one loop that is not unrolled, so one candidate's intermediates are live at a time;
// CLEARANCE_WAVES is chosen from the instances' register counts.
#ifndef RTBVH_CLEARANCE_WAVES   // (an A/B build sets another launch bound: EXTRA=-DRTBVH_CLEARANCE_WAVES=<n>)
#define RTBVH_CLEARANCE_WAVES 5
#endif
constexpr uint32_t CLEARANCE_WAVES = RTBVH_CLEARANCE_WAVES;
__device__ __forceinline__ f3 sel(bool s, f3 x, f3 y) { return mk(s ? x.x : y.x, s ? x.y : y.y, s ? x.z : y.z); }
__device__ __forceinline__ f3 clamp_box(f3 lo, f3 hi, f3 p) {
    return mk(fmaxf(lo.x, fminf(hi.x, p.x)), fmaxf(lo.y, fminf(hi.y, p.y)), fmaxf(lo.z, fminf(hi.z, p.z)));
}
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }   // a NaN becomes 0
__device__ __forceinline__ float box_box_dist2(f3 qlo, f3 qhi, f3 lo, f3 hi) {
    const float dx = fmaxf(fmaxf(lo.x - qhi.x, qlo.x - hi.x), 0.f);
    const float dy = fmaxf(fmaxf(lo.y - qhi.y, qlo.y - hi.y), 0.f);
    const float dz = fmaxf(fmaxf(lo.z - qhi.z, qlo.z - hi.z), 0.f);
    return (dx * dx + dy * dy) + dz * dz;
}
// the closest points of the segments (P1, D1) and (P2, D2), before the box clamps
__device__ __forceinline__ void segment_pair(f3 P1, f3 D1, f3 P2, f3 D2, f3& c1, f3& c2) {
    const f3 r = sub(P1, P2);
    const float A = dot(D1, D1), E = dot(D2, D2), F = dot(D2, r), C = dot(D1, r), B = dot(D1, D2);
    const float den = A * E - B * B;
    float s = den > 0.f ? clamp01((B * F - C * E) / den) : 0.f;
    float t = (B * s + F) / E;
    if (t < 0.f) s = clamp01(-C / A);
    else if (t > 1.f) s = clamp01((B - C) / A);
    t = clamp01(t);
    c1 = add(P1, mul(D1, s));
    c2 = add(P2, mul(D2, t));
}
// candidate k of the header's fifteen for the query (qa, qe1, qe2, [qlo, qhi]) and the scene triangle
// (a, e1, e2, [lo, hi]): its two points, clamped, and their squared distance.  k is the same in every lane.
__device__ __forceinline__ float clearance_candidate(int k, f3 qa, f3 qe1, f3 qe2, f3 qlo, f3 qhi, f3 a, f3 e1, f3 e2,
                                                     f3 lo, f3 hi, f3& cq, f3& cx) {
    if (k < 6) {   // a vertex of one triangle (o) against the other (t): 0..2 the query's vertices, 3..5 the scene's
        const bool s = k >= 3;
        const int i = s ? k - 3 : k;
        const f3 oa = sel(s, a, qa), oe = sel(s, i == 1 ? e1 : e2, i == 1 ? qe1 : qe2);
        const f3 V = i == 0 ? oa : add(oa, oe);
        float u, v;
        f3 c;
        triangle_dist2(V, sel(s, qa, a), sel(s, qe1, e1), sel(s, qe2, e2), sel(s, qlo, lo), sel(s, qhi, hi), u, v, c);
        cq = sel(s, c, V);
        cx = sel(s, V, c);
    } else {       // segment i of the query against segment j of the scene triangle, i major
        const int i = (k - 6) / 3, j = (k - 6) - 3 * i;
        const f3 P1 = i == 2 ? add(qa, qe1) : qa, D1 = i == 0 ? qe1 : i == 1 ? qe2 : sub(qe2, qe1);
        const f3 P2 = j == 2 ? add(a, e1) : a, D2 = j == 0 ? e1 : j == 1 ? e2 : sub(e2, e1);
        segment_pair(P1, D1, P2, D2, cq, cx);
    }
    cq = clamp_box(qlo, qhi, cq);
    cx = clamp_box(lo, hi, cx);
    const f3 e = sub(cq, cx);
    return dot(e, e);
}
// the pair's distance without the override: the first candidate with the smallest d (a NaN never wins), its points
__device__ __forceinline__ float clearance_pair(f3 qa, f3 qe1, f3 qe2, f3 qlo, f3 qhi, f3 a, f3 e1, f3 e2, f3 lo, f3 hi,
                                                f3& bq, f3& bx) {
    float best = __uint_as_float(0x7FC00000u);
#pragma unroll 1
    for (int k = 0; k < 15; k++) {
        f3 cq, cx;
        const float d = clearance_candidate(k, qa, qe1, qe2, qlo, qhi, a, e1, e2, lo, hi, cq, cx);
        if (d < best || best != best) {
            best = d;
            bq = cq;
            bx = cx;
        }
    }
    return best;
}
template <bool COUNT, bool NB>
__global__ __launch_bounds__(BLOCK, CLEARANCE_WAVES) void k_clearance(ClearanceArgs a) {
    const uint32_t n = a.n, T = a.T;
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    Counts c = {0, 0, 0, 0, 0};
    uint32_t nqueries = 0, nfound = 0;
    bool has = false;
    uint32_t r = 0;
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // (bl: the best triangle's sorted leaf index; hit, best unused)
    uint64_t key = 0;
    f3 qlo = mk(0.f, 0.f, 0.f), qhi = mk(0.f, 0.f, 0.f);
    f3 qa = mk(0.f, 0.f, 0.f), qe1 = mk(0.f, 0.f, 0.f), qe2 = mk(0.f, 0.f, 0.f);
    __shared__ uint32_t s_stk[SB][BLOCK];
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    const float4 none0 = make_float4(0.f, 0.f, 0.f, -1.f), none1 = make_float4(0.f, 0.f, 0.f, __uint_as_float(INVALID));
    const float bound0 = a.max_dist2 + 0.f;   // (-0 -> +0: the key's bits order as the floats)
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, n, has, [&](uint32_t k) {   // this lane takes the k-th triangle of the walk order
            r = a.perm ? a.perm[k] : k;
            const float4 t0 = a.tris[3 * (size_t)r], t1 = a.tris[3 * (size_t)r + 1], t2 = a.tris[3 * (size_t)r + 2];
            const f3 v0 = mk(t0.x, t0.y, t0.z), v1 = mk(t1.x, t1.y, t1.z), v2 = mk(t2.x, t2.y, t2.z);
            if (COUNT) nqueries++;
            const bool finite = fabsf(v0.x) < INFINITY && fabsf(v0.y) < INFINITY && fabsf(v0.z) < INFINITY &&
                                fabsf(v1.x) < INFINITY && fabsf(v1.y) < INFINITY && fabsf(v1.z) < INFINITY &&
                                fabsf(v2.x) < INFINITY && fabsf(v2.y) < INFINITY && fabsf(v2.z) < INFINITY;
            if (!(bound0 >= 0.f) || !finite) {   // no walk: no result
                a.out[2 * (size_t)r] = none0;
                a.out[2 * (size_t)r + 1] = none1;
            } else {
                has = true;
                qa = v0;
                qe1 = sub(v1, v0);
                qe2 = sub(v2, v0);
                qlo = mk(fminf(fminf(v0.x, v1.x), v2.x), fminf(fminf(v0.y, v1.y), v2.y), fminf(fminf(v0.z, v1.z), v2.z));
                qhi = mk(fmaxf(fmaxf(v0.x, v1.x), v2.x), fmaxf(fmaxf(v0.y, v1.y), v2.y), fmaxf(fmaxf(v0.z, v1.z), v2.z));
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
                key = (uint64_t)__float_as_uint(bound0) << 32 | 0xFFFFFFFFull;
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (!has) continue;
        bool done = false;
        const bool isleaf = (w.node & LEAF_BIT) != 0;
        // one fetch for every active lane, leaf or node, before the branch (k_nearest)
        v4f q0, q1, q2, q3;
        uint32_t cl = 0, cr = 0;
        if (!NB || isleaf) {
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(a.inner + w.node);
            q0 = rr[0]; q1 = rr[1]; q2 = rr[2]; q3 = rr[3];
            if (!NB && !isleaf) {
                const uint32_t own = __float_as_uint(q3.z);
                cl = child_slot(__float_as_uint(q3.x), own, 0);
                cr = child_slot(__float_as_uint(q3.y), own, 1);
            }
        } else {
            const ChildPair ch = nbt.children(w.node);
            cl = ch.cl;
            cr = ch.cr;
            q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
            q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
            q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
            q3 = v4f{0.f, 0.f, 0.f, 0.f};
        }
        const float bound = key_t(key);
        if (--w.guard == 0) {
            c.overflow++;
            done = true;
        } else if (isleaf) {
            if (COUNT) c.leaf++;
            // the leaf's own box first (words 10..15): a pair's dist2 is never below its box-box distance
            const f3 lo = mk(q2.z, q2.w, q3.x), hi = mk(q3.y, q3.z, q3.w);
            if (box_box_dist2(qlo, qhi, lo, hi) <= bound) {
                const f3 p0 = mk(q0.x, q0.y, q0.z), f1 = mk(q0.w, q1.x, q1.y), f2 = mk(q1.z, q1.w, q2.x);
                float d = 0.f;   // (B) and (X): the triangles cross
                if (!(boxes_meet(qlo, qhi, lo, hi) &&
                      (edges_cross(qa, qe1, qe2, p0, f1, f2) || edges_cross(p0, f1, f2, qa, qe1, qe2)))) {
                    f3 bq, bx;
                    d = clearance_pair(qa, qe1, qe2, qlo, qhi, p0, f1, f2, lo, hi, bq, bx);
                }
                const uint64_t cand = (uint64_t)__float_as_uint(d) << 32 | (__float_as_uint(q2.y) & ~LEAF_BIT);
                if (cand < key) {
                    key = cand;
                    w.bl = w.node & ~LEAF_BIT;
                }
            }
            walk_pop(w, st);
            done = w.sp == -1;
        } else {
            if (COUNT) c.internal++;
            const float bdl = box_box_dist2(qlo, qhi, mk(q0.x, q0.y, q2.x), mk(q0.z, q0.w, q2.y));
            const float bdr = box_box_dist2(qlo, qhi, mk(q1.x, q1.y, q2.z), mk(q1.z, q1.w, q2.w));
            const bool lh = bdl <= bound, rh = bdr <= bound;
            if (!lh && !rh) {
                walk_pop(w, st);
            } else if (lh && rh && w.sp + 1 >= limit) {   // the stack limit: both children lost, counted
                c.overflow++;
                walk_pop(w, st);
            } else {
                const bool swap = lh && rh && bdr < bdl;   // the nearer child first
                if (lh && rh) {
                    st.store(w.sp, w.top);   // push the other
                    w.sp++;
                    w.top = swap ? cl : cr;
                }
                w.node = swap ? cr : (lh ? cl : cr);
            }
            done = w.sp == -1;
        }
        if (done) {
            float4 o0 = none0, o1 = none1;
            if ((uint32_t)key != 0xFFFFFFFFu) {   // the winner's points, recomputed from its leaf record
                const float4* lr = leaf + 4 * (size_t)w.bl;
                const float4 la = lr[0], lb = lr[1], lc = lr[2], ld = lr[3];
                f3 bq = mk(0.f, 0.f, 0.f), bx = mk(0.f, 0.f, 0.f);
                clearance_pair(qa, qe1, qe2, qlo, qhi, mk(la.x, la.y, la.z), mk(la.w, lb.x, lb.y), mk(lb.z, lb.w, lc.x),
                               mk(lc.z, lc.w, ld.x), mk(ld.y, ld.z, ld.w), bq, bx);
                o0 = make_float4(bq.x, bq.y, bq.z, key_t(key));   // (dist2: +0 where the pair crosses)
                o1 = make_float4(bx.x, bx.y, bx.z, __uint_as_float((uint32_t)key));
            }
            a.out[2 * (size_t)r] = o0;
            a.out[2 * (size_t)r + 1] = o1;
            has = false;
            if (COUNT) nfound += (uint32_t)key != 0xFFFFFFFFu;
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[5] = {nqueries, nfound, c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int k = 0; k < 4; k++) atomicAdd(&a.counts[k], v[k]);
            if (v[4]) atomicAdd(a.overflow, v[4]);
        }
    }
}

// ---- sphere-sweep queries (rtbvh_sweep_async): the first contact of a moving sphere --------------------------
// For each sweep (c, d, r, t_max) the member with the smallest (tk bits, triangle id), tk = fmaxf(t, mn) + 0 with mn
// the slab entry of the member's own leaf box grown by r: k_khits at k = 1 with another leaf test and every box grown
// by r.  include/rtbvh.h has the formulas -- the start overlap through triangle_dist2, unchanged, then the first
// smallest of seven candidates (face, three edge segments, three vertices) -- and DESIGN.md 5q why the walk returns
// the brute-force answer bit for bit: growing rounds monotonically, so the grown boxes nest as the boxes do, no
// grown box around a member's leaf box starts above its tk, and a box is entered iff it passes the first two slab
// conditions and !(mn > bound), bound = t_max until a member is found, then the best tk -- a leaf's own box by (B)
// itself, a child's box by (B) without the axes of an infinite 1 / d (the node branch below has why).
// k_khits' frame without the LDS list: the best key, its leaf slot (w.bl), its feature and its genuine t live in
// registers; the winner's point is recomputed at the end from its leaf record by the same functions on the same
// inputs (the edge candidates' s_/ee and the walk's point clamps are then never computed in the walk).
// Plain fp32 as specified: no fma, no fast intrinsics, every `/` and sqrtf the IEEE result.  The seven candidates run
// as one loop that is not unrolled, so one candidate's intermediates are live at a time; SWEEP_WAVES is chosen from
// the instances' register counts.
#ifndef RTBVH_SWEEP_WAVES   // (an A/B build sets another launch bound: EXTRA=-DRTBVH_SWEEP_WAVES=<n>)
#define RTBVH_SWEEP_WAVES 6
#endif
constexpr uint32_t SWEEP_WAVES = RTBVH_SWEEP_WAVES;
// Candidate k of the header's list (0 the face, 1..3 the segments S0..S2, 4..6 the vertices V0..V2): its t, or a
// NaN where one of its "needs" fails; POINT: its point as well, before the clamp.
template <bool POINT>
__device__ __forceinline__ float sweep_candidate(int k, f3 c, f3 d, float dd, float r, f3 a, f3 e1, f3 e2, f3& pt) {
    const float none = __uint_as_float(0x7FC00000u);
    if (k == 0) {
        f3 n = cross(e1, e2);
        const float nn = dot(n, n);
        if (!(nn > 0.f)) return none;
        float s = dot(n, sub(c, a));
        if (s < 0.f) {
            n = mk(-n.x, -n.y, -n.z);
            s = -s;
        }
        const float ln = sqrtf(nn), h = s - r * ln, dn = dot(n, d);
        if (!(dn < 0.f && h >= 0.f)) return none;
        const float t = h / (-dn);
        const f3 p = sub(add(c, mul(d, t)), mul(n, r / ln)), ap = sub(p, a);
        const float d1 = dot(e1, ap), d2 = dot(e2, ap);
        const float e11 = dot(e1, e1), e12 = dot(e1, e2), e22 = dot(e2, e2);
        const float den = e11 * e22 - e12 * e12;
        const float u = (e22 * d1 - e12 * d2) / den, v = (e11 * d2 - e12 * d1) / den;
        if (!(u >= 0.f && v >= 0.f && u + v <= 1.f)) return none;
        if (POINT) pt = p;
        return t;
    }
    const f3 v1 = add(a, e1);
    if (k <= 3) {
        const f3 A = k == 3 ? v1 : a, E = k == 1 ? e1 : k == 2 ? e2 : sub(e2, e1);
        const f3 m = sub(c, A);
        const float ee = dot(E, E), md = dot(m, E), nd = dot(d, E), mm = dot(m, m), mdd = dot(m, d);
        const float a_ = ee * dd - nd * nd, k_ = mm - r * r, c_ = ee * k_ - md * md, b_ = ee * mdd - nd * md;
        if (!(a_ > 0.f && c_ > 0.f && b_ < 0.f)) return none;
        const float disc = b_ * b_ - a_ * c_;
        if (!(disc >= 0.f)) return none;
        const float t = c_ / (sqrtf(disc) - b_);   // the root without cancellation
        const float s_ = md + t * nd;
        if (!(0.f <= s_ && s_ <= ee)) return none;
        if (POINT) pt = add(A, mul(E, s_ / ee));
        return t;
    }
    const f3 V = k == 4 ? a : k == 5 ? v1 : add(a, e2);
    const f3 m = sub(c, V);
    const float b = dot(m, d), cc = dot(m, m) - r * r;
    if (!(cc > 0.f && b < 0.f)) return none;
    const float disc = b * b - dd * cc;
    if (!(disc >= 0.f)) return none;
    if (POINT) pt = V;
    return cc / (sqrtf(disc) - b);
}
// (T) of the pair: the feature (0: no t) and the t
__device__ __forceinline__ uint32_t sweep_pair(f3 c, f3 d, float r, float tmax, f3 a, f3 e1, f3 e2, f3 lo, f3 hi,
                                               float& t) {
    float u, v;
    f3 q;
    t = 0.f;
    if (triangle_dist2(c, a, e1, e2, lo, hi, u, v, q) <= r * r) return 1u;   // the start overlap
    const float dd = dot(d, d);
    uint32_t feature = 0;
#pragma unroll 1
    for (int k = 0; k < 7; k++) {
        const float tc = sweep_candidate<false>(k, c, d, dd, r, a, e1, e2, q);
        if (0.f <= tc && tc <= tmax && (feature == 0 || tc < t)) {   // the first smallest
            t = tc;
            feature = 2u + (uint32_t)k;
        }
    }
    return feature;
}
template <bool ANY, bool COUNT, bool NB>
__global__ __launch_bounds__(BLOCK, SWEEP_WAVES) void k_sweep(SweepArgs a) {
    const uint32_t n = a.n, T = a.T;
    const uint32_t lane = lane_id();
    const int limit = a.stack_limit;
    const float4* __restrict__ leaf = a.leaf;
    const RecordTree rec{a.inner};
    const NodeBoxTree nbt{a.topo, a.nbox, leaf};
    Counts c = {0, 0, 0, 0, 0};
    uint32_t nsweeps = 0, nhits = 0;
    bool has = false;
    uint32_t r = 0;
    Walk w{0u, INVALID, 0, false, 0.f, 0u, 0u};   // (bl: the best member's sorted leaf index; hit, best unused)
    uint64_t key = 0;
    uint32_t feature = 0;   // the best member's, and its genuine t
    float bt = 0.f;
    float tmax = 0.f, rad = 0.f;
    f3 o = mk(0.f, 0.f, 0.f), d = o, inv = o;
    __shared__ uint32_t s_stk[SB][BLOCK];
    uint32_t stack[STACK_SIZE - SB];   // entries [SB, STACK_SIZE)
    BlockStack st{&s_stk[0][threadIdx.x], stack};
    const float4 none0 = make_float4(-1.f, 0.f, 0.f, 0.f), none1 = make_float4(__uint_as_float(INVALID), 0.f, 0.f, 0.f);
    Refill rf;
    while (true) {
        refill_claim(rf, a.next, n, has, [&](uint32_t p) {   // this lane takes the p-th sweep of the walk order
            r = a.perm ? a.perm[p] : p;
            const float4 q0 = a.sweeps[2 * (size_t)r], q1 = a.sweeps[2 * (size_t)r + 1];
            o = mk(q0.x, q0.y, q0.z);
            tmax = q0.w + 0.f;   // (-0 -> +0: the key's bits order as the floats)
            d = mk(q1.x, q1.y, q1.z);
            rad = q1.w + 0.f;
            inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
            if (COUNT) nsweeps++;
            const bool finite = fabsf(o.x) < INFINITY && fabsf(o.y) < INFINITY && fabsf(o.z) < INFINITY &&
                                fabsf(d.x) < INFINITY && fabsf(d.y) < INFINITY && fabsf(d.z) < INFINITY;
            const bool zero = d.x == 0.f && d.y == 0.f && d.z == 0.f;
            if (!finite || zero || !(rad >= 0.f) || !(rad < INFINITY) || !(tmax >= 0.f)) {   // no walk: a miss
                a.hits[2 * (size_t)r] = none0;
                a.hits[2 * (size_t)r + 1] = none1;
            } else {
                has = true;
                w = walk_start(NB ? nbt.root(T) : rec.root(T), T);
                key = (uint64_t)__float_as_uint(tmax) << 32 | 0xFFFFFFFFull;
                feature = 0;
                bt = 0.f;
            }
        });
        if (__ballot(has) == 0 && rf.drained) break;
        if (!has) continue;
        bool done = false;
        const bool isleaf = (w.node & LEAF_BIT) != 0;
        // one fetch for every active lane, leaf or node, before the branch (k_nearest)
        v4f q0, q1, q2, q3;
        uint32_t cl = 0, cr = 0;
        if (!NB || isleaf) {
            const v4f* rr = isleaf ? reinterpret_cast<const v4f*>(leaf + 4 * (size_t)(w.node & ~LEAF_BIT))
                                   : reinterpret_cast<const v4f*>(a.inner + w.node);
            q0 = rr[0]; q1 = rr[1]; q2 = rr[2]; q3 = rr[3];
            pin(q0); pin(q1); pin(q2); pin(q3);
            if (!NB && !isleaf) {
                const uint32_t own = __float_as_uint(q3.z);
                cl = child_slot(__float_as_uint(q3.x), own, 0);
                cr = child_slot(__float_as_uint(q3.y), own, 1);
            }
        } else {
            const ChildPair ch = nbt.children(w.node);
            cl = ch.cl;
            cr = ch.cr;
            q0 = v4f{ch.llo.x, ch.llo.y, ch.lhi.x, ch.lhi.y};   // the record's layout
            q1 = v4f{ch.rlo.x, ch.rlo.y, ch.rhi.x, ch.rhi.y};
            q2 = v4f{ch.lz0, ch.lz1, ch.rz0, ch.rz1};
            q3 = v4f{0.f, 0.f, 0.f, 0.f};
        }
        const float bound = key_t(key);   // t_max until a member is found (ANY: to the end)
        const f2v rr2 = {rad, rad};
        if (--w.guard == 0) {
            c.overflow++;
            done = true;
        } else if (isleaf) {
            if (COUNT) c.leaf++;
            float mn;   // the leaf's own grown box first, with the current bound (words 10..15 of the record)
            if (query_box<true>(o, inv, f2v{q2.z, q2.w} - rr2, f2v{q3.y, q3.z} + rr2, q3.x - rad, q3.w + rad, false, 0.f,
                                bound, mn)) {
                float t;
                const uint32_t f = sweep_pair(o, d, rad, tmax, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y),
                                              mk(q1.z, q1.w, q2.x), mk(q2.z, q2.w, q3.x), mk(q3.y, q3.z, q3.w), t);
                const uint64_t cand = (uint64_t)__float_as_uint(fmaxf(t, mn) + 0.f) << 32 |
                                      (__float_as_uint(q2.y) & ~LEAF_BIT);
                if (f != 0 && cand < key) {
                    key = cand;
                    w.bl = w.node & ~LEAF_BIT;
                    feature = f;
                    bt = t;
                    if (ANY) done = true;
                }
            }
            walk_pop(w, st);
            done = done || w.sp == -1;
        } else {
            if (COUNT) c.internal++;
            // A child's box: the slab test without the axes whose 1 / d is infinite (a NaN there drops the axis out of
            // mn and mx).  On such an axis 0 * inf = NaN drops a face at exactly o_k, so a flat leaf box there passes
            // (B) while a box around it with its other face elsewhere gives [+-inf, +-inf] and fails: the one case
            // where the slab test is not monotone in the box -- and here, unlike a ray, a sphere does
            // touch such a triangle, through its edges.  Without the axis the test is monotone again, enters every
            // box the full test enters, and its mn is never above the full one's.
            // A direction below 2^-128 on all three axes leaves no axis: every child is entered.
            const float qnan = __uint_as_float(0x7FC00000u);
            const bool ix = fabsf(inv.x) == INFINITY, iy = fabsf(inv.y) == INFINITY, iz = fabsf(inv.z) == INFINITY;
            const f3 invn = mk(ix ? qnan : inv.x, iy ? qnan : inv.y, iz ? qnan : inv.z);
            const bool all = ix && iy && iz;
            float ml, mr;
            const bool lh = query_box<true>(o, invn, q0.xy - rr2, q0.zw + rr2, q2.x - rad, q2.y + rad, false, 0.f, bound, ml) || all;
            const bool rh = query_box<true>(o, invn, q1.xy - rr2, q1.zw + rr2, q2.z - rad, q2.w + rad, false, 0.f, bound, mr) || all;
            if (!lh && !rh) {
                walk_pop(w, st);
            } else if (lh && rh && w.sp + 1 >= limit) {   // the stack limit: both children lost, counted
                c.overflow++;
                walk_pop(w, st);
            } else {
                const bool swap = lh && rh && mr < ml;   // the nearer child first, left on a tie
                if (lh && rh) {
                    st.store(w.sp, w.top);   // push the other
                    w.sp++;
                    w.top = swap ? cl : cr;
                }
                w.node = swap ? cr : (lh ? cl : cr);
            }
            done = w.sp == -1;
        }
        if (done) {
            float4 o0 = none0, o1 = none1;
            if (feature != 0) {   // the winner's point, recomputed from its leaf record
                const float4* lr = leaf + 4 * (size_t)w.bl;
                const float4 la = lr[0], lb = lr[1], lc = lr[2], ld = lr[3];
                const f3 ta = mk(la.x, la.y, la.z), te1 = mk(la.w, lb.x, lb.y), te2 = mk(lb.z, lb.w, lc.x);
                const f3 lo = mk(lc.z, lc.w, ld.x), hi = mk(ld.y, ld.z, ld.w);
                f3 pt = mk(0.f, 0.f, 0.f);
                if (feature == 1u) {
                    float u, v;
                    triangle_dist2(o, ta, te1, te2, lo, hi, u, v, pt);
                } else {
                    sweep_candidate<true>((int)feature - 2, o, d, dot(d, d), rad, ta, te1, te2, pt);
                }
                pt = clamp_box(lo, hi, pt);
                o0 = make_float4(bt, pt.x, pt.y, pt.z);
                o1 = make_float4(__uint_as_float((uint32_t)key), __uint_as_float(feature), 0.f, 0.f);
            }
            a.hits[2 * (size_t)r] = o0;
            a.hits[2 * (size_t)r + 1] = o1;
            has = false;
            if (COUNT) nhits += feature != 0;
        }
    }
    if (COUNT || __ballot(c.overflow != 0)) {
        unsigned long long v[5] = {nsweeps, nhits, c.internal, c.leaf, c.overflow};
        wave_sum(v);
        if (lane == 0) {
            if (COUNT)
                for (int k = 0; k < 4; k++) atomicAdd(&a.counts[k], v[k]);
            if (v[4]) atomicAdd(a.overflow, v[4]);
        }
    }
}

}  // namespace

void launch_sweep(const SweepArgs& a, bool any, bool count, hipStream_t s) {
    if (a.n == 0) return;
    // the persistent grid of the kernel's occupancy, or a workgroup per 256 sweeps when that is fewer
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK, blocks = need < 256 * SWEEP_WAVES ? need : 256 * SWEEP_WAVES;
    with_bools([&](auto ANY, auto COUNT, auto NB) {
        hipLaunchKernelGGL((k_sweep<ANY, COUNT, NB>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, any, count, a.nb);
}

void launch_clearance(const ClearanceArgs& a, bool count, hipStream_t s) {
    if (a.n == 0) return;
    // the persistent grid of the kernel's occupancy, or a workgroup per 256 triangles when that is fewer
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK, blocks = need < 256 * CLEARANCE_WAVES ? need : 256 * CLEARANCE_WAVES;
    with_bools([&](auto COUNT, auto NB) {
        hipLaunchKernelGGL((k_clearance<COUNT, NB>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, count, a.nb);
}

void launch_cross(const CrossArgs& a, CrossPass pass, bool count, hipStream_t s) {
    if (a.n == 0) return;
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK, blocks = need < 256 * BOUNCE_WAVES ? need : 256 * BOUNCE_WAVES;
    with_bools([&](auto COUNT, auto NB) {
        if (pass == CROSS_PASS_SIZES)
            hipLaunchKernelGGL((k_cross<CROSS_PASS_SIZES, COUNT, NB>), dim3(blocks), dim3(BLOCK), 0, s, a);
        else if (pass == CROSS_PASS_FILL)
            hipLaunchKernelGGL((k_cross<CROSS_PASS_FILL, COUNT, NB>), dim3(blocks), dim3(BLOCK), 0, s, a);
        else
            hipLaunchKernelGGL((k_cross<CROSS_PASS_FIRST, COUNT, NB>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, count, a.nb);
}

void launch_cross_keys(const float4* tris, uint32_t n, const float* box, uint32_t* keys, uint32_t* vals,
                       hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_cross_keys, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, tris, n, box, keys, vals);
}

void launch_collide(const CollideArgs& a, bool fill, bool count, bool tri, bool sym, hipStream_t s) {
    if (a.T == 0) return;
    const uint32_t need = (a.T + BLOCK - 1) / BLOCK, blocks = need < 256 * BOUNCE_WAVES ? need : 256 * BOUNCE_WAVES;
    with_bools([&](auto FILL, auto COUNT, auto NB, auto TRI, auto SYM) {
        hipLaunchKernelGGL((k_collide<FILL, COUNT, NB, TRI, SYM>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, fill, count, a.nb, tri, sym);
}

void launch_signed(const SignedArgs& a, bool count, bool near, bool vote3, hipStream_t s) {
    if (a.n == 0) return;
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK, blocks = need < 256 * BOUNCE_WAVES ? need : 256 * BOUNCE_WAVES;
    with_bools([&](auto COUNT, auto NB, auto NEAR, auto VOTE3) {
        hipLaunchKernelGGL((k_signed<COUNT, NB, NEAR, VOTE3>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, count, a.nb, near, vote3);
}

void launch_overlap(const OverlapArgs& a, bool fill, bool count, bool tri, hipStream_t s) {
    if (a.n == 0) return;
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK, blocks = need < 256 * BOUNCE_WAVES ? need : 256 * BOUNCE_WAVES;
    with_bools([&](auto FILL, auto COUNT, auto NB, auto TRI) {
        hipLaunchKernelGGL((k_overlap<FILL, COUNT, NB, TRI>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, fill, count, a.nb, tri);
}

void launch_overlap_keys(const float4* boxes, uint32_t n, const float* box, uint32_t* keys, uint32_t* vals,
                         hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_overlap_keys, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, boxes, n, box, keys, vals);
}

void launch_region(const RegionArgs& a, bool fill, bool count, bool tri, hipStream_t s) {
    if (a.n == 0) return;
    // the persistent grid of the kernel's occupancy, or a workgroup per 256 regions when that is fewer
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK, full = 256 * (count ? REGION_COUNT_WAVES : REGION_WAVES);
    const uint32_t blocks = need < full ? need : full;
    with_bools([&](auto FILL, auto COUNT, auto NB, auto TRI) {
        hipLaunchKernelGGL((k_region<FILL, COUNT, NB, TRI>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, fill, count, a.nb, tri);
}

void launch_region_expand(const RegionSplitArgs& a, bool count, hipStream_t s) {
    if (a.r.n == 0) return;
    const size_t lds = 2 * sizeof(uint2) << a.kshift;   // (<= 64 KB: kshift <= REGION_SPLIT_MAX_SHIFT)
    if (a.r.nb) hipLaunchKernelGGL(k_region_expand<true>, dim3(a.r.n), dim3(64), lds, s, a, count);
    else hipLaunchKernelGGL(k_region_expand<false>, dim3(a.r.n), dim3(64), lds, s, a, count);
}

void launch_region_piece(const RegionSplitArgs& a, bool fill, bool count, bool tri, hipStream_t s) {
    if (a.r.n == 0) return;
    const uint32_t slots = a.r.n << a.kshift;
    const uint32_t need = (slots + BLOCK - 1) / BLOCK, full = 256 * (count ? REGION_COUNT_WAVES : REGION_WAVES);
    const uint32_t blocks = need < full ? need : full;
    with_bools([&](auto FILL, auto COUNT, auto NB, auto TRI) {
        hipLaunchKernelGGL((k_region_piece<FILL, COUNT, NB, TRI>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, fill, count, a.r.nb, tri);
}

void launch_region_offsets(const unsigned long long* poff, unsigned long long* offsets, uint32_t n, uint32_t kshift,
                           hipStream_t s) {
    hipLaunchKernelGGL(k_region_offsets, dim3((n + 1 + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, poff, offsets, n, kshift);
}

void launch_leaf_nan(const float4* leaf, uint32_t T, uint32_t* word, hipStream_t s) {
    if (T == 0) return;
    hipLaunchKernelGGL(k_leaf_nan, dim3((T + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, leaf, T, word);
}

void launch_allhits(const AllhitsArgs& a, bool fill, bool count, hipStream_t s) {
    if (a.n == 0) return;
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK, blocks = need < 256 * BOUNCE_WAVES ? need : 256 * BOUNCE_WAVES;
    with_bools([&](auto FILL, auto COUNT, auto NB) {
        hipLaunchKernelGGL((k_allhits<FILL, COUNT, NB>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, fill, count, a.nb);
}

void launch_allhits_order(float4* hits, const unsigned long long* offsets, const uint32_t* written, uint32_t n,
                          uint32_t* list, uint32_t* list_n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_allhits_order_lane, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, hits, offsets, written,
                       n, list, list_n);
    // (the list's length is on the device: the workgroups past it leave at once)
    hipLaunchKernelGGL(k_allhits_order_block, dim3(n < 1024u ? n : 1024u), dim3(BLOCK), 0, s, hits, offsets, written,
                       list, list_n);
}

void launch_knn(const KnnArgs& a, bool count, hipStream_t s) {
    if (a.n == 0) return;
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK;
    auto tier = [&](auto CAP) {   // the persistent grid of the tier's occupancy, or a workgroup per 256 points
        const uint32_t full = 256 * (uint32_t)knn_blocks(CAP), blocks = need < full ? need : full;
        with_bools([&](auto COUNT, auto NB) {
            hipLaunchKernelGGL((k_knn<CAP, COUNT, NB>), dim3(blocks), dim3(BLOCK), 0, s, a);
        }, count, a.nb);
    };
    if (a.k <= 4) tier(std::integral_constant<int, 4>{});
    else if (a.k <= 8) tier(std::integral_constant<int, 8>{});
    else if (a.k <= 16) tier(std::integral_constant<int, 16>{});
    else tier(std::integral_constant<int, 32>{});
}

void launch_khits(const KhitsArgs& a, bool count, hipStream_t s) {
    if (a.n == 0) return;
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK;
    auto tier = [&](auto CAP) {   // the persistent grid of the tier's occupancy, or a workgroup per 256 rays
        const uint32_t full = 256 * (uint32_t)khits_blocks(CAP), blocks = need < full ? need : full;
        with_bools([&](auto COUNT, auto NB) {
            hipLaunchKernelGGL((k_khits<CAP, COUNT, NB>), dim3(blocks), dim3(BLOCK), 0, s, a);
        }, count, a.nb);
    };
    if (a.k <= 4) tier(std::integral_constant<int, 4>{});
    else if (a.k <= 8) tier(std::integral_constant<int, 8>{});
    else tier(std::integral_constant<int, 16>{});
}

void launch_within(const WithinArgs& a, bool fill, bool count, hipStream_t s) {
    if (a.n == 0) return;
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK, blocks = need < 256 * BOUNCE_WAVES ? need : 256 * BOUNCE_WAVES;
    with_bools([&](auto FILL, auto COUNT, auto NB) {
        hipLaunchKernelGGL((k_within<FILL, COUNT, NB>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, fill, count, a.nb);
}

void launch_nearest(const NearestArgs& a, bool count, hipStream_t s) {
    if (a.n == 0) return;
    // k_query's grid: the persistent one, or a workgroup per 256 points when that is fewer
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK, blocks = need < 256 * BOUNCE_WAVES ? need : 256 * BOUNCE_WAVES;
    with_bools([&](auto COUNT, auto NB) {
        hipLaunchKernelGGL((k_nearest<COUNT, NB>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, count, a.nb);
}

void launch_nearest_keys(const float4* points, uint32_t n, const float* box, uint32_t* keys, uint32_t* vals,
                         hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_nearest_keys, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, points, n, box, keys, vals);
}

void launch_query(const QueryArgs& a, bool any, bool count, hipStream_t s) {
    if (a.n == 0) return;
    // the persistent grid of the bounce walk (8 waves per SIMD), or a workgroup per 256 rays when that is fewer
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK, blocks = need < 256 * BOUNCE_WAVES ? need : 256 * BOUNCE_WAVES;
    with_bools([&](auto ANY, auto COUNT, auto NB) {
        hipLaunchKernelGGL((k_query<ANY, COUNT, NB>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, any, count, a.nb);
}

void launch_query_certified(const QueryArgs& a, bool any, bool count, hipStream_t s) {
    if (a.n == 0) return;
    const uint32_t need = (a.n + BLOCK - 1) / BLOCK, blocks = need < 256 * BOUNCE_WAVES ? need : 256 * BOUNCE_WAVES;
    with_bools([&](auto ANY, auto COUNT) {
        hipLaunchKernelGGL((k_query_wide<ANY, COUNT>), dim3(blocks), dim3(BLOCK), 0, s, a);
    }, any, count);
    // the listed rays in the reference order: the plain kernel with the list as its walk order, the list's length
    // read on the device, its own work counters
    QueryArgs b = a;
    b.perm = a.redo;
    b.n_dev = a.redo_n;
    b.next = a.next2;
    launch_query(b, any, count, s);
}

void launch_query_keys(const float4* rays, uint32_t n, const float* box, uint32_t* keys, uint32_t* vals,
                       hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_query_keys, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, rays, n, box, keys, vals);
}

void launch_primary(const TraceArgs& a, RayQ* q, uint32_t* qcount, bool count, bool emit, PrimaryKind kind,
                    hipStream_t s) {
    const uint32_t my_bands = a.my_bands;
    const uint32_t launch_bands = my_bands > a.band0 ? (my_bands - a.band0 + a.bstep - 1) / a.bstep : 0;
    if (launch_bands == 0 || a.W == 0) return;
    dim3 grid((a.W + 31) / 32, launch_bands);
    const auto walk = [&](auto K) {   // k_primary's walk K (PrimaryWalk)
        with_bools([&](auto COUNT, auto LIM) {
            hipLaunchKernelGGL((k_primary<COUNT, K, LIM>), grid, dim3(BLOCK), 0, s, a, q, qcount, (int)emit);
        }, count, a.limited);
    };
    using std::integral_constant;
    switch (kind) {
        case PrimaryKind::LANE_NEAREST: walk(integral_constant<int, 1>{}); break;
        case PrimaryKind::PACKET_REFERENCE: walk(integral_constant<int, 2>{}); break;
        case PrimaryKind::PACKET_NEAREST: walk(integral_constant<int, 3>{}); break;
        case PrimaryKind::PACKET_WIDE:
            if (a.acyclic) walk(integral_constant<int, 5>{});
            else walk(integral_constant<int, 4>{});
            break;
        default:   // LANE_REFERENCE: on the topology and node boxes when the trace says so (a certified one)
            if (a.nb) walk(integral_constant<int, 6>{});
            else walk(integral_constant<int, 0>{});
            break;
    }
}

void launch_zero(const ZeroList& z, hipStream_t s) {
    size_t most = 0;
    for (int k = 0; k < ZeroList::N; k++) most = most > z.words[k] ? most : z.words[k];
    if (most == 0) return;
    size_t blocks = (most + BLOCK - 1) / BLOCK;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_zero, dim3((uint32_t)blocks, ZeroList::N), dim3(BLOCK), 0, s, z);
}

bool pb_keys_used() { return !RTBVH_PB_FUSE; }

void launch_pb_bins(const TraceArgs& a, const PrimBins& pb, uint32_t rows, bool zeroed, hipStream_t s,
                    const BuildArgs* tail) {
    if (rows == 0 || a.W == 0 || a.T == 0) return;
    const uint32_t keys = pb.ntx * pb.nty * PB_NZ;
    if (!zeroed) (void)hipMemsetAsync(pb.off, 0, ((size_t)keys + 1) * sizeof(uint32_t), s);
    if (!zeroed && a.pb_list) (void)hipMemsetAsync(a.pb_list, 0, (size_t)PB_LISTS * PB_LIST_STRIDE * sizeof(uint32_t), s);
    const dim3 lg((a.T + PB_LEAVES - 1) / PB_LEAVES);
    if (tail) launch_pb_count_top(*tail, a, pb.off, pb.cur, pb.bins, pb.cap, pb.ntx, lg.x, s);
    else hipLaunchKernelGGL((k_pb_bin<false>), lg, dim3(BLOCK), 0, s, a, pb.off, pb.cur, pb.bins, pb.cap, pb.ntx);
    const uint32_t sb = (keys + PB_SCAN - 1) / PB_SCAN;
    hipLaunchKernelGGL(k_pb_sums, dim3(sb), dim3(PB_SCAN), 0, s, pb.off, pb.sums, keys);
    hipLaunchKernelGGL(k_pb_scan, dim3(sb), dim3(PB_SCAN), 0, s, pb.off, pb.cur, pb.sums, keys);
    hipLaunchKernelGGL((k_pb_bin<true>), lg, dim3(BLOCK), 0, s, a, pb.off, pb.cur, pb.bins, pb.cap, pb.ntx);
}

void launch_pb_raster(const TraceArgs& a, const PrimBins& pb, uint32_t rows, RayQ* q, uint32_t* qcount, bool count,
                      bool emit, hipStream_t s, const Redo* redo, bool small_tiles) {
    if (rows == 0 || a.W == 0 || a.T == 0) return;
    const dim3 grid(pb.ntx, pb.nty);
    uint32_t* rl = redo ? redo->list : nullptr;
    uint32_t* rc = redo ? redo->count : nullptr;
    const bool rec = a.refl_rec || a.refr_rec;
    const auto raster = [&](auto* kernel, uint32_t rb) {
        hipLaunchKernelGGL(kernel, grid, dim3(rb), 0, s, a, pb.off, pb.bins, pb.cap, pb.ntx, rows, pb.keys, q, qcount,
                           (int)emit, rl, rc);
    };
#if RTBVH_PB_FUSE
    with_bools([&](auto COUNT, auto CERT) {
        if (rec) raster(k_primary_binned<COUNT, CERT, true, true>, PB_RASTER_BLOCK);
        else if (small_tiles)
            raster(k_primary_binned<COUNT, CERT, true, false, PB_RASTER_BLOCK_SMALL>, PB_RASTER_BLOCK_SMALL);
        else raster(k_primary_binned<COUNT, CERT, true, false>, PB_RASTER_BLOCK);
    }, count, redo != nullptr);
#else
    (void)rec;
    (void)small_tiles;
    with_bools([&](auto COUNT) { raster(k_primary_binned<COUNT, false, false, true>, PB_RASTER_BLOCK); }, count);
    with_bools([&](auto COUNT, auto CERT) {
        hipLaunchKernelGGL((k_pb_shade<COUNT, CERT>), grid, dim3(PB_SHADE_BLOCK), 0, s, a, pb.off, pb.cap, pb.ntx, rows,
                           pb.keys, q, qcount, (int)emit, rl, rc);
    }, count, redo != nullptr);
#endif
    if (redo) {   // the flagged pixels, in the reference order
        with_bools([&](auto COUNT) {
            hipLaunchKernelGGL((k_primary_redo<COUNT>), dim3(REDO_BLOCKS), dim3(BLOCK), 0, s, a, rl, rc, q, qcount, (int)emit);
        }, count);
    }
}

void launch_pb_gate(const TraceArgs& a, const PrimBins& pb, RayQ* q, uint32_t* qcount, bool count, bool emit,
                    hipStream_t s, bool reference) {
    if (a.W == 0 || a.T == 0) return;
    // the tiles whose bins overflowed: the per-lane nearest-first walk (every other block returns at
    // once); a binary walk, which reads no leaf pseudo-records (a binned build writes none).  A certified
    // trace takes the reference order there (exact by construction)
    TraceArgs g = a;
    g.pb_gate = pb.off;
    g.pb_cap = pb.cap;
    g.pb_ntx = pb.ntx;
    launch_primary(g, q, qcount, count, emit, reference ? PrimaryKind::LANE_REFERENCE : PrimaryKind::LANE_NEAREST, s);
}

void launch_bounce(const TraceArgs& a, const RayQ* qin, const uint32_t* qin_count, const uint32_t* perm, RayQ* qout,
                   uint32_t* qout_count, bool count, bool emit, bool nearest, hipStream_t s) {
    const uint32_t blocks = 2048;   // 8 waves/SIMD x 1024 SIMDs / 4 waves per block; grid-stride over the queue
    with_bools([&](auto COUNT, auto NEAREST, auto LIM) {
        hipLaunchKernelGGL((k_bounce<COUNT, NEAREST, LIM>), dim3(blocks), dim3(BLOCK), 0, s, a, qin, qin_count, perm, qout,
                           qout_count, (int)emit);
    }, count, nearest, a.limited);
}

void launch_bounce_keys(const RayQ* q, const uint32_t* count, const float* box, uint32_t P, uint32_t* keys,
                        uint32_t* vals, hipStream_t s) {
    hipLaunchKernelGGL(k_bounce_keys, dim3((P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, q, count, box, P, keys, vals);
}

void launch_bounce_traverse(const TraceArgs& a, const RayQ* qin, const uint32_t* qin_count, const uint32_t* perm,
                            bool count, BounceWalk walk, float2* hitrec, uint32_t* next, uint32_t blocks,
                            hipStream_t s, bool cert, uint32_t* defer, const BounceShade* es) {
    if (blocks == 0) blocks = 2048;
    const bool wide = walk == BounceWalk::WIDE_QUANTIZED;
    // the certified walk: the 4-wide one, no stack limit, a clz64 tree (api.hip enqueue_trace)
    const bool certified = wide && cert;
    // early shading (certified passes, es): the hit records start "not written yet", shading workgroups follow the walk's
    const bool early = RTBVH_EARLY_SHADE && certified && es;
    const uint32_t nshade = early ? (es->P + ESHADE_RAYS - 1) / ESHADE_RAYS : 0u;
    if (early) hipLaunchKernelGGL(k_hit_init, dim3(1024), dim3(BLOCK), 0, s, hitrec, qin_count);
    // (the certified walk is exact on any tree over the same leaves: the walk-only tree's QNodes where there are any)
    const QNode* qn = certified && a.qnode_walk ? a.qnode_walk : a.qnode;
    const auto launch = [&](auto* kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks + nshade), dim3(BLOCK), 0, s, a.inner, qn, a.leaf, a.T, qin, qin_count,
                           perm, hitrec, next, a.counters, a.overflow, wide ? a.stack_limit4b : a.stack_limit, defer,
                           a.topo, a.nb ? a.nbox : nullptr, blocks, a, early ? es->qout : nullptr,
                           early ? es->qout_count : nullptr, early ? (int)es->emit : 0, early ? es->redo : nullptr,
                           early ? es->redo_count : nullptr);
    };
    // the guard only for a tree that may have cycles (CPUTests delta), or for COUNT's census
    const bool guard = count || !a.acyclic;
    if (certified)
        with_bools([&](auto COUNT, auto GUARD, auto ES) { launch(k_bounce_trav<COUNT, 2, false, GUARD, true, ES>); }, count,
                   guard, early);
    else if (wide)
        with_bools([&](auto COUNT, auto LIM, auto GUARD) { launch(k_bounce_trav<COUNT, 2, LIM, GUARD>); }, count, a.limited,
                   guard);
    else
        with_bools([&](auto COUNT, auto NEAREST, auto LIM, auto GUARD) {
            launch(k_bounce_trav<COUNT, NEAREST ? 1 : 0, LIM, GUARD>);
        }, count, walk == BounceWalk::NEAREST, a.limited, guard);
}

void launch_bounce_shade(const TraceArgs& a, const RayQ* qin, const uint32_t* qin_count, const float2* hitrec,
                         RayQ* qout, uint32_t* qout_count, bool count, bool emit, uint32_t P, hipStream_t s,
                         const Redo* redo) {
    if (P == 0) return;
    uint32_t* rl = redo ? redo->list : nullptr;
    uint32_t* rc = redo ? redo->count : nullptr;
    const dim3 g((P + BLOCK - 1) / BLOCK);
    with_bools([&](auto COUNT, auto CERT) {
        hipLaunchKernelGGL((k_bounce_shade<COUNT, CERT>), g, dim3(BLOCK), 0, s, a, qin, qin_count, hitrec, qout, qout_count,
                           (int)emit, rl, rc);
    }, count, redo != nullptr);
    if (redo)   // the flagged rays (and the walk's deferred rays left over), in the reference order
        with_bools([&](auto COUNT) {
            hipLaunchKernelGGL((k_bounce_redo<COUNT>), dim3(REDO_BLOCKS), dim3(BLOCK), 0, s, a, qin, rl, rc, qout,
                               qout_count, (int)emit, redo->defer, redo->dnext);
        }, count);
}

void launch_assemble(const float4* bands, const uint32_t* slots, uint32_t stride_rows, uint32_t W, uint32_t H,
                     uint32_t nranks, float4* frame, hipStream_t s) {
    const size_t n = (size_t)W * H;
    hipLaunchKernelGGL(k_assemble, dim3((uint32_t)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, bands, slots,
                       stride_rows, W, H, nranks, frame);
}

void launch_present(const float4* color, uint32_t W, uint32_t H, uint32_t* out, hipStream_t s) {
    const size_t n = (size_t)W * H;
    if (n) hipLaunchKernelGGL(k_present, dim3((uint32_t)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, color, W, H, out);
}

// the camera upload (sync_camera): the 32 floats travel as the kernel's by-value argument, so the copy is
// one dispatch in stream order -- no DMA engine, no staging of the pageable host matrices
__global__ __launch_bounds__(64) void k_set_camera(CameraWords m, float* __restrict__ cam) {
    if (threadIdx.x < 32) cam[threadIdx.x] = m.w[threadIdx.x];
}

void launch_set_camera(const float* wvp, const float* wv, float* cam, hipStream_t s) {
    CameraWords m;
    for (int i = 0; i < 16; i++) {
        m.w[i] = wvp[i];
        m.w[16 + i] = wv[i];
    }
    hipLaunchKernelGGL(k_set_camera, dim3(1), dim3(64), 0, s, m, cam);
}

void launch_count_diff(const float4* a, const float4* b, size_t n, unsigned long long* diff, hipStream_t s) {
    if (n == 0) return;
    size_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_count_diff, dim3((uint32_t)blocks), dim3(BLOCK), 0, s, reinterpret_cast<const uint4*>(a),
                       reinterpret_cast<const uint4*>(b), n, diff);
}

}  // namespace rtbvh
