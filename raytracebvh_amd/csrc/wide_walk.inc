// The 4-wide walk on the quantized nodes: its stack and its step, written once for the kernels that walk it
// (trace.hip k_bounce_trav MODE 2, k_query_wide).  A fragment, not a header: a kernel includes it twice inside its
// body -- RTBVH_WIDE_PART 1 among its declarations, RTBVH_WIDE_PART 2 where an active lane takes a step -- so the
// step is compiled as part of the kernel itself, with the kernel's own variables: as functions called with those
// variables by reference the same text gave k_bounce_trav's unguarded instances other instruction streams
// (DESIGN.md 5b).  The kernel supplies, by these names:
//   constants  COUNT, GUARD, CERT, WIDE (false: an instance that never steps; its arrays shrink to one entry)
//   the tree   inner (node records: a node without a finite grid), qn (QNodes), leaf (leaf records), nk (CERT: the
//              margin's coefficients, mt_node_consts()), limit (stack entries the walk may use, <= STACK4B)
//   the ray    o, d, inv; qfast (it takes the slack test: qnode_fast_ray; CERT walks step only such rays)
//   its walk   node, sp (entries on its stack), guard (GUARD: steps left), key (the lexicographic (t, leaf) minimum,
//              its t the walk's bound -- a caller's initial bound included), btri (that leaf's triangle, leaf
//              record word 9), flg (CERT: set where the walk ended without the margin's word: a node without a
//              finite grid, a stack or guard overflow), c (the lane's Counts), tid (threadIdx.x)
//   part 2     done (set when the walk is over); wide_dbg in RTBVH_DEBUG_PIXEL builds (print this ray's step)
#if RTBVH_WIDE_PART == 1
// The stack: (node, entry distance) entries [0, SW) in LDS, [entry][lane], the distance a bf16 rounded toward -inf
// (6 B each); deeper entries as full pairs in scratch.
__shared__ uint32_t s_wid[WIDE ? SW : 1][BLOCK];
__shared__ uint16_t s_wt[WIDE ? SW : 1][BLOCK];
uint2 wstack[WIDE ? STACK4B - SW : 1];       // entries [SW, STACK4B)
auto wpush = [&](uint32_t id, float t) {
    if (sp < SW) {
        s_wid[sp][tid] = id;
        s_wt[sp][tid] = bf16_down(t);
    } else {
        wstack[sp - SW] = make_uint2(id, __float_as_uint(t));
    }
    ++sp;
};
// WIDE: the QNode at `node` (words q0..q3): its four entries, hit ones first by entry distance
// (k: entry distance, i: id; a missing child has INVALID and +inf)
auto qchildren = [&](v4f q0, v4f q1, v4f q2, v4f q3, float& k0, float& k1, float& k2, float& k3, uint32_t& i0,
                     uint32_t& i1, uint32_t& i2, uint32_t& i3) {
    // the four grandchildren: ids (a3.x, a3.y, b3.x, b3.y), entry distances t0..t3
    uint4 a3, b3;
    float t0, t1, t2, t3;
    bool h0, h1, h2, h3;
    const float kbb = key_t(key);
    if (CERT || q0.w != 0.f) {   // quantized node: q0..q3 = QNode words 0..15 (CERT: the step checked)
        // scl[1], scl[2] carry the node's margin codes in their (otherwise zero) mantissas (margin.h)
        const uint32_t wy = __float_as_uint(q1.x), wz = __float_as_uint(q1.y);
        const float ox = q0.x, oy = q0.y, oz = q0.z, sx = q0.w;
        const float sy = __uint_as_float(wy & 0xFF800000u), sz = __uint_as_float(wz & 0xFF800000u);
        const uint32_t lx = __float_as_uint(q1.z), ly = __float_as_uint(q1.w), lz = __float_as_uint(q2.x);
        const uint32_t hx = __float_as_uint(q2.y), hy = __float_as_uint(q2.z), hz = __float_as_uint(q2.w);
        a3 = make_uint4(__float_as_uint(q3.x), __float_as_uint(q3.y), 0u, 0u);
        b3 = make_uint4(__float_as_uint(q3.z), __float_as_uint(q3.w), 0u, 0u);
        // (CERT: a ray the slack test cannot take never steps -- it is flagged at its first step -- so
        // every stepping ray takes this branch)
        if (qfast || CERT) {
            // CERT: the node's margin rho_n(best) (0 before the first bound) and its range
            float rr = 0.f, tcn = 0.f;
            MtNodeRho nr{0.f, 0.f};
            if (CERT) {
                nr = mt_node_prep(nk, mt_code_val(wy));
                tcn = mt_code_val(wz);
                rr = kbb < __builtin_inff() ? mt_node_eval(nr, kbb) : 0.f;
            }
            const QAxis X = qaxis<CERT>(ox, sx, lx, hx, o.x, inv.x, rr),
                        Y = qaxis<CERT>(oy, sy, ly, hy, o.y, inv.y, rr),
                        Z = qaxis<CERT>(oz, sz, lz, hz, o.z, inv.z, rr);
            if (CERT) {
                const f3 ai = mk(fabsf(inv.x), fabsf(inv.y), fabsf(inv.z));
                h0 = qbox_fast_cert(X, Y, Z, 0, kbb, nk, nr, ai, tcn, t0);
                h1 = qbox_fast_cert(X, Y, Z, 1, kbb, nk, nr, ai, tcn, t1);
                h2 = qbox_fast_cert(X, Y, Z, 2, kbb, nk, nr, ai, tcn, t2);
                h3 = qbox_fast_cert(X, Y, Z, 3, kbb, nk, nr, ai, tcn, t3);
            } else {
                h0 = qbox_fast(X, Y, Z, 0, true, kbb, t0);
                h1 = qbox_fast(X, Y, Z, 1, true, kbb, t1);
                h2 = qbox_fast(X, Y, Z, 2, true, kbb, t2);
                h3 = qbox_fast(X, Y, Z, 3, true, kbb, t3);
            }
        } else {
#define RTBVH_QBOX(c, t)                                                                                      \
ray_box(o, inv, qdecode(ox, sx, lx, c), qdecode(oy, sy, ly, c), qdecode(oz, sz, lz, c), qdecode(ox, sx, hx, c), \
    qdecode(oy, sy, hy, c), qdecode(oz, sz, hz, c), true, kbb, t)
            h0 = RTBVH_QBOX(0, t0);
            h1 = RTBVH_QBOX(1, t1);
            h2 = RTBVH_QBOX(2, t2);
            h3 = RTBVH_QBOX(3, t3);
#undef RTBVH_QBOX
        }
        h1 = h1 & (a3.y != INVALID);
        h3 = h3 & (b3.y != INVALID);
    } else {
        // a node without a finite grid: its exact record pair (node = its slot; the
        // pair of its children's records is at 2 * own, own = word 14 of its record; the
        // build writes the pseudo-records of such a node's leaf children whatever the flags).
        // (Not widened by the margin: a certified walk ends the ray there, flagged -- below)
        const uint32_t own = __float_as_uint(reinterpret_cast<const v4f*>(inner + node)[3].z);
        const v4f* pr = reinterpret_cast<const v4f*>(inner + 2 * (size_t)own);
        q0 = pr[0]; q1 = pr[1]; q2 = pr[2]; q3 = pr[3];
        const v4f q4 = pr[4], q5 = pr[5], q6 = pr[6], q7 = pr[7];
        a3 = make_uint4(__float_as_uint(q3.x), __float_as_uint(q3.y), 0u, 0u);
        b3 = make_uint4(__float_as_uint(q7.x), __float_as_uint(q7.y), 0u, 0u);
        // grandchild ids -> slots (2 * parent + side; parent = word 14)
        const uint32_t ol = __float_as_uint(q3.z), orr = __float_as_uint(q7.z);
        if (!(a3.x & LEAF_BIT)) a3.x = 2 * ol;
        if (a3.y != INVALID && !(a3.y & LEAF_BIT)) a3.y = 2 * ol + 1;
        if (!(b3.x & LEAF_BIT)) b3.x = 2 * orr;
        if (b3.y != INVALID && !(b3.y & LEAF_BIT)) b3.y = 2 * orr + 1;
        h0 = ray_box_xy(o, inv, q0.xy, q0.zw, q2.x, q2.y, true, kbb, t0);
        h1 = ray_box_xy(o, inv, q1.xy, q1.zw, q2.z, q2.w, true, kbb, t1) & (a3.y != INVALID);
        h2 = ray_box_xy(o, inv, q4.xy, q4.zw, q6.x, q6.y, true, kbb, t2);
        h3 = ray_box_xy(o, inv, q5.xy, q5.zw, q6.z, q6.w, true, kbb, t3) & (b3.y != INVALID);
    }
    const float INF = __builtin_inff();
    k0 = h0 ? t0 : INF; k1 = h1 ? t1 : INF; k2 = h2 ? t2 : INF; k3 = h3 ? t3 : INF;
    i0 = h0 ? a3.x : INVALID; i1 = h1 ? a3.y : INVALID; i2 = h2 ? b3.x : INVALID; i3 = h3 ? b3.y : INVALID;
    // 4-element sorting network on the entry distance (missing children last)
    sort2(k0, i0, k1, i1);
    sort2(k2, i2, k3, i3);
    sort2(k0, i0, k2, i2);
    sort2(k1, i1, k3, i3);
    sort2(k1, i1, k2, i2);
};
#elif RTBVH_WIDE_PART == 2
// A step: the QNode of an internal `node`, then one leaf test -- the nearest child when it
// is a leaf (the next child is visited), or the leaf the step began at -- so a leaf found
// by the node test costs no step of its own, and the leaf test is one block of code.
uint32_t L = INVALID;
if (GUARD && --guard == 0) {
    c.overflow++;
    done = true;
    if (CERT) flg = true;
} else {
    if (node & LEAF_BIT) {
        L = node;
        node = INVALID;
    } else {
        const v4f* rr = reinterpret_cast<const v4f*>(qn + node);
        v4f q0 = rr[0], q1 = rr[1], q2 = rr[2], q3 = rr[3];
        pin(q0); pin(q1); pin(q2); pin(q3);
        if (COUNT) c.internal++;
        float k0 = 0.f, k1 = 0.f, k2 = 0.f, k3 = 0.f;
        uint32_t i0 = INVALID, i1 = INVALID, i2 = INVALID, i3 = INVALID;
        // CERT: a node without a finite grid (its corners past 2^100: the margin does not cover
        // its exact boxes) ends the walk, the ray flagged for the reference-order re-trace
        if (CERT && q0.w == 0.f) {
            flg = true;
            done = true;
        } else {
            qchildren(q0, q1, q2, q3, k0, k1, k2, k3, i0, i1, i2, i3);
        }
#ifdef RTBVH_DEBUG_PIXEL   // (scripts/debug_walk.py: one ray's walk, step by step, from the COUNT kernel)
        if (wide_dbg)
            printf("DBG %d q %u sp %d kb %.6g key %.6g | %.6g %x %.6g %x %.6g %x %.6g %x\n", (int)CERT, node,
                   sp, key_t(key), key_t(key), k0, i0, k1, i1, k2, i2, k3, i3);
#endif
        const bool lf0 = i0 != INVALID && (i0 & LEAF_BIT);
        L = lf0 ? i0 : INVALID;
        node = lf0 ? i1 : i0;   // INVALID when no child is left -> pop below
        if (sp + 3 > limit) {
            c.overflow++;
            done = true;
            if (CERT) flg = true;
        } else {   // push the others farthest first
            if (i3 != INVALID) wpush(i3, k3);
            if (i2 != INVALID) wpush(i2, k2);
            if (!lf0 && i1 != INVALID) wpush(i1, k1);
        }
    }
#ifdef RTBVH_DEBUG_PIXEL
    if (wide_dbg && L != INVALID)
        printf("DBG %d leaf %x sp %d kb %.6g key %.6g\n", (int)CERT, L, sp, key_t(key), key_t(key));
#endif
    if (L != INVALID) {   // branch-free test (the same accept predicate), u64 key minimum
        const uint32_t j = L & ~LEAF_BIT;
        const v4f* lr = reinterpret_cast<const v4f*>(leaf + 4 * (size_t)j);
        v4f la = lr[0], lb = lr[1], lc = lr[2];
        pin(la); pin(lb); pin(lc);
        if (COUNT) c.leaf++;
        const float tw = ray_triangle_flat(o, d, mk(la.x, la.y, la.z), mk(la.w, lb.x, lb.y),
                                           mk(lb.z, lb.w, lc.x), true);
        const uint64_t k = tw == -1.f ? ~0ull : (uint64_t)__float_as_uint(tw) << 32 | j;
        btri = k < key ? __float_as_uint(lc.y) & ~LEAF_BIT : btri;
        key = k < key ? k : key;
    }
    if (!done && node == INVALID) {   // pop, dropping entries that cannot improve
        while (sp > 0) {
            --sp;
            uint2 e;
            if (sp < SW) e = make_uint2(s_wid[sp][tid], __float_as_uint(bf16_up(s_wt[sp][tid])));
            else e = wstack[sp - SW];
            if (__uint_as_float(e.y) <= key_t(key)) {
                node = e.x;
                break;
            }
        }
        done = node == INVALID;
    }
}
#else
#error "wide_walk.inc: define RTBVH_WIDE_PART as 1 (declarations) or 2 (the step)"
#endif
#undef RTBVH_WIDE_PART
