// dtrav.h — BVH traversal: the per-lane stack, the interior and leaf steps, and what the persistent kernels of kernels_trav.hip
// share of their loop. Part of dpath.h, which includes it between the ray / primitive tests it uses and the code that uses it.
// (Included inside dpath.h's namespace iile.)
#pragma once
// ===========================================================================
// BVH traversal (accelerators/bvh.cpp:662-738, core/geometry.h:1411-1438)
// ===========================================================================
// Same tree, same visiting order and the same accept / reject decisions as the
// reference, restructured for 64-lane wavefronts:
//
//  * "Wide" 64-byte interior records hold the boxes of BOTH children
//    (children[0] = the node at i+1, children[1] = secondChildOffset), so one
//    fetch resolves two of the reference's node visits and leaves need no node
//    fetch at all (a leaf reference is ~firstPrimitive; the last primitive of a
//    leaf carries a flag bit in its vertex record).
//  * The near child is tested and entered at once. The far child's slab test
//    does not depend on ray.tMax except for its final `tMin < ray.tMax`
//    comparison (geometry.h:1437), so its tMin is cached on the stack and that
//    one comparison is repeated at pop time against the tMax of that moment —
//    the decision the reference takes when it visits the node later.
//  * while-while: lanes first walk interior nodes (cheap iterations), then all
//    lanes that reached a leaf run the triangle test together, instead of paying
//    the triangle code on every iteration because some lane is at a leaf.
//  * One ray per lane; per-lane stack of (ref, tMin) in LDS as stack[level][lane]
//    (64 dwords per level): lane l always hits bank l mod 32, so pushes and pops
//    are conflict-free whatever depth each lane is at. The LDS part is a ring holding the
//    newest kLdsStackDepth levels; older ones are evicted to an HBM column (see stack_push).
//
// LDS pointers carry their address space explicitly so that pushes and pops
// compile to ds_write_b32 / ds_read_b32 (a generic pointer would go through flat_*).
typedef __attribute__((address_space(3))) int lds_int;
#ifndef IILE_LDS_STACK
#define IILE_LDS_STACK 11  // 22 KB per block + the 3 KB copy of the tree's top: six blocks per 160 KB CU
#endif
constexpr int kLdsStackDepth = IILE_LDS_STACK;  // measured max depth on killeroo-simple: 19 (binary steps)
// The reference's stack holds 64 binary entries (bvh.cpp:670); a four-wide step defers up to
// three slots where the binary walk defers one child, so the same tree needs up to 1.5x that.
constexpr int kSpillStackDepth = 128 - IILE_LDS_STACK;
// The deepest tree a lane's stack is sure to hold; iile_scene_create refuses a deeper one (api_scene.hip). Depth = interior nodes
// on the longest path from the root to a leaf: what the reference's nodesToVisit[64] holds at most, since its walk defers one
// child per interior node it enters — and it does not check either (bvh.cpp:670), so 64 is also where the reference ends.
// Here a binary step (instrumented kernels, rays with an infinite 1/d) defers one entry per level; a four-wide step at node P
// descends to a grandchild, two levels, and defers at most the three other slots (entering a leaf child, one level, it defers at
// most two and the descent ends). A path of `depth` levels therefore holds at most 3 * ceil(depth / 2) entries: 96 for 64, of
// the kLdsStackDepth + kSpillStackDepth = 128 a lane's ring and HBM column hold together, and of the 255 Trav::sp counts.
constexpr int kMaxBvhDepth = 64;
constexpr int stack_levels_needed(int depth) { return 3 * ((depth + 1) / 2); }
static_assert(stack_levels_needed(kMaxBvhDepth) <= IILE_LDS_STACK + kSpillStackDepth && kMaxBvhDepth <= IILE_LDS_STACK + kSpillStackDepth,
              "a tree of kMaxBvhDepth levels must fit a lane's LDS ring plus its HBM column");
static_assert(IILE_LDS_STACK + kSpillStackDepth < 256, "Trav::sp counts the stack's levels in 8 bits");
constexpr int kStackWordsPerWave = 2 * kLdsStackDepth * 64;  // ref plane + tMin plane

struct TraceStats {
    uint32_t nodes, tris, tri_hits, spheres;
};

struct HitRec {
    int prim;  // -1 = miss
    float t, b0, b1, b2;
};

// Bounds3::IntersectP(ray, invDir, dirIsNeg) without its final ray.tMax
// comparison: returns whether the slabs overlap with tMax_box > 0 and the entry
// distance tMin. The caller finishes with `tMin < ray.tMax`.
DEV bool slab_entry(const RayCtx &rc, float bminx, float bminy, float bminz, float bmaxx, float bmaxy, float bmaxz,
                    float *tmin_out) {
    const bool nx = rc.neg_mask & 1, ny = (rc.neg_mask & 2) != 0, nz = (rc.neg_mask & 4) != 0;
    float tmin = ((nx ? bmaxx : bminx) - rc.ox) * rc.inv_dir.x;
    float tmx = ((nx ? bminx : bmaxx) - rc.ox) * rc.inv_dir.x;
    float tymin = ((ny ? bmaxy : bminy) - rc.oy) * rc.inv_dir.y;
    float tymax = ((ny ? bminy : bmaxy) - rc.oy) * rc.inv_dir.y;
    tmx *= kSlabScale;
    tymax *= kSlabScale;
    bool ok = !(tmin > tymax || tymin > tmx);
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmx) tmx = tymax;
    float tzmin = ((nz ? bmaxz : bminz) - rc.oz) * rc.inv_dir.z;
    float tzmax = ((nz ? bminz : bmaxz) - rc.oz) * rc.inv_dir.z;
    tzmax *= kSlabScale;
    ok = ok && !(tmin > tzmax || tzmin > tmx);
    if (tzmin > tmin) tmin = tzmin;
    if (tzmax < tmx) tmx = tzmax;
    *tmin_out = tmin;
    return ok && (tmx > 0);
}

// The same test for a ray whose slab products cannot be NaN (all 1/d finite: neg_mask bit 7
// clear). Without NaNs the reference's compare-and-replace chain selects exactly
// max(tx0, ty0, tz0) and min(tx1, ty1, tz1), and its two overlap tests pass iff the three
// intervals share a point, i.e. iff that maximum <= that minimum. (The chain never tests an
// axis interval against itself; one can only be inverted by the 1+2*gamma(3) scaling of a
// negative far plane, and then tMax < 0 fails both formulations.) v_max3/v_min3 replace
// eight compare/select pairs; signed zeros can differ but tMin/tMax are only ever compared.
// Both child boxes at once, as float2 lanes (v_pk_add_f32 / v_pk_mul_f32 are full rate).
typedef float v2f __attribute__((ext_vector_type(2)));
DEV void slab_entry_finite2(const RayCtx &rc, const float4 q0, const float4 q1, const float4 q2, bool *ok_a,
                            bool *ok_b, float *tmin_a, float *tmin_b) {
    // children[0] = (q0.xyz, q0.w q1.xy), children[1] = (q1.zw q2.x, q2.yzw)
    const bool nx = rc.neg_mask & 1, ny = (rc.neg_mask & 2) != 0, nz = (rc.neg_mask & 4) != 0;
    const v2f x0 = v2f{nx ? q0.w : q0.x, nx ? q2.y : q1.z}, x1 = v2f{nx ? q0.x : q0.w, nx ? q1.z : q2.y};
    const v2f y0 = v2f{ny ? q1.x : q0.y, ny ? q2.z : q1.w}, y1 = v2f{ny ? q0.y : q1.x, ny ? q1.w : q2.z};
    const v2f z0 = v2f{nz ? q1.y : q0.z, nz ? q2.w : q2.x}, z1 = v2f{nz ? q0.z : q1.y, nz ? q2.x : q2.w};
    const float fox = rc.ox, foy = rc.oy, foz = rc.oz, fix = rc.inv_dir.x, fiy = rc.inv_dir.y, fiz = rc.inv_dir.z;
    const v2f ox = v2f{fox, fox}, oy = v2f{foy, foy}, oz = v2f{foz, foz}, ix = v2f{fix, fix}, iy = v2f{fiy, fiy},
              iz = v2f{fiz, fiz}, sc = v2f{kSlabScale, kSlabScale};
    const v2f tx0 = (x0 - ox) * ix, tx1 = (x1 - ox) * ix * sc;
    const v2f ty0 = (y0 - oy) * iy, ty1 = (y1 - oy) * iy * sc;
    const v2f tz0 = (z0 - oz) * iz, tz1 = (z1 - oz) * iz * sc;
    const float mna = __builtin_fmaxf(__builtin_fmaxf(tx0.x, ty0.x), tz0.x);
    const float mxa = __builtin_fminf(__builtin_fminf(tx1.x, ty1.x), tz1.x);
    const float mnb = __builtin_fmaxf(__builtin_fmaxf(tx0.y, ty0.y), tz0.y);
    const float mxb = __builtin_fminf(__builtin_fminf(tx1.y, ty1.y), tz1.y);
    *tmin_a = mna;
    *tmin_b = mnb;
    *ok_a = mna <= mxa && mxa > 0;
    *ok_b = mnb <= mxb && mxb > 0;
}

// Resumable traversal state of one lane. The persistent kernels keep a Trav per
// lane and run the interior / leaf phases for the whole wavefront, refilling
// lanes whose ray has finished; traverse() below is the single-ray wrapper.
struct Trav {
    RayCtx rc;
    float tmax;
    int cur = 0;  // >= 0: wide interior record; < 0: leaf, ~cur = first primitive (the initialisers: an idle lane, no ray)
    int sp = 0;
    bool have = false;  // cur is a node that passed its box test and still has to be processed
    int hit_prim = -1;  // -1: none; else primitive index | hit_tag(flags)
    float b0, b1, b2;  // barycentrics of the closest triangle hit (t itself is t.tmax)
};
// The vertex record's flag word carries the primitive's shading class (bits 5..7: material
// type, +4 for a sphere) and whether it is an area light (bit 8; bits 9..11 are clear; WHICH light
// is the record's third word). Both ride along in hit_prim bits 24..30, so that extend can tag
// shade-queue entries with the class and the MIS kernel knows whether its ray ended on an emitter,
// without fetching the primitive again.
constexpr int kHitClassShift = 24;
constexpr int kHitLightShift = 27;
constexpr int kHitPrimMask = (1 << kHitClassShift) - 1;
DEV int hit_tag(uint32_t flags) { return int((flags >> 5) & 0x7fu) << kHitClassShift; }
DEV int hit_index(int hit_prim) { return hit_prim < 0 ? -1 : (hit_prim & kHitPrimMask); }
// The top of the tree in LDS. The traversal kernels are bound by the vector memory pipe, not by arithmetic (r03 counters:
// TA busy 0.74-0.86, TD busy 0.92-0.99 of the kernel's cycles; a divergent dwordx4 load costs ~26 address-unit cycles and an
// interior step issues seven of them against ~60 cycles of VALU per CU): the records every ray passes through first — the
// breadth-first top of the four-wide tree — are therefore read from a per-block LDS copy, which takes no part in that pipe.
// A reference to such a record is kTopFlag | slot (still > 0 = interior); the copies refer to each other that way and to
// everything below by the ordinary record index. Same records, same decisions.
constexpr int kTopStride = 144;  // bytes per LDS record: 128 + 16, so that neighbouring records start 4 banks apart
typedef __attribute__((address_space(3))) char lds_char;
struct StackRef {
    lds_int *lds;          // this lane's LDS column: ref plane [level*64], tMin plane [(kLdsStackDepth+level)*64]
    int *spill_base;       // HBM overflow: lane column = spill_base + spill_col, 2 ints per level
    uint32_t spill_col;
    uint32_t spill_stride;
    lds_char *top = nullptr;  // the block's copy of DScene::top4 (kTopStride bytes per record), or null
    int root = 0;             // where a traversal starts: DScene::root_ref_top with `top`, else DScene::root_ref
    DEV int *spill() const { return spill_base + spill_col; }
};
// a block's threads copy the top records into its LDS array (kMaxTop * kTopStride bytes); the caller synchronises
typedef float lds_v4f_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) lds_v4f_t lds_v4f;  // (HIP's float4 is a class: no assignment across address spaces)
DEV float4 lds_load4(lds_char *p) {
    const lds_v4f_t v = *reinterpret_cast<lds_v4f *>(p);
    return make_float4(v.x, v.y, v.z, v.w);
}
DEV void stage_top_records(const DScene &S, lds_char *top, int tid, int n_threads) {
    for (int i = tid; i < S.n_top * 8; i += n_threads) {
        const float4 v = S.top4[i];
        *reinterpret_cast<lds_v4f *>(top + (i >> 3) * kTopStride + (i & 7) * 16) = lds_v4f_t{v.x, v.y, v.z, v.w};
    }
}

template <bool COUNT>
DEV void trav_begin(const DScene &S, Trav &t, F3 ro, F3 rd, float tmax, TraceStats *st, int root) {
    t.rc = make_ray_ctx(ro, rd);
    t.tmax = tmax;
    t.sp = 0;
    t.hit_prim = -1;
    t.b0 = t.b1 = t.b2 = 0;
    t.cur = root;
    t.have = false;
    if (S.n_nodes == 0) return;
    // the root is visited like any node: its own box against ray.tMax
    float tmin;
    if (COUNT) ++st->nodes;
    const bool ok = slab_entry(t.rc, S.root_box[0], S.root_box[1], S.root_box[2], S.root_box[3], S.root_box[4],
                               S.root_box[5], &tmin);
    t.have = ok && (tmin < tmax);
}

// The per-lane stack keeps its *newest* kLdsStackDepth levels in LDS, as a ring
// (level l lives in LDS slot l mod kLdsStackDepth); when it grows beyond that, the oldest
// level is evicted to the lane's HBM column — a store nobody waits for — and comes back only
// if the traversal ever unwinds that far. (Spilling the newest levels instead, as a plain
// array would, puts an HBM round trip on the very next pop: 12 vs 14 LDS levels cost 5 ms
// per frame that way.) Trav::sp packs both cursors: bits 0..7 = number of levels on the
// stack, bits 8.. = number of levels that live in HBM (levels [0, lo)).
// level % kLdsStackDepth for level < 128 without an integer division (exact for depths 8..32)
static_assert(kLdsStackDepth >= 5 && kLdsStackDepth <= 32, "lds_slot's reciprocal is checked for depths 5..32 (levels < 256)");
DEV int lds_slot(int level) {
    constexpr int kRecip = (65536 + kLdsStackDepth - 1) / kLdsStackDepth;
    return level - kLdsStackDepth * ((level * kRecip) >> 16);
}
DEV int stack_size(const Trav &t) { return t.sp & 0xff; }
DEV void stack_push(Trav &t, const StackRef &sr, int ref, float tmin) {
    const int sp = t.sp & 0xff, lo = t.sp >> 8;
    if (sp - lo == kLdsStackDepth) {
        const int slot = lds_slot(lo);
        const size_t off = size_t(lo) * 2 * sr.spill_stride;
        sr.spill()[off] = sr.lds[slot * 64];
        sr.spill()[off + sr.spill_stride] = sr.lds[(kLdsStackDepth + slot) * 64];
        t.sp += 256;
    }
    const int slot = lds_slot(sp);
    sr.lds[slot * 64] = ref;
    sr.lds[(kLdsStackDepth + slot) * 64] = __float_as_int(tmin);
    t.sp += 1;
}
// resume at the most recent deferred (far) child that still passes `tMin < ray.tMax`
template <bool COUNT>
DEV void trav_pop(Trav &t, const StackRef &sr, TraceStats *st) {
    t.have = false;
    while ((t.sp & 0xff) > 0) {
        --t.sp;
        const int sp = t.sp & 0xff, lo = t.sp >> 8;
        int ref;
        float tmin;
        if (sp >= lo) {
            const int slot = lds_slot(sp);
            ref = sr.lds[slot * 64];
            tmin = __int_as_float(sr.lds[(kLdsStackDepth + slot) * 64]);
        } else {  // LDS ring empty: level sp is the newest one in HBM
            const size_t off = size_t(sp) * 2 * sr.spill_stride;
            ref = sr.spill()[off];
            tmin = __int_as_float(sr.spill()[off + sr.spill_stride]);
            t.sp = sp | (sp << 8);
        }
        if (COUNT) ++st->nodes;
        if (tmin < t.tmax) {
            t.cur = ref;
            t.have = true;
            break;
        }
    }
}

// one wide interior record (already fetched): two of the reference's node visits
template <bool COUNT>
DEV void trav_interior(Trav &t, const StackRef &sr, TraceStats *st, const float4 q0, const float4 q1, const float4 q2,
                       const float4 q3) {
    const int ref_a = __float_as_int(q3.x), ref_b = __float_as_int(q3.y);
    const int axis = __float_as_int(q3.z) & 3;
    // children[0] = (q0.xyz, q0.w q1.xy), children[1] = (q1.zw q2.x, q2.yzw)
    float tmin_a, tmin_b;
    bool ok_a, ok_b;
    if (__builtin_expect(__ballot(t.rc.neg_mask & 0x80) == 0, 1)) {
        slab_entry_finite2(t.rc, q0, q1, q2, &ok_a, &ok_b, &tmin_a, &tmin_b);
    } else {
        ok_a = slab_entry(t.rc, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, &tmin_a);
        ok_b = slab_entry(t.rc, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, &tmin_b);
    }
    // bvh.cpp:686-692: with a negative direction along the split axis the second
    // child is nearer; the other one is deferred
    const bool second_first = (t.rc.neg_mask >> axis) & 1;
    const int near_ref = second_first ? ref_b : ref_a, far_ref = second_first ? ref_a : ref_b;
    const bool near_ok = second_first ? ok_b : ok_a, far_ok = second_first ? ok_a : ok_b;
    const float near_tmin = second_first ? tmin_b : tmin_a, far_tmin = second_first ? tmin_a : tmin_b;
    if (COUNT || far_ok) {
        // a far child whose slabs can never pass is only kept for the visit count
        const float ft = far_ok ? far_tmin : IILE_INF;
        stack_push(t, sr, far_ref, ft);
    }
    if (COUNT) ++st->nodes;
    if (near_ok && near_tmin < t.tmax)
        t.cur = near_ref;
    else
        trav_pop<COUNT>(t, sr, st);
}
// Interior step of one lane: fetch its 64-byte record (4 x dwordx4) and process it.
// (A quad-cooperative fetch — four lanes loading one record per request and a DPP 4x4
// transpose — was measured: it removes the vector-L1 pending-miss stalls but its
// 64 extra VALU/DPP moves cost more than they save: 61 ms vs 49 ms per step.)
template <bool COUNT>
DEV void trav_interior_step(const DScene &S, Trav &t, const StackRef &sr, TraceStats *st) {
    // index clamped so that a load the compiler hoists above the loop test
    // (observed with hipcc 7.2 on this loop nest) can never leave the array
    const float4 *w = S.wide + 4 * size_t(t.cur < 0 ? 0 : t.cur);
    trav_interior<COUNT>(t, sr, st, w[0], w[1], w[2], w[3]);
}

// ---------------------------------------------------------------------------
// Four-wide step (uninstrumented kernels only). A wide4 record of binary node P holds the
// boxes and refs of its *grandchildren* in fixed slots — slots 0,1: children of P's first
// child L (or L itself in slot 0 when L is a leaf), slots 2,3: likewise for P's second child
// R — and the split axes of P, L and R. One step enters the first grandchild the reference
// would reach and defers the others in the reference's order (L's near, L's far, R's near,
// R's far, each pair and the pairs themselves ordered by dirIsNeg of the respective axis).
//
// The intermediate nodes L and R are never tested. That cannot change which leaves are tested,
// nor in which order: a child's box lies inside its parent's (Union is exact), every slab
// operation ((plane - o) * invDir, * (1 + 2 gamma3), max3/min3) is monotone, so for a ray
// without NaN slab products "child passes" implies "parent passes" — both the slab overlap
// with tMax > 0 and tMin < ray.tMax, whatever ray.tMax was when the parent was visited
// (it only shrinks). What the reference decides at L or R is therefore implied by what it
// decides at their children. Rays with an infinite 1/d (NaN-capable) take the binary step,
// which shares refs and stack entries with this one. The visit *counters* do need L and R,
// so the instrumented kernels keep the binary step.
// The six box planes of a record are loaded as "entry x / y / z" and "exit x / y / z": which of the min / max planes
// that is depends on the ray's direction signs only, so the choice is made in the load ADDRESS (per-lane anyway) from the
// three byte offsets RayCtx keeps, instead of 24 selects on loaded values per step. The exit plane of an axis is 48 bytes
// from its entry plane, in the direction an XOR gives (records are 128-byte aligned: offset bits 0..6 are the plane's).
struct Wide4Planes {
    float4 ex, ey, ez, lx, ly, lz, refs;
    uint32_t meta;
};
template <bool WITH_META>
DEV Wide4Planes load_wide4(const float4 *wide4, int cur, int neg_mask, lds_char *top = nullptr) {
    const char *base = reinterpret_cast<const char *>(wide4);
    const uint32_t nm = uint32_t(neg_mask);
    const uint32_t px = (nm >> 8) & 0xffu, py = (nm >> 16) & 0xffu, pz = nm >> 24;  // entry planes' offsets inside a record
    Wide4Planes w;
    const bool in_top = top != nullptr && cur >= kTopFlag;
    if (top != nullptr && __ballot(in_top) != 0) {
        if (in_top) {
            typedef __attribute__((address_space(3))) uint32_t lu32;
            lds_char *r = top + uint32_t(cur - kTopFlag) * uint32_t(kTopStride);
            w.ex = lds_load4(r + px);
            w.ey = lds_load4(r + py);
            w.ez = lds_load4(r + pz);
            w.lx = lds_load4(r + (px ^ 48u));
            w.ly = lds_load4(r + (py ^ 80u));
            w.lz = lds_load4(r + (pz ^ 112u));
            w.refs = lds_load4(r + 96u);
            w.meta = (WITH_META && !kRefShift) ? *reinterpret_cast<lu32 *>(r + 112u) : 0u;
        }
        if (__ballot(!in_top) == 0) return w;  // (wave-uniform: a wavefront fresh from a refill is all in the top levels)
    }
    if (!in_top) {
        const uint32_t rec = uint32_t(cur < 0 ? 0 : cur) * 128u;  // (32-bit offsets: checked at upload)
        const uint32_t ax = rec + px, ay = rec + py, az = rec + pz;
        w.ex = *reinterpret_cast<const float4 *>(base + ax);
        w.ey = *reinterpret_cast<const float4 *>(base + ay);
        w.ez = *reinterpret_cast<const float4 *>(base + az);
        w.lx = *reinterpret_cast<const float4 *>(base + (ax ^ 48u));
        w.ly = *reinterpret_cast<const float4 *>(base + (ay ^ 80u));
        w.lz = *reinterpret_cast<const float4 *>(base + (az ^ 112u));
        w.refs = *reinterpret_cast<const float4 *>(base + (rec + 96u));
        w.meta = (WITH_META && !kRefShift) ? *reinterpret_cast<const uint32_t *>(base + (rec + 112u)) : 0u;
    }
    return w;
}
// the four refs of a record as the step uses them, and its axes word (both unpacked from the refs)
DEV void unpack_refs(const Wide4Planes &w, int *r0, int *r1, int *r2, int *r3, uint32_t *meta) {
    const int p0 = __float_as_int(w.refs.x), p1 = __float_as_int(w.refs.y), p2 = __float_as_int(w.refs.z), p3 = __float_as_int(w.refs.w);
    if (kRefShift) {
        *meta = uint32_t(p0 & 3) | uint32_t(p1 & 3) << 2 | uint32_t(p2 & 3) << 4;
        *r0 = p0 >> kRefShift, *r1 = p1 >> kRefShift, *r2 = p2 >> kRefShift, *r3 = p3 >> kRefShift;  // (arithmetic: a leaf ref is negative)
    } else {
        *meta = w.meta;
        *r0 = p0, *r1 = p1, *r2 = p2, *r3 = p3;
    }
}
// The slab step of a four-wide record: per slot, the largest entry distance and the smallest (scaled) exit distance over the
// three axes — tMin and tMax of Bounds3::IntersectP before its comparisons, for a ray without NaN slab products.
DEV void slab4(const RayCtx &rc, const Wide4Planes &w, float (&tmin)[4], float (&tmx)[4]) {
    // entry / exit planes of slots (0,1) and (2,3) as float2 lanes
    const v2f x0a = v2f{w.ex.x, w.ex.y}, x0b = v2f{w.ex.z, w.ex.w}, x1a = v2f{w.lx.x, w.lx.y}, x1b = v2f{w.lx.z, w.lx.w};
    const v2f y0a = v2f{w.ey.x, w.ey.y}, y0b = v2f{w.ey.z, w.ey.w}, y1a = v2f{w.ly.x, w.ly.y}, y1b = v2f{w.ly.z, w.ly.w};
    const v2f z0a = v2f{w.ez.x, w.ez.y}, z0b = v2f{w.ez.z, w.ez.w}, z1a = v2f{w.lz.x, w.lz.y}, z1b = v2f{w.lz.z, w.lz.w};
    const float fox = rc.ox, foy = rc.oy, foz = rc.oz, fix = rc.inv_dir.x, fiy = rc.inv_dir.y, fiz = rc.inv_dir.z;
    const v2f ox = v2f{fox, fox}, oy = v2f{foy, foy}, oz = v2f{foz, foz}, ix = v2f{fix, fix}, iy = v2f{fiy, fiy},
              iz = v2f{fiz, fiz}, sc = v2f{kSlabScale, kSlabScale};
    const v2f tx0a = (x0a - ox) * ix, tx0b = (x0b - ox) * ix;
    const v2f tx1a = (x1a - ox) * ix * sc, tx1b = (x1b - ox) * ix * sc;
    const v2f ty0a = (y0a - oy) * iy, ty0b = (y0b - oy) * iy;
    const v2f ty1a = (y1a - oy) * iy * sc, ty1b = (y1b - oy) * iy * sc;
    const v2f tz0a = (z0a - oz) * iz, tz0b = (z0b - oz) * iz;
    const v2f tz1a = (z1a - oz) * iz * sc, tz1b = (z1b - oz) * iz * sc;
    auto max3 = [](float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); };
    auto min3 = [](float a, float b, float c) { return __builtin_fminf(__builtin_fminf(a, b), c); };
    tmin[0] = max3(tx0a.x, ty0a.x, tz0a.x), tmx[0] = min3(tx1a.x, ty1a.x, tz1a.x);
    tmin[1] = max3(tx0a.y, ty0a.y, tz0a.y), tmx[1] = min3(tx1a.y, ty1a.y, tz1a.y);
    tmin[2] = max3(tx0b.x, ty0b.x, tz0b.x), tmx[2] = min3(tx1b.x, ty1b.x, tz1b.x);
    tmin[3] = max3(tx0b.y, ty0b.y, tz0b.y), tmx[3] = min3(tx1b.y, ty1b.y, tz1b.y);
}
DEV void trav_interior4(Trav &t, const StackRef &sr, const Wide4Planes &w) {
    const RayCtx &rc = t.rc;
    float tmin[4], tmx[4];
    slab4(rc, w, tmin, tmx);
    // per slot: tMin, and whether it is to be visited as things stand (key = tMin, else +inf;
    // a visitable tMin is < ray.tMax <= inf, so +inf is free to mean "no")
    auto slot_key = [&](int i) { return (tmin[i] <= tmx[i] && tmx[i] > 0 && tmin[i] < t.tmax) ? tmin[i] : IILE_INF; };
    const float k0 = slot_key(0), k1 = slot_key(1), k2 = slot_key(2), k3 = slot_key(3);
    int r0, r1, r2, r3;
    uint32_t meta;
    unpack_refs(w, &r0, &r1, &r2, &r3, &meta);
    // the reference's visiting order (bvh.cpp:686-692 applied at P, L and R)
    const bool swap_p = (rc.neg_mask >> (meta & 3u)) & 1, swap_l = (rc.neg_mask >> ((meta >> 2) & 3u)) & 1,
               swap_r = (rc.neg_mask >> ((meta >> 4) & 3u)) & 1;
    const int a0r = swap_l ? r1 : r0, a1r = swap_l ? r0 : r1, b0r = swap_r ? r3 : r2, b1r = swap_r ? r2 : r3;
    const float a0k = swap_l ? k1 : k0, a1k = swap_l ? k0 : k1, b0k = swap_r ? k3 : k2, b1k = swap_r ? k2 : k3;
    const int e0r = swap_p ? b0r : a0r, e1r = swap_p ? b1r : a1r, e2r = swap_p ? a0r : b0r, e3r = swap_p ? a1r : b1r;
    const float e0k = swap_p ? b0k : a0k, e1k = swap_p ? b1k : a1k, e2k = swap_p ? a0k : b0k, e3k = swap_p ? a1k : b1k;
    const bool v0 = e0k < IILE_INF, v1 = e1k < IILE_INF, v2 = e2k < IILE_INF, v3 = e3k < IILE_INF;
    // defer everything behind the first visitable slot, farthest first
    if (v3 && (v0 || v1 || v2)) stack_push(t, sr, e3r, e3k);
    if (v2 && (v0 || v1)) stack_push(t, sr, e2r, e2k);
    if (v1 && v0) stack_push(t, sr, e1r, e1k);
    if (v0 || v1 || v2 || v3)
        t.cur = v0 ? e0r : (v1 ? e1r : (v2 ? e2r : e3r));
    else
        trav_pop<false>(t, sr, nullptr);
}
// The same step for any-hit rays (BVHAccel::IntersectP, bvh.cpp:702-738) in the uninstrumented kernels: whether SOME
// primitive is hit does not depend on the order the tree is walked in, and ray.tMax never shrinks, so the reference's
// near / far ordering (three dirIsNeg decisions and the selects that apply them to four refs and keys) is dropped:
// enter the first visitable slot, defer the rest as they come. Only the visit counters depend on the order, and the
// instrumented kernels keep the ordered binary walk.
DEV void trav_interior4_any(Trav &t, const StackRef &sr, const Wide4Planes &w) {
    float tmin[4], tmx[4];
    slab4(t.rc, w, tmin, tmx);
    auto visit = [&](int i) { return tmin[i] <= tmx[i] && tmx[i] > 0 && tmin[i] < t.tmax; };
    const bool v0 = visit(0), v1 = visit(1), v2 = visit(2), v3 = visit(3);
    int r0, r1, r2, r3;
    uint32_t meta_unused;
    unpack_refs(w, &r0, &r1, &r2, &r3, &meta_unused);
    // (the cached tMin of a deferred slot only feeds trav_pop's `tMin < ray.tMax`, already decided: any value below tMax)
    if (v3 && (v0 || v1 || v2)) stack_push(t, sr, r3, 0.f);
    if (v2 && (v0 || v1)) stack_push(t, sr, r2, 0.f);
    if (v1 && v0) stack_push(t, sr, r1, 0.f);
    if (v0 || v1 || v2 || v3)
        t.cur = v0 ? r0 : (v1 ? r1 : (v2 ? r2 : r3));
    else
        trav_pop<false>(t, sr, nullptr);
}
// One interior step of the uninstrumented kernels: the four-wide record, unless a lane of the
// wavefront carries a NaN-capable ray (or the scene's boxes are not nested, which a BVH built as
// bvh.cpp:236-402 builds it cannot produce; iile_scene_create checks).
template <bool ANY = false>
DEV void trav_interior_step_fast(const DScene &S, Trav &t, const StackRef &sr) {
    if (__builtin_expect(S.boxes_nested && __ballot(t.rc.neg_mask & 0x80) == 0, 1)) {
        if (ANY)   // an any-hit ray takes its children in record order (no near-first sort: any hit ends it)
            trav_interior4_any(t, sr, load_wide4<false>(S.wide4, t.cur, t.rc.neg_mask, sr.top));
        else
            trav_interior4(t, sr, load_wide4<true>(S.wide4, t.cur, t.rc.neg_mask, sr.top));
    } else {
        int g = t.cur < 0 ? 0 : t.cur;
        // a record of the LDS top carries its own index among the binary records behind its axes word
        if (sr.top != nullptr && g >= kTopFlag)
            g = int(*reinterpret_cast<__attribute__((address_space(3))) uint32_t *>(sr.top + uint32_t(g - kTopFlag) * uint32_t(kTopStride) + 116u));
        const float4 *w = S.wide + 4 * size_t(g);
        trav_interior<false>(t, sr, nullptr, w[0], w[1], w[2], w[3]);
    }
}
template <bool COUNT, bool ANY = false>
DEV void trav_step(const DScene &S, Trav &t, const StackRef &sr, TraceStats *st) {
    if (COUNT)
        trav_interior_step<true>(S, t, sr, st);
    else
        trav_interior_step_fast<ANY>(S, t, sr);
}

// screen-space derivatives of a hit's (u, v): SurfaceInteraction::dudx ... (interaction.h:127-128)
struct TexDiff {
    float dudx, dvdx, dudy, dvdy;
};
DEV F3 tex_image(const DScene &S, int tex, float u, float v, const TexDiff &td);  // defined with the textures below
// where a texture is evaluated: SurfaceInteraction's uv, p and their screen-space differentials (dpdx / dpdy: zero where the
// caller's (u, v) differentials are zero)
struct TexCtx {
    float u, v;
    TexDiff td;
    F3 p, dpdx, dpdy;
};

// The alpha test of Triangle::Intersect / IntersectP (triangle.cpp:325-331, 509-541) on a hit that passed the
// geometric test: isectLocal carries uvHit and zero differentials, so an ImageTexture<Float, Float> filters
// bilinearly at level 0. any_hit (IntersectP) also asks the shadow alpha mask.
DEV bool alpha_rejects(const DScene &S, int prim, uint32_t flags, float b0, float b1, float b2, bool any_hit) {
    float uv00 = 0, uv01 = 0, uv10 = 1, uv11 = 0, uv20 = 1, uv21 = 1;  // triangle.h:98-108
    if (flags & 4u) {
        const float2 *u = S.tri_uv + 3 * size_t(prim);
        const float2 a = u[0], b = u[1], c = u[2];
        uv00 = a.x, uv01 = a.y, uv10 = b.x, uv11 = b.y, uv20 = c.x, uv21 = c.y;
    }
    const float u = b0 * uv00 + b1 * uv10 + b2 * uv20, v = b0 * uv01 + b1 * uv11 + b2 * uv21;
    const int2 masks = S.prim_alpha[prim];
    const TexDiff zero = TexDiff{0, 0, 0, 0};
    if (masks.x == -2) return true;  // IILE_ALPHA_ZERO
    if (masks.x >= 0 && tex_image(S, masks.x, u, v, zero).x == 0) return true;
    if (any_hit) {
        if (masks.y == -2) return true;
        if (masks.y >= 0 && tex_image(S, masks.y, u, v, zero).x == 0) return true;
    }
    return false;
}

// ray_d: the float4 record holding the ray direction — only the (rare) sphere
// test needs it, so it is re-read there instead of living in registers.
// ALPHA: the rare build — some mesh of the scene has an alpha mask (vertex-record flag bit 12 marks its triangles), or the scene
// has disks or cylinders, or more than kFewSpheres spheres (DScene::rare_prims): only this build tests quadrics and bounds the
// turns of its shape test, so the common build stays as it was without them
template <bool COUNT, bool ALPHA = false>
DEV bool trav_leaf(const DScene &S, Trav &t, const StackRef &sr, TraceStats *st, const bool any_hit,
                   const float4 *ray_d) {
    int prim = t.cur < 0 ? ~t.cur : 0;  // clamped like trav_interior's index; tri_verts has one pad record
    bool last;
    do {
        // the primitive's three records in one round trip: the flag word (sphere? last of its leaf?) rides in the first one, and
        // waiting for it before asking for the other two made every leaf step two dependent trips to memory
        // (the room 474 -> 455 ms, killeroo 47.3 -> 46.7: profiles/r04_ab_traversal_scheduling.txt)
        float4 v0 = S.tri_verts[3 * size_t(prim)];
        float4 v1_ = S.tri_verts[3 * size_t(prim) + 1];
        float4 v2_ = S.tri_verts[3 * size_t(prim) + 2];
        asm volatile("" : "+v"(v0.w), "+v"(v1_.x), "+v"(v2_.x));  // (keeps the compiler from sinking the two loads behind the flag test)
        const uint32_t flags = f2b(v0.w);
        last = (flags & 16u) != 0;
        if (flags & 1u) {
            if (COUNT) ++st->spheres;
            float th;
            F3 od, ph;
            const float4 d4 = *ray_d;
            // the lanes that test the same sphere or quadric go together, its fields in SGPRs (uniform_entry): one turn of the
            // loop when the scene has one sphere and no quadric, which is the common case. prim_shape >= 0 is a sphere, ~index a
            // quadric (disk, cylinder): the kind is decided per turn, on the wave-uniform index
            const int sphere = (S.n_spheres == 1 && !(ALPHA && S.n_quadrics > 0)) ? 0 : S.prim_shape[prim];
            bool sphere_hit = false;
            if (ALPHA) {
                // the rare build takes two turns at the most, however many shapes the wavefront's lanes hold (a scene of many
                // small spheres or columns: up to 64 of them, and as many serial turns of the loop below). The first is the
                // loop's: the first lane's shape from SGPRs, for every lane that shares it. Whoever is left tests its own
                // shape in one pass, the record read through vector loads as the test asks for its fields; a sphere lane, a
                // disk lane and a cylinder lane may sit side by side. Same functions, same operations, same bits
                const int s_now = __builtin_amdgcn_readfirstlane(sphere);
                if (sphere == s_now) {
                    if (s_now < 0)
                        sphere_hit = quadric_test(uniform_entry(S.quadrics, ~s_now), t.rc.o(), F3{d4.x, d4.y, d4.z}, t.tmax, &th, &od, &ph);
                    else
                        sphere_hit = sphere_test(uniform_entry(S.spheres, s_now), t.rc.o(), F3{d4.x, d4.y, d4.z}, t.tmax, &th, &od, &ph);
                } else if (sphere < 0) {
                    sphere_hit = quadric_test(S.quadrics[~sphere], t.rc.o(), F3{d4.x, d4.y, d4.z}, t.tmax, &th, &od, &ph);
                } else {
                    sphere_hit = sphere_test(S.spheres[sphere], t.rc.o(), F3{d4.x, d4.y, d4.z}, t.tmax, &th, &od, &ph);
                }
            } else {
                // the common build: at most 8 spheres and no quadric (DScene::rare_prims), one turn per distinct sphere
                for (bool pending = true; pending;) {
                    const int s_now = __builtin_amdgcn_readfirstlane(sphere);
                    if (sphere == s_now) {
                        sphere_hit = sphere_test(uniform_entry(S.spheres, s_now), t.rc.o(), F3{d4.x, d4.y, d4.z}, t.tmax, &th, &od, &ph);
                        pending = false;
                    }
                }
            }
            if (sphere_hit) {
                if (any_hit) {
                    t.have = false;
                    return true;
                }
                t.tmax = th;
                t.hit_prim = prim | hit_tag(flags);
                t.b0 = t.b1 = t.b2 = 0;
            }
        } else {
            const float4 v1 = v1_, v2 = v2_;
            if (COUNT) ++st->tris;
            float th, b0, b1, b2;
            if (triangle_test(t.rc, t.tmax, F3{v0.x, v0.y, v0.z}, F3{v1.x, v1.y, v1.z}, F3{v2.x, v2.y, v2.z}, &th, &b0,
                              &b1, &b2) &&
                !(ALPHA && (flags & 4096u) && alpha_rejects(S, prim, flags, b0, b1, b2, any_hit))) {
                if (COUNT) ++st->tri_hits;
                if (any_hit) {
                    t.have = false;
                    return true;
                }
                t.tmax = th;
                t.hit_prim = prim | hit_tag(flags);
                t.b0 = b0;
                t.b1 = b1;
                t.b2 = b2;
            }
        }
        ++prim;
        // one primitive per step: the wavefront's next vote sees the lanes whose leaf goes on,
        // instead of every lane waiting for the longest leaf (most leaves hold one primitive)
        if (!last) {
            t.cur = ~prim;
            return false;
        }
    } while (!last);
    trav_pop<COUNT>(t, sr, st);
    return false;
}

// What the persistent kernels (k_extend / k_shadow / k_mis) share of their loop. A block's traversal storage — a stack ring per
// wavefront and the block's copy of the tree's top, staged here — and the calling lane's view of it; `spill` holds one HBM
// column per thread of the grid. BLOCK: threads per block.
template <bool COUNT, int BLOCK>
DEV StackRef trav_block_begin(const DScene &S, int *spill) {
    __shared__ int lds_stack[BLOCK / 64][2 * kLdsStackDepth][64];
    __shared__ __attribute__((aligned(16))) char lds_top[COUNT ? 16 : kMaxTop * kTopStride];
    StackRef sr{(lds_int *)&lds_stack[threadIdx.x >> 6][0][threadIdx.x & 63], spill, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK};
    sr.root = S.root_ref;
    if (!COUNT && S.n_top > 0) {  // the instrumented build walks the binary records: no four-wide steps, no top
        stage_top_records(S, (lds_char *)lds_top, int(threadIdx.x), BLOCK);
        __syncthreads();
        sr.top = (lds_char *)lds_top;
        sr.root = S.root_ref_top;
    }
    return sr;
}
// They take ONE step per iteration for the whole wavefront, interior or leaf, whichever has more lanes waiting: an interior
// step when interior lanes x kVoteNum >= leaf lanes x kVoteDen (leaf steps are the dearer ones).
constexpr int kVoteNum = 4, kVoteDen = 5;
// What a wave step reports: kind -1 nothing (no lane has a node to process), 0 an interior step, 1 a leaf step; the lanes that took
// it and those waiting at a node of the other kind; whether this lane's leaf step returned a hit (any_hit: the ray is occluded).
struct WaveStep { int kind, n_go, n_wait; bool hit; };
// `active`: the lane carries a ray; ANYORDER: the interior step may take the slots unordered (trav_interior4_any)
template <bool COUNT, bool ALPHA, bool ANYORDER>
DEV WaveStep trav_wave_step(const DScene &S, bool active, Trav &t, const StackRef &sr, TraceStats *st, bool any_hit, const float4 *ray_d) {
    const bool wi = active && t.have && t.cur >= 0;
    const bool wl = active && t.have && t.cur < 0;
    const int n_int = __popcll(__ballot(wi)), n_leaf = __popcll(__ballot(wl));
    if (n_int > 0 && n_int * kVoteNum >= n_leaf * kVoteDen) {
        if (wi) trav_step<COUNT, ANYORDER>(S, t, sr, st);
        return {0, n_int, n_leaf, false};
    }
    if (n_leaf == 0) return {-1, 0, 0, false};
    return {1, n_leaf, n_int, wl && trav_leaf<COUNT, ALPHA>(S, t, sr, st, any_hit, ray_d)};
}

// single-ray wrapper (kernel-level probes)
template <bool ANY_HIT, bool COUNT, bool ALPHA = true>
DEV bool traverse(const DScene &S, F3 ro, F3 rd, float tmax, lds_int *lds_stack, int *spill, uint32_t spill_stride,
                  HitRec *hit, TraceStats *st) {
    Trav t;
    StackRef sr{lds_stack, spill, 0u, spill_stride};
    sr.root = S.root_ref;
    const float4 d4 = make_float4(rd.x, rd.y, rd.z, 0.f);
    trav_begin<COUNT>(S, t, ro, rd, tmax, st, sr.root);
    while (t.have) {
        while (t.have && t.cur >= 0) trav_step<COUNT, ANY_HIT>(S, t, sr, st);
        if (t.have && trav_leaf<COUNT, ALPHA>(S, t, sr, st, ANY_HIT, &d4)) return true;
    }
    hit->prim = hit_index(t.hit_prim);
    hit->t = t.tmax;
    hit->b0 = t.b0;
    hit->b1 = t.b1;
    hit->b2 = t.b2;
    return t.hit_prim >= 0;
}
