// snk_contacts.hpp -- ground contacts of a cylinder, as far as both solves share them: the lowest rim point, the
// cylinder's world frame and friction directions, and Bullet's persistent manifold [U] (one cached point set per
// cylinder: update, overflow rule, its block in global memory, its place in the compact contact list).
#pragma once
#include "snk_lds.hpp"
#include "snk_model.hpp"
#include "snk_wave.hpp"

namespace snk {

constexpr int kMfFloats = 28;      // per cylinder: [count, 3 pad, 4 x (a3, b.x, b.y, lambda)]

// The wave-uniform model fields the contact functions read, fetched ONCE per call by scalar loads.  Such a function is
// called, not inlined: its model arrives as a generic reference in vector registers, and every read through it is a vector
// load of a wave-uniform value with a full wait behind it.  The model lives in constant or global memory and no kernel
// writes it, so its address -- made uniform -- may be read through the constant address space.  Only loads move: the
// arithmetic on these values is what it was.  Per-lane tables (cyl_R[c], cyl_c[c]) stay vector loads through M.
struct ContactK {
    float break_thr, margin, cyl_r, cyl_hl, cyl_zoff, aniso[3], fricB, warm_factor;
    int hull_sides, contact_model, self_collision, obstacle, warm_start, contact_order, support_serial;
};
typedef const DevModel __attribute__((address_space(4))) * ModelConstPtr;
__device__ __forceinline__ ModelConstPtr model_const(const DevModel& M) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(&M);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return (ModelConstPtr)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ ContactK contact_k(const DevModel& M) {
    const ModelConstPtr C = model_const(M);
    ContactK K;
    K.break_thr = C->break_thr; K.margin = C->margin; K.cyl_r = C->cyl_r; K.cyl_hl = C->cyl_hl; K.cyl_zoff = C->cyl_zoff;
    K.aniso[0] = C->aniso[0]; K.aniso[1] = C->aniso[1]; K.aniso[2] = C->aniso[2];
    K.fricB = C->fricB; K.warm_factor = C->warm_factor;
    K.hull_sides = C->hull_sides; K.contact_model = C->contact_model; K.self_collision = C->self_collision;
    K.obstacle = C->obstacle; K.warm_start = C->warm_start; K.contact_order = C->contact_order;
    K.support_serial = C->support_serial;
    return K;
}

// The hull's vertex table in the lanes of two registers: lane k holds hull_xy[(k >> 1) & 31], both floats, from ONE
// coalesced load.  Call it with every lane of the wave active: hull_support reads lanes that sit out the search itself.
struct HullLanes {
    float x, y;
};
__device__ __forceinline__ HullLanes hull_lanes(const DevModel& M, int lane) {
    typedef float hl_v2 __attribute__((ext_vector_type(2)));
    typedef const hl_v2 __attribute__((address_space(4))) * TablePtr;
    const hl_v2 v = ((TablePtr)&model_const(M)->hull_xy[0][0])[(lane >> 1) & 31];
    HullLanes H = {v.x, v.y};
    // The two registers are pinned HERE, where every lane is active.  Their only reader sits inside the callers'
    // `if (lane < 2 N)`, and a load whose only use is in a later block may be sunk into it: executed by the lower lanes
    // alone, it left vertices 16..31 of the 16-link streamed-row kernels unloaded (the first build of this function:
    // 24 contacts for a snake lying flat on 32 cylinders).  The price is that the load's round trip is waited for here.
    asm volatile("" : "+v"(H.x), "+v"(H.y));
    return H;
}
__device__ __forceinline__ float lane_value(float v, int l) {       // v of lane l (wave-uniform l), whatever EXEC says
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
// Support vertex of the hull towards dl: the FIRST maximum of dot(dl, c) over the candidates in the importer's order,
//   CAPS   c = (vertex s, +hl), (vertex s, -hl) for s = 0, 1, ...: the prism's 2 * sides vertices (manifold_core)
//   !CAPS  c = vertex s: the polygon's (rim_point; z of the result is 0)
// the value it replaces came from a loop with one load of hull_xy per candidate and a divergent block on a new best
// (SNK_SUPPORT_SERIAL=1 keeps those loops: tests/test_gpu_support_vertex.py holds the two against each other, bit for
// bit).  Here vertex s comes out of the lanes (v_readlane, uniform index), and everything else is a select.  What is
// kept, so that the bits are: the order k ascending; the start value, the strict >, so the first maximum wins and a NaN
// changes nothing (the comparison is false); and the arithmetic tree the compiler made of dot(dl, c) there --
//   t = dl.x * vx;  t = fma(dl.y, vy, t);  val = fma(dl.z, +-hl, t)       (rim_point: val = fma(dl.y, vy, dl.x * vx))
// read off the parent's ISA (v_mul, v_fma, v_fma, with dl's negations of Rw's third row folded into operand modifiers,
// which is exact) and spelled out under contract(off).  The first two steps do not depend on the sign of hl: they are
// computed once per vertex for its two candidates, the same operations on the same operands.
template <bool CAPS>
__device__ __forceinline__ f3 hull_support(const HullLanes& H, int sides, f3 dl, float hl) {
#pragma clang fp contract(off)
    float best = -3.0e38f;
    f3 sv = mk3(0.f, 0.f, 0.f);
    for (int s = 0; s < sides; s++) {
        const float vx = lane_value(H.x, 2 * s), vy = lane_value(H.y, 2 * s);
        const float t = __builtin_fmaf(dl.y, vy, dl.x * vx);
        if (CAPS) {
            const float vp = __builtin_fmaf(dl.z, hl, t);
            const bool gp = vp > best;
            best = gp ? vp : best;
            const float vm = __builtin_fmaf(dl.z, -hl, t);
            const bool gm = vm > best;
            best = gm ? vm : best;
            sv.x = (gp || gm) ? vx : sv.x;
            sv.y = (gp || gm) ? vy : sv.y;
            sv.z = gm ? -hl : (gp ? hl : sv.z);
        } else {
            const bool g = t > best;
            best = g ? t : best;
            sv.x = g ? vx : sv.x;
            sv.y = g ? vy : sv.y;
        }
    }
    return sv;
}

// lowest rim point (x, y in the cylinder's frame) towards dl = world "down" in that frame
__device__ __forceinline__ void rim_point(const DevModel& M, const ContactK& K, const HullLanes& H, f3 dl, float& lx, float& ly) {
    lx = 0.f; ly = 0.f;
    if (K.hull_sides > 0) {
        if (K.support_serial) {
            float best = -3.0e38f;
            for (int s = 0; s < K.hull_sides; s++) {          // first maximum, the importer's vertex order
                const float vx = M.hull_xy[s][0], vy = M.hull_xy[s][1];
                const float val = dl.x * vx + dl.y * vy;
                if (val > best) { best = val; lx = vx; ly = vy; }
            }
        } else {
            const f3 sv = hull_support<false>(H, K.hull_sides, dl, 0.f);
            lx = sv.x; ly = sv.y;
        }
    } else {
        const float rr = sqrtf(dl.x * dl.x + dl.y * dl.y);
        if (rr > 1e-12f) { lx = K.cyl_r * dl.x / rr; ly = K.cyl_r * dl.y / rr; }
    }
}
// world rotation of cylinder c's frame
__device__ __forceinline__ void cyl_world_rot(const float* Rb, const float* Rc, float* Rw) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            Rw[3 * i + j] = Rb[3 * i] * Rc[j] + Rb[3 * i + 1] * Rc[3 + j] + Rb[3 * i + 2] * Rc[6 + j];
}
// friction directions (0,-1,0), (1,0,0) scaled anisotropically in the link's axes: d' = Rw diag(aniso) Rw^T d
template <class MK>      // (DevModel, or the contact functions' ContactK)
__device__ __forceinline__ void friction_dirs(const MK& M, const float* Rw, f3& dA, f3& dB) {
    const f3 a = mk3(M.aniso[0], M.aniso[1], M.aniso[2]);
    const f3 l1 = mulRtv(Rw, mk3(0.f, -1.f, 0.f));
    const f3 l2 = mulRtv(Rw, mk3(1.f, 0.f, 0.f));
    dA = mulRv(Rw, mk3(l1.x * a.x, l1.y * a.y, l1.z * a.z));
    // friction_directions 1: the second tangent is a zero vector -- its row comes out J = 0, M^-1 J^T = 0, den = 0 and
    // resolves to nothing in either friction form (the cone over (x, 0) is the box bound of the one row)
    dB = mulRv(Rw, mk3(l2.x * a.x, l2.y * a.y, l2.z * a.z)) * M.fricB;
}

// One cached manifold point: the point on the link in the LINK's coordinates (cylinder frame + cyl_zoff along z),
// the point on the ground in world coordinates (z = 0: the plane's), the refreshed distance, and the normal impulse
// the point carried in the last substep (btManifoldPoint::m_appliedImpulse [U]; warm starting reads it).
struct MPt {
    f3 a, b;
    float d, lam;
};
typedef float mf_v4 __attribute__((ext_vector_type(4)));
// dst = c ? src : dst, field by field.  (A conditional struct assignment inside an unrolled `if (j == where)` chain gets
// its stores merged into ONE store at a computed address, which puts the whole point cache into scratch memory: ~100
// scratch round trips per substep, measured in the ISA of round 3's first build.)
__device__ __forceinline__ void mpt_sel(MPt& dst, const MPt& src, bool c) {
    dst.a.x = c ? src.a.x : dst.a.x; dst.a.y = c ? src.a.y : dst.a.y; dst.a.z = c ? src.a.z : dst.a.z;
    dst.b.x = c ? src.b.x : dst.b.x; dst.b.y = c ? src.b.y : dst.b.y; dst.b.z = c ? src.b.z : dst.b.z;
    dst.d = c ? src.d : dst.d; dst.lam = c ? src.lam : dst.lam;
}
__device__ __forceinline__ void f3_sel(f3& dst, f3 src, bool c) {
    dst.x = c ? src.x : dst.x; dst.y = c ? src.y : dst.y; dst.z = c ? src.z : dst.z;
}

// btPersistentManifold::sortCachedPoints with gContactCalcArea3Points [U]: which cached point the new one replaces
__device__ __forceinline__ int manifold_sort_cached(const MPt (&p)[4], const MPt& np) {
    int mpi = -1;
    float mp = np.d;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (p[i].d < mp) { mpi = i; mp = p[i].d; }
    auto area = [](f3 a1, f3 a0, f3 b1, f3 b0) { const f3 c = cross(a1 - a0, b1 - b0); return dot(c, c); };
    float res[4] = {0.f, 0.f, 0.f, 0.f};
    if (mpi != 0) res[0] = area(np.a, p[1].a, p[3].a, p[2].a);
    if (mpi != 1) res[1] = area(np.a, p[0].a, p[3].a, p[2].a);
    if (mpi != 2) res[2] = area(np.a, p[0].a, p[3].a, p[1].a);
    if (mpi != 3) res[3] = area(np.a, p[0].a, p[2].a, p[1].a);
    int best = 0;
    float bv = fabsf(res[0]);
#pragma unroll
    for (int i = 1; i < 4; i++)
        if (fabsf(res[i]) > bv) { bv = fabsf(res[i]); best = i; }
    return best;
}

// The manifold of this lane's cylinder (n cached points p[0 .. n-1], registers), updated for the current pose -- see
// the oracle's find_contacts_manifold for the Bullet calls restated: a link's collider is a btCompoundShape, so
// btCompoundCollisionAlgorithm first REFRESHES the child's manifold from the new pose (positions, distances, and the
// removal of points that lifted off or drifted: refreshContactPoints), then the child's convex-plane algorithm adds
// this step's support point (getCacheEntry / replaceContactPoint / addManifoldPoint with sortCachedPoints, which sees
// the refreshed distances) [U].  Returns the new number of cached points; their world positions on the link and
// distances in wa / p[].d.  Everything is a select (mpt_sel): the cache stays in registers.
__device__ __forceinline__ int manifold_core(const DevModel& M, const ContactK& K, const HullLanes& H, int n, MPt (&p)[4],
                                             const float* Rw, f3 centre, f3 dl, f3 (&wa)[4] SNK_PROF_F_PARAM) {
    n = n < 0 ? 0 : (n > 4 ? 4 : n);
    const float thr = K.break_thr;
    const f3 zoff = mk3(0.f, 0.f, K.cyl_zoff);
    // refresh from the current pose, then drop what lifted off or drifted (last to first, the last one moves in)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        wa[j] = centre + mulRv(Rw, p[j].a - zoff);
        p[j].d = wa[j].z - p[j].b.z;
    }
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        bool drop = !(p[j].d <= thr);
        {
            const float dx = p[j].b.x - wa[j].x, dy = p[j].b.y - wa[j].y, dz = p[j].b.z - (wa[j].z - p[j].d);
            drop = drop || (dx * dx + dy * dy + dz * dz > thr * thr);
        }
        drop = drop && j < n;
        const int last = n - 1;
        MPt pl = p[0];
        f3 wl = wa[0];
#pragma unroll
        for (int k = 1; k < 4; k++) { mpt_sel(pl, p[k], k == last); f3_sel(wl, wa[k], k == last); }
        mpt_sel(p[j], pl, drop && j != last);
        f3_sel(wa[j], wl, drop && j != last);
        n = drop ? n - 1 : n;
    }
    SNK_FSTAMP(10)
    // the new point: support vertex towards the plane (+ margin along that direction)
    f3 sv;
    if (K.hull_sides > 0) {
        if (K.support_serial) {
            float best = -3.0e38f;
            sv = mk3(0.f, 0.f, 0.f);
            for (int k = 0; k < 2 * K.hull_sides; k++) {      // the importer's order: (+z, -z) of vertex 0, 1, ...
                const f3 c = mk3(M.hull_xy[k >> 1][0], M.hull_xy[k >> 1][1], (k & 1) ? -K.cyl_hl : K.cyl_hl);
                const float val = dot(dl, c);
                if (val > best) { best = val; sv = c; }
            }
        } else {
            sv = hull_support<true>(H, K.hull_sides, dl, K.cyl_hl);
        }
    } else {                                              // btCylinderShapeZ's support function [U]
        const float rr = sqrtf(dl.x * dl.x + dl.y * dl.y);
        sv = rr != 0.f ? mk3(K.cyl_r * dl.x / rr, K.cyl_r * dl.y / rr, 0.f) : mk3(K.cyl_r, 0.f, 0.f);
        sv.z = dl.z < 0.f ? -K.cyl_hl : K.cyl_hl;
    }
    SNK_FSTAMP(11)
    MPt np;
    const f3 loc = sv + dl * K.margin;                    // in the cylinder's own (centred) frame
    np.a = loc + zoff;
    const f3 wnew = centre + mulRv(Rw, loc);
    np.d = wnew.z;
    np.b = mk3(wnew.x, wnew.y, 0.f);
    np.lam = 0.f;
    {
        const bool add = np.d < thr;
        int nearest = -1;
        float shortest = thr * thr;
        float lam_near = 0.f;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const f3 d = p[j].a - np.a;
            const float dd = dot(d, d);
            const bool nr = j < n && dd < shortest;
            shortest = nr ? dd : shortest; nearest = nr ? j : nearest; lam_near = nr ? p[j].lam : lam_near;
        }
        const int evict = manifold_sort_cached(p, np);
        // replaceContactPoint keeps the cached point's applied impulse; a point that is added, or that evicts another
        // one (addManifoldPoint -> sortCachedPoints), starts at zero [U]
        np.lam = nearest >= 0 ? lam_near : 0.f;
        const int where = nearest >= 0 ? nearest : (n < 4 ? n : evict);
        n = (add && nearest < 0 && n < 4) ? n + 1 : n;
#pragma unroll
        for (int j = 0; j < 4; j++) { mpt_sel(p[j], np, add && j == where); f3_sel(wa[j], wnew, add && j == where); }
    }
    SNK_FSTAMP(12)
    return n;
}

// Which of a cylinder's n cached points get rows when the environment holds more points than the solve has slots for
// (`room` of them; Bullet has no such limit, snk_contact_overflow counts how often this build's is hit).  Every cylinder
// ranks its points the way Bullet's own manifold reduction values them (sortCachedPoints: the deepest point, then
// spread): first the deepest, second the one farthest from it (the other end cap), third the one that spans the
// larger triangle with those two, then the last; ties go to the lower manifold index.  Slots are handed out in
// passes: every cylinder's first point, in cylinder order, then every cylinder's second, ... until they are used up,
// so a resting snake keeps one point per end cap of every cylinder before any cylinder keeps a third.  Lane =
// cylinder; returns the lane's bit mask of kept points (the oracle's max_contacts mirrors the rule for the tests).
__device__ __forceinline__ int manifold_keep_mask(int n, const MPt (&p)[4], int lane, int total, int room) {
    if (total <= room) return (1 << n) - 1;
    int rank[4] = {4, 4, 4, 4};
    int p0 = 0, p1 = -1, p2 = -1;
    {
        float best = 3.0e38f;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (i < n && p[i].d < best) { best = p[i].d; p0 = i; }
    }
    f3 a0 = p[0].a;
#pragma unroll
    for (int i = 1; i < 4; i++) f3_sel(a0, p[i].a, i == p0);
    {
        float best = -1.f;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const f3 d = p[i].a - a0;
            const float dd = dot(d, d);
            if (i < n && i != p0 && dd > best) { best = dd; p1 = i; }
        }
    }
    f3 a1 = p[0].a;
#pragma unroll
    for (int i = 1; i < 4; i++) f3_sel(a1, p[i].a, i == p1);
    {
        float best = -1.f;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const f3 c = cross(a1 - a0, p[i].a - a0);
            const float cc = dot(c, c);
            if (i < n && i != p0 && i != p1 && cc > best) { best = cc; p2 = i; }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) rank[i] = i == p0 ? 0 : (i == p1 ? 1 : (i == p2 ? 2 : 3));
    int granted = 0;                       // passes in which this cylinder got a slot (monotone: once refused, refused)
    int left = room;
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
        const unsigned long long el = __ballot(n > pass);
        const int before = __popcll(el & ((1ull << lane) - 1ull));
        if (n > pass && before < left) granted = pass + 1;
        left -= __popcll(el);
        left = left < 0 ? 0 : left;
    }
    int mask = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (i < n && rank[i] < granted) mask |= 1 << i;
    return mask;
}

// The streamed-row kernels keep the manifolds in global memory: mfc -> the cylinder's kMfFloats floats
// [count, 3 pad, 4 x (a3, b.x, b.y, lambda)], read and written write-through (sc1): an env-step moves between waves at
// substep boundaries, and the bytes must be where the next wave's loads look (same rule as the state record,
// store_rec_through).
__device__ __forceinline__ int manifold_load_global(const float* __restrict__ mfc, MPt (&p)[4]) {
    mf_v4 v[7];
    asm volatile(
        "global_load_dwordx4 %0, %7, off sc1\n\t"
        "global_load_dwordx4 %1, %7, off offset:16 sc1\n\t"
        "global_load_dwordx4 %2, %7, off offset:32 sc1\n\t"
        "global_load_dwordx4 %3, %7, off offset:48 sc1\n\t"
        "global_load_dwordx4 %4, %7, off offset:64 sc1\n\t"
        "global_load_dwordx4 %5, %7, off offset:80 sc1\n\t"
        "global_load_dwordx4 %6, %7, off offset:96 sc1\n\t"
        "s_waitcnt vmcnt(0)"
        : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6])
        : "v"(mfc)
        : "memory");
    float f[kMfFloats];
#pragma unroll
    for (int i = 0; i < 7; i++) { f[4 * i] = v[i].x; f[4 * i + 1] = v[i].y; f[4 * i + 2] = v[i].z; f[4 * i + 3] = v[i].w; }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        p[j].a = mk3(f[4 + 6 * j], f[5 + 6 * j], f[6 + 6 * j]);
        p[j].b = mk3(f[7 + 6 * j], f[8 + 6 * j], 0.f);
        p[j].lam = f[9 + 6 * j];
        p[j].d = 0.f;
    }
    const int n = (int)f[0];
    return n < 0 ? 0 : (n > 4 ? 4 : n);      // (manifold_core clamps as well; the count indexes registers here)
}
__device__ __forceinline__ void manifold_store_global(float* __restrict__ mfc, int n, const MPt (&p)[4]) {
    mf_v4 v[7];
    float f[kMfFloats];
    f[0] = (float)n; f[1] = 0.f; f[2] = 0.f; f[3] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        f[4 + 6 * j] = p[j].a.x; f[5 + 6 * j] = p[j].a.y; f[6 + 6 * j] = p[j].a.z;
        f[7 + 6 * j] = p[j].b.x; f[8 + 6 * j] = p[j].b.y; f[9 + 6 * j] = p[j].lam;
    }
#pragma unroll
    for (int i = 0; i < 7; i++) { v[i].x = f[4 * i]; v[i].y = f[4 * i + 1]; v[i].z = f[4 * i + 2]; v[i].w = f[4 * i + 3]; }
    asm volatile(
        "global_store_dwordx4 %7, %0, off sc1\n\t"
        "global_store_dwordx4 %7, %1, off offset:16 sc1\n\t"
        "global_store_dwordx4 %7, %2, off offset:32 sc1\n\t"
        "global_store_dwordx4 %7, %3, off offset:48 sc1\n\t"
        "global_store_dwordx4 %7, %4, off offset:64 sc1\n\t"
        "global_store_dwordx4 %7, %5, off offset:80 sc1\n\t"
        "global_store_dwordx4 %7, %6, off offset:96 sc1"
        :
        : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(mfc)
        : "memory");
}

// exclusive prefix sum over lanes of a small count (0..7), wave-uniform total in `total`
__device__ __forceinline__ int lane_prefix3(int cnt, int lane, int& total) {
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long b0 = __ballot(cnt & 1), b1 = __ballot(cnt & 2), b2 = __ballot(cnt & 4);
    total = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
    return __popcll(b0 & below) + 2 * __popcll(b1 & below) + 4 * __popcll(b2 & below);
}

// Where cylinder `lane`'s points start in the compact contact list: the exclusive prefix of the kept counts in the ORDER THE
// SOLVER SWEEPS THE MANIFOLDS (snk_params::contact_order; 0 = cylinder = link order, the prefix over the lanes as they are).
// Otherwise position r fetches the count of the cylinder that sits there (DevModel::cyl_at), the prefix runs over
// positions, and every cylinder fetches its own from its position (cyl_rank): two ds_bpermute per substep.
// (wave-uniform branch: the model sits in constant memory)
__device__ __forceinline__ int manifold_base(const DevModel& M, const ContactK& K, int ncyl, int kept, int lane, int& total) {
    if (K.contact_order == 0) return lane_prefix3(kept, lane, total);
    const int at = lane < ncyl ? (int)M.cyl_at[lane] : lane;
    const int rk = lane < ncyl ? (int)M.cyl_rank[lane] : lane;
    const int kept_r = __shfl(kept, at);
    const int base_r = lane_prefix3(kept_r, lane, total);
    return __shfl(base_r, rk);
}

}  // namespace snk
