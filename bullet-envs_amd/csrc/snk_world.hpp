// snk_world.hpp -- device parts of the tensor seam that are not step arithmetic (include/snk.h: snk_link_states,
// snk_contacts, snk_copy_envs, snk_closest_points): the per-link read-out of the unmerged URDF tree, the contact cache as
// contact records, the env-to-env copy of the simulator state, and the narrow phase of the link-box and link-link pairs as
// a query.
// Only snk_world.hip includes this: the step kernels' code object (snk_api.hip) has none of it.
#pragma once
#include <hip/hip_runtime.h>

#include "snk_query.hpp"
#include "snk_selfcol.hpp"

namespace snk {

// One output row = 16 floats (64 bytes): [COM 3 | quaternion xyzw 4 | link-frame origin 3 | COM velocity 3 | omega 3]
constexpr int kLinkStateFloats = 16;
// The staging image of one pass: float j of the pass's row l at stage[j][l] (snk_query.hpp: store_rows_as_quads)
constexpr int kStageStride = 66;

// world orientation of a link from its rotation matrix (row-major, link -> world): the branch of the largest of
// (trace, m00, m11, m22) -- Shepperd's rule, no cancellation in the square root --, normalised, signed so that w >= 0
__device__ __forceinline__ void quat_of(const float* m, float* q) {
    const float tr = m[0] + m[4] + m[8];
    float x, y, z, w;
    if (tr >= m[0] && tr >= m[4] && tr >= m[8]) {
        w = 1.f + tr; x = m[7] - m[5]; y = m[2] - m[6]; z = m[3] - m[1];
    } else if (m[0] >= m[4] && m[0] >= m[8]) {
        x = 1.f + m[0] - m[4] - m[8]; w = m[7] - m[5]; y = m[1] + m[3]; z = m[2] + m[6];
    } else if (m[4] >= m[8]) {
        y = 1.f - m[0] + m[4] - m[8]; w = m[2] - m[6]; x = m[1] + m[3]; z = m[5] + m[7];
    } else {
        z = 1.f - m[0] - m[4] + m[8]; w = m[3] - m[1]; x = m[2] + m[6]; y = m[5] + m[7];
    }
    float s = 1.0f / sqrtf(x * x + y * y + z * z + w * w);
    if (w < 0.f) s = -s;
    q[0] = x * s; q[1] = y * s; q[2] = z * s; q[3] = w * s;
}

// ----------------------------------------------------------------------------------
// link_state_kernel: one wave per output row block (one env id).  The env's record -> forward kinematics and body
// twists (as obs_kernel does) -> lane = link, in passes of 64 (3n + 2 = 50 links for 16 modules: one pass; 98 for 32: two).
// A pass's rows are staged in LDS and leave as consecutive float4s: a wave-wide store instruction writes 1 KB of
// consecutive bytes, every 128-byte line whole.  Plain loads; nothing of the handle's state is written.
// ----------------------------------------------------------------------------------
template <int N, bool V2>
__global__ __launch_bounds__(64) void link_state_kernel(const DevModel* __restrict__ Mp, const float* __restrict__ recs,
                                                        const float* __restrict__ links,
                                                        const int32_t* __restrict__ env_ids, float* __restrict__ out,
                                                        int n_rows, int n_envs) {
    using LT = Lds<N, V2>;
    constexpr int LR = 3 * N + 2;
    __shared__ float4 smem_raw[(sizeof(LT) + 15) / 16];
    __shared__ float stage[kLinkStateFloats][kStageStride];
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    const DevModel& M = *Mp;
    const int lane = threadIdx.x;
    for (int blk = blockIdx.x; blk < n_rows; blk += gridDim.x) {
        int env;
        const bool known = load_row_env(L, M, recs, env_ids, blk, n_envs, lane, env);      // (not known: its rows are zeros)
        float4* dst = reinterpret_cast<float4*>(out + (size_t)blk * LR * kLinkStateFloats);
#pragma unroll 1
        for (int r0 = 0; r0 < LR; r0 += 64) {
            const int r = r0 + lane;
            float v[kLinkStateFloats];
#pragma unroll
            for (int j = 0; j < kLinkStateFloats; j++) v[j] = 0.f;
            if (known && r == 0) {
                // the root is the record itself: position, quaternion, omega and velocity verbatim (snk_get_state's bits)
                const float* bs = L.base();
#pragma unroll
                for (int j = 0; j < 7; j++) v[j] = bs[j];
#pragma unroll
                for (int j = 0; j < 3; j++) { v[7 + j] = bs[j]; v[10 + j] = bs[10 + j]; v[13 + j] = bs[7 + j]; }
            } else if (known && r < LR) {
                float Rw[9];
                f3 ow, cw;
                const int b = link_row_frame(L, links + (size_t)r * kLinkFloats, Rw, ow, cw);
                const f3 ob = ld3(L.o[b]);
                // the body's twist at its joint origin carries the joint's own rate: v(COM) = v(o_b) + omega x (c - o_b)
                const f3 w = ld3(L.w[b]);
                const f3 vc = ld3(L.v[b]) + cross(w, cw - ob);
                st3(v, cw); quat_of(Rw, v + 3); st3(v + 7, ow); st3(v + 10, vc); st3(v + 13, w);
            }
#pragma unroll
            for (int j = 0; j < kLinkStateFloats; j++) stage[j][lane] = v[j];
            lds_sync();
            // = store_rows_as_quads<64>(stage, dst + 4 r0, rows of this pass, lane), written out: through the call the 16-link
            // kernels form the destination in two more vector registers and measured 0.5 to 4 % slower
            const int quads = (LR - r0 < 64 ? LR - r0 : 64) * (kLinkStateFloats / 4);
#pragma unroll
            for (int k = 0; k < kLinkStateFloats / 4; k++) {
                const int Q = 64 * k + lane;
                if (Q < quads) {
                    const int row = Q >> 2, f0 = 4 * (Q & 3);
                    dst[(size_t)r0 * (kLinkStateFloats / 4) + Q] =
                        make_float4(stage[f0][row], stage[f0 + 1][row], stage[f0 + 2][row], stage[f0 + 3][row]);
                }
            }
            lds_sync();      // (the stage and the record are read by every lane above: the next pass / env waits for them)
        }
    }
}

// ----------------------------------------------------------------------------------
// contacts_kernel: the contact cache as contact records (include/snk.h, "The reported contacts": that text is the
// contract).  One wave per output row (one env id).  The env's record -> forward kinematics -> lane = contact unit, in
// passes of 64: unit u < 2N is cylinder u, unit 2N the free box (16 links: lane 32 of the one pass; 32 links: lane 0 of a
// second pass).  A lane loads its unit's cache as whole float4s, forms its four 16-float records with selects, and
// stages them in LDS; a pass's records then leave as consecutive float4s, a wave-wide store instruction writing 1 KB of
// consecutive bytes.  Plain stores, no atomics; nothing of the handle's state is written.
// ----------------------------------------------------------------------------------
constexpr int kContactFloats = 16;
// the staging image: unit l's four records = 16 quads at stage[l][0 .. 15]; the 17th quad keeps the units' rows apart
constexpr int kContactStageQuads = 4 * kContactFloats / 4 + 1;

template <int N, bool V2>
__global__ __launch_bounds__(64) void contacts_kernel(const DevModel* __restrict__ Mp, const float* __restrict__ recs,
                                                      const float* __restrict__ mf_all, const float* __restrict__ box_all,
                                                      const int32_t* __restrict__ env_ids, float* __restrict__ points,
                                                      float* __restrict__ force, int32_t* __restrict__ count, int n_rows,
                                                      int n_envs) {
    using LT = Lds<N, V2>;
    constexpr int NC = 2 * N;                      // cylinders; unit NC is the box
    __shared__ float4 smem_raw[(sizeof(LT) + 15) / 16];
    __shared__ float4 stage[64][kContactStageQuads];
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    const DevModel& M = *Mp;
    const int lane = threadIdx.x;
    const int units = NC + (box_all ? 1 : 0);      // units with slots; force has NC + 1 entries either way
    for (int blk = blockIdx.x; blk < n_rows; blk += gridDim.x) {
        int env;
        const bool known = load_row_env(L, M, recs, env_ids, blk, n_envs, lane, env);      // (not known: its outputs are zeros)
        float4* dst = points ? reinterpret_cast<float4*>(points + (size_t)blk * units * 4 * kContactFloats) : nullptr;
        float live_total = 0.f;
#pragma unroll 1
        for (int u0 = 0; u0 <= NC; u0 += 64) {
            const int u = u0 + lane;
            // the unit's frame (R, origin), the offset its cached points are kept with, its count and its four points
            float R[9];
            f3 org = mk3(0.f, 0.f, 0.f);
            float zo = 0.f;
            int n = 0;
            MPt p[4];
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = 0.f;
#pragma unroll
            for (int j = 0; j < 4; j++) { p[j].a = mk3(0.f, 0.f, 0.f); p[j].b = mk3(0.f, 0.f, 0.f); p[j].d = 0.f; p[j].lam = 0.f; }
            if (known && u < NC) {
                org = cyl_frame(L, M, u, R);
                zo = M.cyl_zoff;
                n = manifold_load_global(mf_all + ((size_t)env * NC + u) * kMfFloats, p);
            } else if (known && u == NC && box_all) {
                box_pose(box_all, env, org, R);
                n = box_manifold(box_all, env, p);
            }
            const f3 zoff = mk3(0.f, 0.f, zo);
            float fsum = 0.f;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool on = j < n;
                const f3 w = org + mulRv(R, p[j].a - zoff);
                const float newton = p[j].lam / M.dt;
                fsum += on ? newton : 0.f;
                stage[lane][4 * j + 0] = make_float4(on ? w.x : 0.f, on ? w.y : 0.f, on ? w.z : 0.f, on ? p[j].b.x : 0.f);
                stage[lane][4 * j + 1] = make_float4(on ? p[j].b.y : 0.f, 0.f, 0.f, 0.f);
                stage[lane][4 * j + 2] = make_float4(on ? 1.f : 0.f, on ? w.z - 0.f : 0.f, on ? newton : 0.f, on ? p[j].lam : 0.f);
                stage[lane][4 * j + 3] = make_float4(on ? (float)u : 0.f, on ? (float)j : 0.f, on ? 1.f : 0.f, 0.f);
            }
            live_total += wave_sum<64>((float)n);
            if (force && u <= NC) force[(size_t)blk * (NC + 1) + u] = fsum;
            lds_sync();
            if (dst) {
                const int quads = ((units - u0 < 64) ? units - u0 : 64) * kContactFloats;      // 16 quads per unit
                for (int k = 0; 64 * k < quads; k++) {
                    const int Q = 64 * k + lane;
                    if (Q < quads) dst[(size_t)u0 * kContactFloats + Q] = stage[Q >> 4][Q & 15];
                }
            }
            lds_sync();      // (the stage and the record are read by every lane above: the next pass / env waits for them)
        }
        if (count && lane == 0) count[blk] = (int)live_total;
    }
}

// ----------------------------------------------------------------------------------
// closest_points_kernel: the narrow phase of snk_selfcol.hpp as a query (include/snk.h, "The closest points": that text is
// the contract).  One wave per output row (one env id).  The env's record -> forward kinematics -> lane = cylinder forms
// its world frame once and stages it in LDS (64 cylinders fill the wave at 32 links), then
//   box pairs    lane = cylinder, one pass: bounding spheres, the separating-axis cull, the tiers of GJK; slot c is dense
//   link pairs   (a) cull: lane = a, pass = offset b - a = 2, 3, ...; the survivors are appended to a list in LDS by
//                ballot and prefix popcount, which keeps the solver's (b - a, a) order without a sort;
//                (b) narrow phase: lane = candidate, 64 at a time, so the GJK runs on full waves whether one offset
//                passed the cull with two lanes or with sixty; the hits are compacted by ballot again.
// The work per env ranges from nothing (no pair passes the cull) to C(2n, 2) - (2n - 1) runs of GJK (a distance beyond the
// snake's length); the list holds every pair.  Found records are staged in LDS (float j of record r at stage[j][r]:
// snk_query.hpp, store_rows_as_quads) and leave 64 at a time as consecutive float4s -- a record that waits for
// its 64 stays staged, so every store instruction but an env's last writes 4 KB whole.  The per-cylinder minimum of the
// link-link distances is an integer minimum in LDS over an order-preserving key (any order of arrival gives the same
// bits); the running counts are wave-uniform.  Plain stores; no atomics to global memory; nothing of the handle's state
// is written.
// ----------------------------------------------------------------------------------
constexpr int kClosestStageRows = 128;         // up to 63 records waiting + the 64 of a chunk
constexpr int kClosestStageStride = 130;
__host__ __device__ constexpr int link_pairs_of(int ncyl) { return ncyl * (ncyl - 1) / 2 - (ncyl - 1); }

struct Closest {
    f3 P, PB, n;
    float dist;
    int tier;
};
// A shape as the kernel stages it in LDS: the Cvx itself and one float, so that lane = cylinder strides by an odd count.
// gjk_distance is out of line and takes its shapes and its witness points by reference: referred to where they lie in LDS
// they cost nothing, while references to a caller's registers would put them in scratch memory.
struct CvxSlot {
    Cvx s;
    float pad;
};
static_assert(sizeof(CvxSlot) == 17 * sizeof(float), "an odd stride");
struct Witness {
    f3 pa, pb;
    float pad;
};
// gjk_distance of snk_selfcol.hpp run further, for the implicit cylinder (hull_sides 0) alone: the same loop over the same
// simplex code, to a relative duality gap of 1e-6 within 40 steps where the solver's stops at 1e-5 within 32.  On a smooth
// surface GJK converges linearly and its answer carries the termination tolerance: the solver's choice leaves the
// DISTANCE good to 1e-7 m, all its rows need, but the NORMAL good to sqrt(1e-5) of a radian only (90th percentile 4.0e-4
// against 1.6e-4 for the float32 build of the oracle, which stops at 1e-6 too) -- and the normal is what a caller of the
// query reads.  A hull terminates on a vertex after a handful of steps whatever the tolerance: those pairs go through the
// solver's own function, bit for bit its answer.
__device__ __noinline__ float gjk_distance_fine(const DevModel& M, const Cvx& a, const Cvx& b, float shrink, f3& pa, f3& pb) {
    Simplex S;
    S.n = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) { S.W[i] = mk3(0, 0, 0); S.A[i] = mk3(0, 0, 0); S.B[i] = mk3(0, 0, 0); S.lam[i] = 0.f; }
    f3 v = a.c - b.c;
    if (dot(v, v) == 0.f) v.x = 1.f;
    const float eps = 1e-6f;
    for (int it = 0; it < 40; it++) {
        Vtx nw;
        nw.a = support_core(M, a, -v, shrink);
        nw.b = support_core(M, b, v, shrink);
        nw.w = nw.a - nw.b;
        const float vv = dot(v, v), vw = dot(v, nw.w);
        if (S.n > 0 && vv - vw <= eps * vv) break;
        bool dup = false;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const f3 d = S.W[i] - nw.w;
            if (i < S.n && dot(d, d) <= 1e-12f) dup = true;
        }
        if (dup) break;
        sx_put(S, S.n, nw, 0.f);
        S.n++;
        if (!simplex_closest(S, v)) return -1.0f;
        if (dot(v, v) <= 1e-12f) return -1.0f;
    }
    f3 qa = mk3(0.f, 0.f, 0.f), qb = mk3(0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (i < S.n) { qa = qa + S.A[i] * S.lam[i]; qb = qb + S.B[i] * S.lam[i]; }
    pa = qa;
    pb = qb;
    return sqrtf(dot(v, v));
}
// the two-tier rule of find_self_contacts_v1 for a cylinder A against a cylinder or the box B, both in LDS
__device__ __forceinline__ Closest closest_of(const DevModel& M, const Cvx& A, const Cvx& B, Witness& w) {
    Closest r;
    float mg = M.margin;
    r.tier = 0;
    const bool hull = M.hull_sides > 0;
    float dd = hull ? gjk_distance(M, A, B, 0.f, w.pa, w.pb) : gjk_distance_fine(M, A, B, 0.f, w.pa, w.pb);
    if (dd < 0.f) {
        dd = hull ? gjk_distance(M, A, B, kShrink, w.pa, w.pb) : gjk_distance_fine(M, A, B, kShrink, w.pa, w.pb);
        mg = M.margin + kShrink;
        r.tier = 1;
    }
    if (dd < 0.f) {
        const f3 d = A.c - B.c;
        const float nn = sqrtf(dot(d, d));
        r.tier = 2;
        r.n = nn > 0.f ? d * (1.0f / nn) : (B.box ? mk3(-1.f, 0.f, 0.f) : mk3(0.f, 0.f, 1.f));
        r.P = B.box ? A.c : (A.c + B.c) * 0.5f;
        r.PB = r.P;
        r.dist = -2.0f * mg;
    } else {
        const f3 pa = w.pa, pb = w.pb;
        r.n = (pa - pb) * (1.0f / dd);
        r.dist = dd - 2.0f * mg;
        r.P = pa - r.n * mg;
        r.PB = pb + r.n * mg;
    }
    return r;
}
// a float as an integer with the same order (an involution): the minimum over floats of either sign as an integer minimum
__device__ __forceinline__ int order_key(int bits) { return bits >= 0 ? bits : bits ^ 0x7fffffff; }

template <int N, bool V2>
__global__ __launch_bounds__(64) void closest_points_kernel(const DevModel* __restrict__ Mp, const float* __restrict__ recs,
                                                            const float* __restrict__ box_all,
                                                            const int32_t* __restrict__ env_ids, float distance, int flags,
                                                            int max_pairs, float* __restrict__ points,
                                                            float* __restrict__ clearance, int32_t* __restrict__ count,
                                                            int n_rows, int n_envs) {
    using LT = Lds<N, V2>;
    constexpr int NC = 2 * N;                      // cylinders; b = NC names the box
    constexpr int NP = link_pairs_of(NC);
    static_assert(NC <= 64, "one cylinder per lane, and a pair packs into 12 bits");
    __shared__ float4 smem_raw[(sizeof(LT) + 15) / 16];
    __shared__ CvxSlot fr[NC + 1];                 // the cylinders' world frames; entry NC: the box
    __shared__ Witness wit[64];
    __shared__ unsigned short cand[NP + (NP & 1)];
    __shared__ int cmin[NC];
    __shared__ float stage[kContactFloats][kClosestStageStride];
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    const DevModel& M = *Mp;
    const int lane = threadIdx.x;
    const int slots = NC + max_pairs;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int blk = blockIdx.x; blk < n_rows; blk += gridDim.x) {
        int env;
        const bool known = load_row_env(L, M, recs, env_ids, blk, n_envs, lane, env);
        float4* dst = points ? reinterpret_cast<float4*>(points + (size_t)blk * slots * kContactFloats) : nullptr;
        float* clr = clearance ? clearance + (size_t)blk * 2 * NC : nullptr;
        if (!known) {      // its outputs are zeros; nothing of L was read
            if (dst)
                for (int q = lane; q < slots * (kContactFloats / 4); q += 64) dst[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (clr)
                for (int i = lane; i < 2 * NC; i += 64) clr[i] = 0.f;
            if (count && lane < 2) count[2 * (size_t)blk + lane] = 0;
            continue;
        }
        // records 0 .. n - 1 (n <= 64) of the stage to slots slot0 ..: consecutive float4s
        auto flush = [&](int slot0, int n) { store_rows_as_quads<64>(stage, dst + (size_t)slot0 * (kContactFloats / 4), n, lane); };
        auto put = [&](int row, const Closest& r, int a, int b) {
            stage[0][row] = r.P.x; stage[1][row] = r.P.y; stage[2][row] = r.P.z;
            stage[3][row] = r.PB.x; stage[4][row] = r.PB.y; stage[5][row] = r.PB.z;
            stage[6][row] = r.n.x; stage[7][row] = r.n.y; stage[8][row] = r.n.z;
            stage[9][row] = r.dist; stage[10][row] = (float)r.tier; stage[11][row] = 0.f;
            stage[12][row] = (float)a; stage[13][row] = (float)b; stage[14][row] = 1.f; stage[15][row] = 0.f;
        };
        // frames once: lane = cylinder
        const int a = lane < NC ? lane : NC - 1;
        f3 ca, axa;
        {
            float Rw[9];
            ca = cyl_frame(L, M, a, Rw);
            axa = mk3(Rw[2], Rw[5], Rw[8]);      // the cylinder's axis in the world
            if (lane < NC) {
                Cvx& F = fr[a].s;
                F.c = ca;
#pragma unroll
                for (int i = 0; i < 9; i++) F.R[i] = Rw[i];
                F.box = 0;
                F.half = mk3(0.f, 0.f, 0.f);
                cmin[a] = order_key(__float_as_int(distance));
            }
        }
        lds_sync();
        const float rb = sqrtf(M.cyl_r * M.cyl_r + M.cyl_hl * M.cyl_hl) + M.margin;

        // ---- the (cylinder, box) pairs: slot c, dense
        bool bhit = false;
        Closest bx;
        bx.P = bx.PB = bx.n = mk3(0.f, 0.f, 0.f);
        bx.dist = 0.f;
        bx.tier = 0;
        if ((flags & SNK_PAIRS_BOX) && M.obstacle) {
            // the box's frame: wave-uniform, staged like the cylinders' for the narrow phase
            f3 bc = mk3(M.obs_c[0], M.obs_c[1], M.obs_c[2]);
            float Rx[9];
#pragma unroll
            for (int i = 0; i < 9; i++) Rx[i] = (i % 4 == 0) ? 1.f : 0.f;
            if (M.obstacle == 2 && box_all) box_pose(box_all, env, bc, Rx);      // the free box where it is now
            const f3 half = mk3(M.obs_h[0], M.obs_h[1], M.obs_h[2]);
            if (lane == 0) {
                Cvx& F = fr[NC].s;
                F.c = bc;
#pragma unroll
                for (int i = 0; i < 9; i++) F.R[i] = Rx[i];
                F.box = 1;
                F.half = half;
            }
            lds_sync();
            const float rbox = sqrtf(dot(half, half));
            const f3 d = ca - bc;
            const float reach_ob = rb + rbox + distance;
            if (lane < NC && dot(d, d) <= reach_ob * reach_ob && cyl_box_may_touch(M, ca, axa, bc, Rx, half, distance)) {
                bx = closest_of(M, fr[a].s, fr[NC].s, wit[lane]);
                bhit = bx.dist < distance;
            }
        }
        const int nbox = __popcll(__ballot(bhit));
        if (clr && lane < NC) clr[lane] = bhit ? bx.dist : distance;
        if (dst) {
            if (lane < NC) {
                if (bhit) put(lane, bx, lane, NC);
                else {
#pragma unroll
                    for (int j = 0; j < kContactFloats; j++) stage[j][lane] = 0.f;
                }
            }
            lds_sync();
            flush(0, NC);
            lds_sync();
        }

        // ---- the link-link pairs: slots NC .., compact, in the solver's order
        int nfound = 0;
        if (flags & SNK_PAIRS_LINKS) {
            const float reach = 2.0f * rb + distance;
            int ncand = 0;
#pragma unroll 1
            for (int delta = 2; delta < NC; delta++) {
                const int b = lane + delta;
                const bool valid = b < NC;            // (lane < NC with it)
                const int bb = valid ? b : a;
                const Cvx& Fb = fr[bb].s;
                const f3 cb = Fb.c;
                const f3 d = ca - cb;
                bool c = valid && dot(d, d) <= reach * reach;
                if (c) c = cyl_cyl_may_touch(M, ca, axa, cb, mk3(Fb.R[2], Fb.R[5], Fb.R[8]), distance);
                const unsigned long long bal = __ballot(c);
                if (c) cand[ncand + __popcll(bal & below)] = (unsigned short)(a | (b << 6));
                ncand += __popcll(bal);
            }
            lds_sync();
            int pend = 0, written = 0;           // records staged and not yet stored; records stored or clipped
#pragma unroll 1
            for (int base = 0; base < ncand; base += 64) {
                const int i = base + lane;
                bool hit = false;
                int pa = 0, pb = 0;
                Closest r;
                r.P = r.PB = r.n = mk3(0.f, 0.f, 0.f);
                r.dist = 0.f;
                r.tier = 0;
                if (i < ncand) {
                    const int pk = cand[i];
                    pa = pk & 63;
                    pb = pk >> 6;
                    r = closest_of(M, fr[pa].s, fr[pb].s, wit[lane]);
                    hit = r.dist < distance;
                }
                const unsigned long long bal = __ballot(hit);
                if (hit) {
                    const int key = order_key(__float_as_int(r.dist));
                    atomicMin(&cmin[pa], key);
                    atomicMin(&cmin[pb], key);
                    if (dst) put(pend + __popcll(bal & below), r, pa, pb);
                }
                const int k = __popcll(bal);
                nfound += k;
                pend += k;
                if (dst && pend >= 64) {
                    lds_sync();
                    const int room = max_pairs - written;
                    flush(NC + written, room < 64 ? (room > 0 ? room : 0) : 64);
                    lds_sync();
                    float keep[kContactFloats];
#pragma unroll
                    for (int j = 0; j < kContactFloats; j++) keep[j] = stage[j][64 + lane];
                    lds_sync();
#pragma unroll
                    for (int j = 0; j < kContactFloats; j++)
                        if (lane < pend - 64) stage[j][lane] = keep[j];
                    written += 64;
                    pend -= 64;
                }
            }
            if (dst && pend > 0) {
                lds_sync();
                const int room = max_pairs - written;
                flush(NC + written, room < pend ? (room > 0 ? room : 0) : pend);
            }
        }
        lds_sync();
        if (dst) {      // the slots behind the found pairs: zeros
            const int live = nfound < max_pairs ? nfound : max_pairs;
            for (int q = (NC + live) * (kContactFloats / 4) + lane; q < slots * (kContactFloats / 4); q += 64)
                dst[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (clr && lane < NC) clr[NC + lane] = __int_as_float(order_key(cmin[lane]));
        if (count && lane == 0) { count[2 * (size_t)blk] = nbox; count[2 * (size_t)blk + 1] = nfound; }
        lds_sync();      // (the frames, the minima and the record are read by every lane above: the next env waits for them)
    }
}

// ----------------------------------------------------------------------------------
// copy_envs_kernel: one workgroup per (src, dst) pair.  Every table row of env src -- its padding included: the rows are
// whole 16-byte quads, the state's whole 128-byte lines -- goes to env dst as float4s; the one table of single floats
// (ground friction) as a float.  A pair with an id outside the handle does nothing.
// ----------------------------------------------------------------------------------
constexpr int kCopyTables = 5;
struct CopyArgs {
    float* d[kCopyTables];        // null: no such table (or not asked for)
    int floats[kCopyTables];      // per env
};
__global__ __launch_bounds__(256) void copy_envs_kernel(CopyArgs a, const int32_t* __restrict__ src_ids,
                                                        const int32_t* __restrict__ dst_ids, int n_pairs, int n_envs) {
    for (int p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const int s = src_ids[p], d = dst_ids[p];
        if (s < 0 || s >= n_envs || d < 0 || d >= n_envs || s == d) continue;
#pragma unroll
        for (int t = 0; t < kCopyTables; t++) {
            float* base = a.d[t];
            if (!base) continue;
            const int nf = a.floats[t];
            const float* from = base + (size_t)s * nf;
            float* to = base + (size_t)d * nf;
            if ((nf & 3) == 0) {
                for (int i = threadIdx.x; i < nf / 4; i += 256)
                    reinterpret_cast<float4*>(to)[i] = reinterpret_cast<const float4*>(from)[i];
            } else {
                for (int i = threadIdx.x; i < nf; i += 256) to[i] = from[i];
            }
        }
    }
}

}  // namespace snk
