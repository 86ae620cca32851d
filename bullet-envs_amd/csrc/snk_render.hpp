// snk_render.hpp -- device parts of the ray caster (include/snk.h: "The rendered scene" is the contract): the per-image
// tables render_scene_kernel writes and render_rays_kernel reads, the ray / solid intersections, the shading -- and of
// the ray test ("The ray test"): the same tables and intersections under caller-given rays, hit records for colours.
// Only snk_render.hip includes this: the step kernels' code object (snk_api.hip) has none of it.
#pragma once
#include <hip/hip_runtime.h>

#include "snk_query.hpp"

namespace snk {

// One primitive = 16 floats (64 bytes).  Per image: 2n cylinders, then the box; kPrimStride(n) entries (the last unused).
//   cylinder  [centre 3 | radius | unit axis 3 | half length | 8 unused]          (half length < 0: nothing there)
//   box       [centre 3 | half extents 3 | R 9, row-major, box -> world | 1 unused]   (half extents < 0: no box)
constexpr int kPrimFloats = 16;
__host__ __device__ constexpr int prim_stride(int n) { return (2 * n + 2) * kPrimFloats; }
// The camera of an image = 32 floats: [inverse of M = P V, column-major 16 | M, column-major 16], the inverse taken in
// float64 and rounded
constexpr int kCamFloats = 32;
constexpr int kRenderTile = 16;

constexpr float kRenderInf = __builtin_huge_valf();
constexpr float kRenderTie = 2e-4f;      // a later primitive replaces the kept hit only when nearer by more than this [m]

// the light: (0.4, -0.3, 0.85) normalised (its length is sqrt(0.9725))
constexpr double kLightLen = 0.98615414616580109;
constexpr float kLx = (float)(0.4 / kLightLen), kLy = (float)(-0.3 / kLightLen), kLz = (float)(0.85 / kLightLen);

// The solids of one env as table entries at P, from the forward kinematics in L: lane = cylinder, lane 0 the box too.
// What render_scene_kernel and ray_scene_kernel share.  !known (an env id outside the handle): nothing there.
// QT: the arithmetic of the free box's rotation (quat_rot) -- float for the render, as it always was; double for the ray
// test, whose records carry a column of that matrix as the hit's normal.
template <int N, bool V2, typename QT>
__device__ __forceinline__ void scene_prims(const Lds<N, V2>& L, const DevModel& M, const float* box_all, int env,
                                            bool known, int lane, float* P) {
    if (lane < 2 * N) {
        const int c = lane;
        float* o = P + c * kPrimFloats;
        f3 ctr = mk3(0.f, 0.f, 0.f), ax = mk3(0.f, 0.f, 1.f);
        float hl = -1.f;
        if (known) {
            float Rw[9];
            ctr = cyl_frame(L, M, c, Rw);
            ax = mk3(Rw[2], Rw[5], Rw[8]);
            hl = M.cyl_hl;
        }
        o[0] = ctr.x; o[1] = ctr.y; o[2] = ctr.z; o[3] = M.cyl_r;
        o[4] = ax.x; o[5] = ax.y; o[6] = ax.z; o[7] = hl;
    }
    if (lane == 0) {
        float* o = P + 2 * N * kPrimFloats;
        float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        f3 ctr = ld3(M.obs_c), hh = mk3(-1.f, -1.f, -1.f);
        if (known && M.obstacle != 0) hh = ld3(M.obs_h);
        if (known && M.obstacle == 2 && box_all) box_pose<QT>(box_all, env, ctr, R);
        o[0] = ctr.x; o[1] = ctr.y; o[2] = ctr.z;
        o[3] = hh.x; o[4] = hh.y; o[5] = hh.z;
#pragma unroll
        for (int i = 0; i < 9; i++) o[6 + i] = R[i];      // (6 + 8 = 14: inside the entry's 16 floats)
        o[15] = 0.f;
    }
}

// ----------------------------------------------------------------------------------
// render_scene_kernel: one wave per image.  The env's record -> forward kinematics -> lane = cylinder.
// Plain loads of the records, the free boxes and the model; nothing of the handle's state is written.
// ----------------------------------------------------------------------------------
template <int N, bool V2>
__global__ __launch_bounds__(64) void render_scene_kernel(const DevModel* __restrict__ Mp, const float* __restrict__ recs,
                                                          const float* __restrict__ box_all,
                                                          const int32_t* __restrict__ env_ids,
                                                          const float* __restrict__ cameras, int shared_camera,
                                                          float* __restrict__ prims, float* __restrict__ cams,
                                                          int n_images, int n_envs) {
    using LT = Lds<N, V2>;
    __shared__ float4 smem_raw[(sizeof(LT) + 15) / 16];
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    const DevModel& M = *Mp;
    const int lane = threadIdx.x;
    for (int img = blockIdx.x; img < n_images; img += gridDim.x) {
        int env;
        const bool known = load_row_env(L, M, recs, env_ids, img, n_envs, lane, env);      // (not known: the ground alone)
        float* P = prims + (size_t)img * prim_stride(N);
        scene_prims<N, V2, float>(L, M, box_all, env, known, lane, P);
        if (lane == 1) {
            // M = P V and its inverse (cofactors), in float64: the near and far planes of a camera are orders of
            // magnitude apart, and every ray of the image goes through this inverse
            const float* cm = cameras + (size_t)(shared_camera ? 0 : img) * 32;
            double Mx[16], inv[16];
            for (int c = 0; c < 4; c++)
                for (int r = 0; r < 4; r++) {
                    double s = 0.0;
                    for (int k = 0; k < 4; k++) s += (double)cm[16 + 4 * k + r] * (double)cm[4 * c + k];
                    Mx[4 * c + r] = s;
                }
            const double* m = Mx;
            inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
            inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
            inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
            inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
            inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
            inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
            inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
            inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
            inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
            inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
            inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
            inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
            inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
            inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
            inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
            inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
            const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
            const double idet = 1.0 / det;
            float* o = cams + (size_t)img * kCamFloats;
            for (int i = 0; i < 16; i++) { o[i] = (float)(inv[i] * idet); o[16 + i] = (float)Mx[i]; }
        }
        lds_sync();      // (the image's record is read by every lane above: the next image's load waits for them)
    }
}

// ----------------------------------------------------------------------------------
// ray against solid: the parameter interval [tin, tout] in which o + t d is inside.  false: the ray's line misses.
// ----------------------------------------------------------------------------------
// capped cylinder, m = o - centre.  cap: the entry is through an end cap (else through the side)
__device__ __forceinline__ bool cyl_interval(f3 m, f3 d, f3 A, float r, float hl, float& tin, float& tout, bool& cap, float& dp_out) {
    const float dp = dot(d, A), mp = dot(m, A);
    const f3 dq = d - A * dp, mq = m - A * mp;
    const float a = dot(dq, dq), b = dot(mq, dq), c = dot(mq, mq) - r * r;
    float s_in = -kRenderInf, s_out = kRenderInf;
    if (a > 0.f) {
        const float disc = b * b - a * c;
        if (!(disc >= 0.f)) return false;
        const float sq = sqrtf(disc);
        s_in = (-b - sq) / a; s_out = (-b + sq) / a;
    } else if (c > 0.f) return false;
    float c_in = -kRenderInf, c_out = kRenderInf;
    if (dp != 0.f) {
        const float t1 = (-hl - mp) / dp, t2 = (hl - mp) / dp;
        c_in = fminf(t1, t2); c_out = fmaxf(t1, t2);
        if (hl < 0.f) return false;
    } else if (!(fabsf(mp) <= hl)) return false;
    cap = c_in > s_in;
    tin = cap ? c_in : s_in;
    tout = fminf(s_out, c_out);
    dp_out = dp;
    return tin <= tout;
}
// box: B = its table entry [centre 3 | half extents 3 | R 9 row-major, box -> world].  axis / sign: the face the ray enters through, outward normal
// sign * column `axis` of R
__device__ __forceinline__ bool box_interval(f3 m, f3 d, const float* __restrict__ B, float& tin, float& tout, int& axis, float& sign) {
    tin = -kRenderInf; tout = kRenderInf; axis = 0; sign = 1.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const f3 ak = mk3(B[6 + k], B[9 + k], B[12 + k]);
        const float ok = dot(ak, m), dk = dot(ak, d), hk = B[3 + k];
        if (hk < 0.f) return false;
        if (dk != 0.f) {
            const float t1 = (-hk - ok) / dk, t2 = (hk - ok) / dk;
            const float lo = fminf(t1, t2), hi = fmaxf(t1, t2);
            if (lo > tin) { tin = lo; axis = k; sign = dk > 0.f ? -1.f : 1.f; }
            tout = fminf(tout, hi);
        } else if (!(fabsf(ok) <= hk)) return false;
    }
    return tin <= tout;
}

// ----------------------------------------------------------------------------------
// render_rays_kernel: one 256-thread workgroup per 16 x 16 pixel tile of one image; thread = pixel.
// T: the image's table in LDS, [prim_stride(n) floats of primitives | kCamFloats of camera].
// ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void render_rays_kernel(const float* __restrict__ prims, const float* __restrict__ cams,
                                                          int ncyl, int width, int height, int tiles_x, int tiles_y,
                                                          long long n_work, int flags, uint32_t* __restrict__ rgba,
                                                          float* __restrict__ depth, int32_t* __restrict__ seg) {
    __shared__ float4 T4[(prim_stride(kMaxN) + kCamFloats) / 4];
    const float* T = reinterpret_cast<const float*>(T4);
    const int tid = threadIdx.x;
    const int pstride = (ncyl + 2) * kPrimFloats;                 // = prim_stride(n), ncyl = 2 n
    const int tiles = tiles_x * tiles_y;
    for (long long w = blockIdx.x; w < n_work; w += gridDim.x) {
        const long long img = w / tiles;
        const int tile = (int)(w - img * tiles);
        const int ty0 = tile / tiles_x, tx0 = tile - ty0 * tiles_x;
        {
            const float4* src = reinterpret_cast<const float4*>(prims + (size_t)img * pstride);
            const int nq = (ncyl + 1) * (kPrimFloats / 4);           // cylinders and the box
            for (int q = tid; q < nq; q += 256) T4[q] = src[q];
            const float4* cs = reinterpret_cast<const float4*>(cams + (size_t)img * kCamFloats);
            if (tid < kCamFloats / 4) T4[pstride / 4 + tid] = cs[tid];
        }
        __syncthreads();
        // a wave = four rows of sixteen pixels: its stores are four runs of 64 consecutive bytes
        const int i = tx0 * kRenderTile + (tid & 15), j = ty0 * kRenderTile + (tid >> 4);
        if (i < width && j < height) {
            const float* C = T + pstride;                             // [Minv 16 | M 16], column-major
            const float x = (2.0f * ((float)i + 0.5f)) / (float)width - 1.0f;
            const float y = 1.0f - (2.0f * ((float)j + 0.5f)) / (float)height;
            // the pixel centre on the near plane (NDC z = -1) and on the far plane (z = +1), back in the world
            float an[4], af[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float base = C[r] * x + C[4 + r] * y + C[12 + r];
                an[r] = base - C[8 + r];
                af[r] = base + C[8 + r];
            }
            const f3 o = mk3(an[0] / an[3], an[1] / an[3], an[2] / an[3]);
            const f3 pf = mk3(af[0] / af[3], af[1] / af[3], af[2] / af[3]);
            f3 d = pf - o;
            const float tf = sqrtf(dot(d, d));
            d = d * (1.0f / tf);
            // nearest hit: a later primitive replaces the kept one only when it is nearer by more than kRenderTie
            float tbest = kRenderInf;
            int id = -1;
            f3 nrm = mk3(0.f, 0.f, 1.f);
            if (d.z != 0.f) {
                const float t = -o.z / d.z;
                if (t >= 0.f && t <= tf) { tbest = t; id = 0; }
            }
            for (int c = 0; c < ncyl; c++) {
                const float* p = T + c * kPrimFloats;
                const f3 A = ld3(p + 4);
                float tin, tout, dp;
                bool cap;
                if (cyl_interval(o - ld3(p), d, A, p[3], p[7], tin, tout, cap, dp) && tin >= 0.f && tin <= tf &&
                    tin < tbest - kRenderTie) {
                    tbest = tin; id = 1 + c;
                    if (cap) nrm = A * (dp > 0.f ? -1.f : 1.f);
                    else {
                        const f3 m = o - ld3(p);
                        const f3 q = m + d * tin;
                        nrm = (q - A * dot(q, A)) * (1.0f / p[3]);
                    }
                }
            }
            {
                const float* p = T + ncyl * kPrimFloats;
                float tin, tout, sign;
                int axis;
                if (box_interval(o - ld3(p), d, p, tin, tout, axis, sign) && tin >= 0.f && tin <= tf && tin < tbest - kRenderTie) {
                    tbest = tin; id = 1 + ncyl;
                    nrm = mk3(p[6 + axis], p[9 + axis], p[12 + axis]) * sign;
                }
            }
            uint32_t px = 200u | (215u << 8) | (235u << 16) | (255u << 24);
            float dep = 1.0f;
            if (id >= 0) {
                const f3 X = o + d * tbest;
                f3 alb;
                if (id == 0) {
                    const int par = ((int)floorf(X.x * 2.0f) + (int)floorf(X.y * 2.0f)) & 1;      // 0.5 m cells
                    alb = par ? mk3(0.55f, 0.65f, 0.85f) : mk3(0.95f, 0.95f, 0.95f);
                } else if (id <= ncyl) {
                    alb = ((id - 1) & 1) ? mk3(0.25f, 0.25f, 0.28f) : mk3(0.85f, 0.35f, 0.15f);
                } else {
                    alb = mk3(0.45f, 0.75f, 0.45f);
                }
                const f3 Lv = mk3(kLx, kLy, kLz);
                const float ndl = fmaxf(0.f, dot(nrm, Lv));
                float lit = 1.0f;
                if ((flags & SNK_RENDER_SHADOW) && ndl > 0.f) {
                    // occluded: the ray from just outside the surface towards the light meets a cylinder or the box
                    const f3 so = X + nrm * 1e-4f;
                    for (int c = 0; c < ncyl; c++) {
                        const float* p = T + c * kPrimFloats;
                        float tin, tout, dp;
                        bool cap;
                        if (cyl_interval(so - ld3(p), Lv, ld3(p + 4), p[3], p[7], tin, tout, cap, dp) && tout >= 0.f) lit = 0.f;
                    }
                    const float* p = T + ncyl * kPrimFloats;
                    float tin, tout, sign;
                    int axis;
                    if (box_interval(so - ld3(p), Lv, p, tin, tout, axis, sign) && tout >= 0.f) lit = 0.f;
                } else if (flags & SNK_RENDER_SHADOW) {
                    lit = 0.f;
                }
                const float k = 0.4f + 0.6f * ndl * lit;
                const uint32_t r8 = (uint32_t)floorf(255.0f * (alb.x * k) + 0.5f);
                const uint32_t g8 = (uint32_t)floorf(255.0f * (alb.y * k) + 0.5f);
                const uint32_t b8 = (uint32_t)floorf(255.0f * (alb.z * k) + 0.5f);
                px = r8 | (g8 << 8) | (b8 << 16) | (255u << 24);
                const float cz = C[16 + 2] * X.x + C[16 + 6] * X.y + C[16 + 10] * X.z + C[16 + 14];
                const float cw = C[16 + 3] * X.x + C[16 + 7] * X.y + C[16 + 11] * X.z + C[16 + 15];
                dep = 0.5f * (cz / cw) + 0.5f;
            }
            const size_t at = ((size_t)img * (size_t)height + (size_t)j) * (size_t)width + (size_t)i;
            rgba[at] = px;
            if (depth) depth[at] = dep;
            if (seg) seg[at] = id;
        }
        __syncthreads();      // (the table is replaced by the next work item's)
    }
}

// ----------------------------------------------------------------------------------
// The ray test (include/snk.h: "The ray test" is the contract).
// A row's table is the render's, with the parent frame of the row's rays in the entry the render leaves unused:
//   entry 2n + 1  [R 9, row-major, frame -> world | origin 3 | known: 1, or 0 for an env id outside the handle | 3 unused]
// ----------------------------------------------------------------------------------
constexpr int kRayChunk = 256;            // rays of one workgroup, one per thread
constexpr int kRayFloats = 6, kHitFloats = 8;
// The staging image of a chunk's records: float j of ray w at stage[j][w] (snk_query.hpp: store_rows_as_quads)
constexpr int kHitStride = 260;

// ray_scene_kernel: one wave per row.  render_scene_kernel without a camera, plus the frame of link-table row
// `parent_row` of the row's own env (-1: the world's; link_row_frame): origin = the link's COM.
template <int N, bool V2>
__global__ __launch_bounds__(64) void ray_scene_kernel(const DevModel* __restrict__ Mp, const float* __restrict__ recs,
                                                       const float* __restrict__ box_all, const float* __restrict__ links,
                                                       const int32_t* __restrict__ env_ids, int parent_row,
                                                       float* __restrict__ prims, int n_rows, int n_envs) {
    using LT = Lds<N, V2>;
    __shared__ float4 smem_raw[(sizeof(LT) + 15) / 16];
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    const DevModel& M = *Mp;
    const int lane = threadIdx.x;
    for (int row = blockIdx.x; row < n_rows; row += gridDim.x) {
        int env;
        const bool known = load_row_env(L, M, recs, env_ids, row, n_envs, lane, env);
        float* P = prims + (size_t)row * prim_stride(N);
        scene_prims<N, V2, double>(L, M, box_all, env, known, lane, P);
        if (lane == 1) {
            float* o = P + (2 * N + 1) * kPrimFloats;
            float Rw[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
            f3 org = mk3(0.f, 0.f, 0.f);
            if (known && parent_row >= 0) {
                f3 ow;
                link_row_frame(L, links + (size_t)parent_row * kLinkFloats, Rw, ow, org);
            }
#pragma unroll
            for (int i = 0; i < 9; i++) o[i] = Rw[i];
            o[9] = org.x; o[10] = org.y; o[11] = org.z;
            o[12] = known ? 1.f : 0.f;
            o[13] = 0.f; o[14] = 0.f; o[15] = 0.f;
        }
        lds_sync();      // (the row's record is read by every lane above: the next row's load waits for them)
    }
}

// ray_cast_kernel: one 256-thread workgroup per (row, chunk of 256 rays); thread = ray.
// A ray is 24 bytes and a record 32: thread = ray accesses of global memory would stride.  So the chunk's 6 x 256 input
// floats come in as consecutive dwords (lane i of a load reads dword i: the rays are 4-byte aligned, nothing more) and
// each thread takes its ray from LDS as three 8-byte reads (24 t is a multiple of 8; ds_read_b64 banks on the dword
// address mod 64, and 6 t mod 64 are 32 distinct even numbers over a half: no conflicts).  The records are staged
// (kHitStride above) and leave as consecutive float4s: a wave-wide store writes 1 KB, every 128-byte line whole.
__global__ __launch_bounds__(kRayChunk) void ray_cast_kernel(const float* __restrict__ prims, const float* __restrict__ rays,
                                                             int shared_rays, int ncyl, int n_rays, int chunks,
                                                             long long n_work, int flags, float* __restrict__ hits) {
    __shared__ float4 T4[prim_stride(kMaxN) / 4];
    __shared__ float2 in2[kRayChunk * kRayFloats / 2];
    __shared__ float stage[kHitFloats][kHitStride];
    const float* T = reinterpret_cast<const float*>(T4);
    float* in = reinterpret_cast<float*>(in2);
    const int tid = threadIdx.x;
    const int pstride = (ncyl + 2) * kPrimFloats;                 // = prim_stride(n), ncyl = 2 n
    for (long long w = blockIdx.x; w < n_work; w += gridDim.x) {
        const long long row = w / chunks;
        const int r0 = (int)(w - row * chunks) * kRayChunk;
        const int cnt = n_rays - r0 < kRayChunk ? n_rays - r0 : kRayChunk;      // rays of this chunk: nothing beyond them is touched
        {
            const float4* src = reinterpret_cast<const float4*>(prims + (size_t)row * pstride);
            const int nq = (ncyl + 2) * (kPrimFloats / 4);           // cylinders, the box and the frame
            for (int q = tid; q < nq; q += kRayChunk) T4[q] = src[q];
            const float* rs = rays + ((size_t)(shared_rays ? 0 : row) * (size_t)n_rays + (size_t)r0) * kRayFloats;
#pragma unroll
            for (int k = 0; k < kRayFloats; k++) {
                const int i = kRayChunk * k + tid;
                if (i < cnt * kRayFloats) in[i] = rs[i];
            }
        }
        __syncthreads();
        if (tid < cnt) {
            const float2 a = in2[3 * tid], b = in2[3 * tid + 1], c = in2[3 * tid + 2];
            const float* F = T + (ncyl + 1) * kPrimFloats;            // [R 9 | origin 3 | known]
            const bool finite = isfinite(a.x) && isfinite(a.y) && isfinite(b.x) && isfinite(b.y) && isfinite(c.x) && isfinite(c.y);
            const f3 org = ld3(F + 9);
            const f3 o = org + mulRv(F, mk3(a.x, a.y, b.x));
            const f3 pt = org + mulRv(F, mk3(b.y, c.x, c.y));
            f3 d = pt - o;
            const float tf = sqrtf(dot(d, d));
            float tbest = kRenderInf;
            int id = -1;
            f3 nrm = mk3(0.f, 0.f, 1.f);
            // a zero-length ray, a non-finite one (or one whose length is) and an env outside the handle hit nothing
            if (finite && tf > 0.f && tf < kRenderInf && F[12] != 0.f) {
                d = mk3(d.x / tf, d.y / tf, d.z / tf);      // (a division each: the ranges carry the direction's round-off)
                // nearest hit: a later primitive replaces the kept one only when it is nearer by more than kRenderTie
                if ((flags & SNK_RAYS_GROUND) && d.z != 0.f) {
                    const float t = -o.z / d.z;
                    if (t >= 0.f && t <= tf) { tbest = t; id = 0; }
                }
                if (flags & SNK_RAYS_SNAKE)
                    for (int cy = 0; cy < ncyl; cy++) {
                        const float* p = T + cy * kPrimFloats;
                        const f3 A = ld3(p + 4);
                        float tin, tout, dp;
                        bool cap;
                        if (cyl_interval(o - ld3(p), d, A, p[3], p[7], tin, tout, cap, dp) && tin >= 0.f && tin <= tf &&
                            tin < tbest - kRenderTie) {
                            tbest = tin; id = 1 + cy;
                            if (cap) nrm = A * (dp > 0.f ? -1.f : 1.f);
                            else {
                                const f3 m = o - ld3(p);
                                const f3 q = m + d * tin;
                                nrm = (q - A * dot(q, A)) * (1.0f / p[3]);
                            }
                        }
                    }
                if (flags & SNK_RAYS_BOX) {
                    const float* p = T + ncyl * kPrimFloats;
                    float tin, tout, sign;
                    int axis;
                    if (box_interval(o - ld3(p), d, p, tin, tout, axis, sign) && tin >= 0.f && tin <= tf && tin < tbest - kRenderTie) {
                        tbest = tin; id = 1 + ncyl;
                        nrm = mk3(p[6 + axis], p[9 + axis], p[12 + axis]) * sign;
                    }
                }
            }
            // the miss record is [1, 0 x 6, -1]: never zeros, which would read as the ground hit at the ray's origin
            float v[kHitFloats] = {1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -1.f};
            if (id >= 0) {
                const f3 X = o + d * tbest;
                v[0] = tbest / tf;
                v[1] = X.x; v[2] = X.y; v[3] = X.z;
                v[4] = nrm.x; v[5] = nrm.y; v[6] = nrm.z;
                v[7] = (float)id;
            }
#pragma unroll
            for (int j = 0; j < kHitFloats; j++) stage[j][tid] = v[j];
        }
        __syncthreads();
        float4* dst = reinterpret_cast<float4*>(hits + ((size_t)row * (size_t)n_rays + (size_t)r0) * kHitFloats);
        store_rows_as_quads<kRayChunk>(stage, dst, cnt, tid);
        __syncthreads();      // (the table and both staging images are replaced by the next work item's)
    }
}

}  // namespace snk
