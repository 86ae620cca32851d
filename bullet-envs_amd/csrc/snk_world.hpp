// snk_world.hpp -- device parts of the tensor seam that are not step arithmetic (include/snk.h: snk_link_states,
// snk_contacts, snk_copy_envs): the per-link read-out of the unmerged URDF tree, the contact cache as contact records,
// and the env-to-env copy of the simulator state.
// Only snk_world.hip includes this: the step kernels' code object (snk_api.hip) has none of it.
#pragma once
#include <hip/hip_runtime.h>

#include "snk_dynamics.hpp"
#include "snk_env_io.hpp"
#include "snk_lds.hpp"
#include "snk_model.hpp"
#include "snk_wave.hpp"

namespace snk {

// One output row = 16 floats (64 bytes): [COM 3 | quaternion xyzw 4 | link-frame origin 3 | COM velocity 3 | omega 3]
constexpr int kLinkStateFloats = 16;
// The staging image of one pass: float j of the pass's row l at stage[j][l].  A row stride of 66 floats keeps both sides
// free of bank conflicts (cdna_hip_programming.md 2: ds_write_b32 and ds_read_b32 bank = dword address mod 32 within a
// 32-lane half): the writes go lane = row, consecutive banks; the read of float 4 p + e of row w by lane 4 w + p sits at
// bank (8 p + 2 e + w) mod 32, distinct over the p = 0..3, w = 8 consecutive rows of a half.
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
        const int env = env_ids ? env_ids[blk] : blk;
        // an env id cannot be refused from inside a launch: one outside the handle reads nothing, its rows are zeros
        const bool known = env >= 0 && env < n_envs;
        if (known) {
            load_rec(L, recs + (size_t)env * LT::REC, lane);
            fk_vel(L, M, lane);
        }
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
                const float* T = links + (size_t)r * kLinkFloats;
                const int b = __float_as_int(T[15]);
                const float* Rb = L.R[b];
                float Rw[9];
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++)
                        Rw[3 * i + j] = Rb[3 * i] * T[j] + Rb[3 * i + 1] * T[3 + j] + Rb[3 * i + 2] * T[6 + j];
                const f3 ob = ld3(L.o[b]);
                const f3 ow = ob + mulRv(Rb, ld3(T + 9));
                const f3 cw = ow + mulRv(Rw, ld3(T + 12));
                // the body's twist at its joint origin carries the joint's own rate: v(COM) = v(o_b) + omega x (c - o_b)
                const f3 w = ld3(L.w[b]);
                const f3 vc = ld3(L.v[b]) + cross(w, cw - ob);
                st3(v, cw); quat_of(Rw, v + 3); st3(v + 7, ow); st3(v + 10, vc); st3(v + 13, w);
            }
#pragma unroll
            for (int j = 0; j < kLinkStateFloats; j++) stage[j][lane] = v[j];
            lds_sync();
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
        const int env = env_ids ? env_ids[blk] : blk;
        // an env id cannot be refused from inside a launch: one outside the handle reads nothing, its outputs are zeros
        const bool known = env >= 0 && env < n_envs;
        if (known) {
            load_rec(L, recs + (size_t)env * LT::REC, lane);
            fk_vel(L, M, lane);
        }
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
                const int b = (u + 1) >> 1;
                const float* Rb = L.R[b];
                cyl_world_rot(Rb, M.cyl_R[u], R);
                org = ld3(L.o[b]) + mulRv(Rb, ld3(M.cyl_c[u]));
                zo = M.cyl_zoff;
                n = manifold_load_global(mf_all + ((size_t)env * NC + u) * kMfFloats, p);
            } else if (known && u == NC && box_all) {
                // [state 13 | count | 4 x (a3, b.x, b.y, lambda) | padding]: floats 0 .. 39 as ten quads
                const float4* bq = reinterpret_cast<const float4*>(box_all + (size_t)env * kBoxFloats);
                float f[40];
#pragma unroll
                for (int i = 0; i < 10; i++) { const float4 q = bq[i]; f[4 * i] = q.x; f[4 * i + 1] = q.y; f[4 * i + 2] = q.z; f[4 * i + 3] = q.w; }
                const float qx = f[3], qy = f[4], qz = f[5], qw = f[6];      // R(quat) as box_frame_v1 forms it
                const float s2 = 2.0f / (qx * qx + qy * qy + qz * qz + qw * qw);
                const float xs = qx * s2, ys = qy * s2, zs = qz * s2;
                const float wx = qw * xs, wy = qw * ys, wz = qw * zs, xx = qx * xs, xy = qx * ys, xz = qx * zs, yy = qy * ys,
                            yz = qy * zs, zz = qz * zs;
                R[0] = 1 - (yy + zz); R[1] = xy - wz; R[2] = xz + wy; R[3] = xy + wz; R[4] = 1 - (xx + zz); R[5] = yz - wx;
                R[6] = xz - wy; R[7] = yz + wx; R[8] = 1 - (xx + yy);
                org = mk3(f[0], f[1], f[2]);
                n = (int)f[13];
                n = n < 0 ? 0 : (n > 4 ? 4 : n);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    p[j].a = mk3(f[14 + 6 * j], f[15 + 6 * j], f[16 + 6 * j]);
                    p[j].b = mk3(f[17 + 6 * j], f[18 + 6 * j], 0.f);
                    p[j].lam = f[19 + 6 * j];
                }
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
