// snk_world.hpp -- device parts of the tensor seam that are not step arithmetic (include/snk.h: snk_link_states,
// snk_copy_envs): the per-link read-out of the unmerged URDF tree and the env-to-env copy of the simulator state.
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
