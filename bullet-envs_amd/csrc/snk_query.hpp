// snk_query.hpp -- what the read-only query kernels below the fused step share (snk_world.hpp: link states, contacts,
// closest points; snk_render.hpp: the render's and the ray test's tables): the prologue of a wave-per-row kernel, the world
// frames of a link-table row, of a cylinder and of the free box, and the staged, transposed store.  One definition each;
// a new query kernel is written in these ("Adding a query kernel").  Device code only, all of it inlined: no
// LDS of its own, no atomics, no scratch memory.  The step kernels' code object (snk_api.hip) has none of it.
// These kernels' bits are pinned (tests/test_gpu_query_bits.py): an edit here that is meant to leave them alone is checked.
#pragma once
#include <hip/hip_runtime.h>

#include "snk_contacts.hpp"
#include "snk_dynamics.hpp"
#include "snk_env_io.hpp"
#include "snk_lds.hpp"
#include "snk_model.hpp"
#include "snk_wave.hpp"

namespace snk {

// The prologue of a wave-per-row kernel's row loop: the row's env (env_ids null: the row itself) and whether the handle
// knows it; if so its record is in L and the forward kinematics and body twists are run (as obs_kernel does).  An env id
// cannot be refused from inside a launch: one outside the handle reads nothing, and the kernel writes its row as "nothing
// there" (zeros; the ground alone).  Every lane reads L behind this, so the row loop ends in lds_sync(): a block that
// takes another row (more rows than grid_for's blocks) must not load the next record under lanes still reading this one.
template <class LT>
__device__ __forceinline__ bool load_row_env(LT& L, const DevModel& M, const float* __restrict__ recs,
                                             const int32_t* __restrict__ env_ids, int row, int n_envs, int lane, int& env) {
    env = env_ids ? env_ids[row] : row;
    const bool known = env >= 0 && env < n_envs;
    if (known) {
        load_rec(L, recs + (size_t)env * LT::REC, lane);
        fk_vel(L, M, lane);
    }
    return known;
}

// The world frame of the link-table row T (snk_model.hpp: build_link_table; [R 9, link in body | origin 3 | COM 3 | body])
// from the forward kinematics in L: Rw = R(body) R(link in body), ow the link frame's origin, cw the link's COM.
// Returns the row's body.
template <class LT>
__device__ __forceinline__ int link_row_frame(const LT& L, const float* T, float* Rw, f3& ow, f3& cw) {
    const int b = __float_as_int(T[15]);
    const float* Rb = L.R[b];
    cyl_world_rot(Rb, T, Rw);
    ow = ld3(L.o[b]) + mulRv(Rb, ld3(T + 9));
    cw = ow + mulRv(Rw, ld3(T + 12));
    return b;
}

// The world frame of cylinder c from the forward kinematics in L: Rw = R(body) R(cylinder in body) -- its column 2 is the
// cylinder's axis -- and, returned, the centre.  (find_contacts_v1 and find_self_contacts_v1 form the same in the step kernels.)
template <class LT>
__device__ __forceinline__ f3 cyl_frame(const LT& L, const DevModel& M, int c, float* Rw) {
    const int b = (c + 1) >> 1;
    const float* Rb = L.R[b];
    cyl_world_rot(Rb, M.cyl_R[c], Rw);
    return ld3(L.o[b]) + mulRv(Rb, ld3(M.cyl_c[c]));
}

// The free box's record of an env (obstacle 2; snk_env_io.hpp: kBoxFloats per env, whole 16-byte quads), indexed HERE:
//   [position 3 | quaternion xyzw 4 | omega 3 | velocity 3 | point count | 4 x (a 3, b.x, b.y, lambda) | padding]
// box_pose: its centre and rotation (QT: quat_rot's arithmetic).
template <typename QT = float>
__device__ __forceinline__ void box_pose(const float* __restrict__ box_all, int env, f3& centre, float* R) {
    const float4* bq = reinterpret_cast<const float4*>(box_all + (size_t)env * kBoxFloats);
    const float4 q0 = bq[0], q1 = bq[1];
    centre = mk3(q0.x, q0.y, q0.z);
    quat_rot<QT>(q0.w, q1.x, q1.y, q1.z, R);
}
// box_manifold: its cached points against the ground (a, b, lambda; d is not kept) and their count, clamped to 0 .. 4
__device__ __forceinline__ int box_manifold(const float* __restrict__ box_all, int env, MPt (&p)[4]) {
    const float4* bq = reinterpret_cast<const float4*>(box_all + (size_t)env * kBoxFloats);
    float f[28];      // floats 12 .. 39 of the record
#pragma unroll
    for (int i = 0; i < 7; i++) { const float4 q = bq[3 + i]; f[4 * i] = q.x; f[4 * i + 1] = q.y; f[4 * i + 2] = q.z; f[4 * i + 3] = q.w; }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        p[j].a = mk3(f[2 + 6 * j], f[3 + 6 * j], f[4 + 6 * j]);
        p[j].b = mk3(f[5 + 6 * j], f[6 + 6 * j], 0.f);
        p[j].lam = f[7 + 6 * j];
    }
    const int n = (int)f[1];
    return n < 0 ? 0 : (n > 4 ? 4 : n);
}

// The staged, transposed store: a kernel whose thread = output row of FLOATS floats stages float j of row r at
// stage[j][r]; `rows` <= THREADS rows then leave as consecutive float4s at dst, quad Q by thread Q mod THREADS: a
// wave-wide store instruction writes 1 KB of consecutive bytes, every 128-byte line whole.  The caller puts a barrier
// between its writes of the stage and this, and another before the stage is written again.
// STRIDE keeps both sides free of bank conflicts (cdna_hip_programming.md 2: ds_write_b32 and ds_read_b32 bank = dword
// address mod 32 within a 32-lane half).  The writes go lane = row, consecutive banks.  With q = FLOATS / 4 quads per row,
// the read of float 4 p + e of row w by lane q w + p sits at bank ((4 p + e) STRIDE + w) mod 32, and a half holds p = 0 ..
// q - 1 of 32 / q consecutive rows: distinct for STRIDE = 2 mod 32 at q = 4 (8 p + 2 e + w: 66 for a pass of 64 rows, 130 =
// 4 x 32 + 2 for the closest points' 128) and for STRIDE = 4 mod 8 at q = 2 (16 p + 4 e + w: 260, the first >= 256 rays).
template <int THREADS, int FLOATS, int STRIDE>
__device__ __forceinline__ void store_rows_as_quads(const float (&stage)[FLOATS][STRIDE], float4* dst, int rows, int tid) {
    constexpr int QPR = FLOATS / 4;      // quads per row
    static_assert(FLOATS % 4 == 0 && (QPR & (QPR - 1)) == 0, "whole quads, a power of two of them per row");
    const int quads = rows * QPR;
#pragma unroll
    for (int k = 0; k < QPR; k++) {
        const int Q = THREADS * k + tid;
        if (Q < quads) {
            const int row = Q >> __builtin_ctz(QPR), f0 = 4 * (Q & (QPR - 1));
            dst[Q] = make_float4(stage[f0][row], stage[f0 + 1][row], stage[f0 + 2][row], stage[f0 + 3][row]);
        }
    }
}

}  // namespace snk
