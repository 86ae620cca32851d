// snk_wave.hpp -- what everything else is written in: the f3 / 3x3 helpers, the wave64 primitives (DPP sums, lane
// reads and writes, the 32-lane half swap), the acquire of a wave's own stores, and the DPP reduction steps that the
// hand-written row steps splice into their inline assembly.  Uses nothing of the project.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace snk {

// ----------------------------------------------------------------------------------
// small vector helpers
// ----------------------------------------------------------------------------------
struct f3 {
    float x, y, z;
};
__device__ __forceinline__ f3 mk3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ f3 ld3(const float* p) { return mk3(p[0], p[1], p[2]); }
__device__ __forceinline__ void st3(float* p, f3 a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 operator*(f3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ f3 operator-(f3 a) { return mk3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ f3 cross(f3 a, f3 b) {
    return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// y = R v (R row-major 3x3)
__device__ __forceinline__ f3 mulRv(const float* R, f3 v) {
    return mk3(R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z,
               R[6] * v.x + R[7] * v.y + R[8] * v.z);
}
__device__ __forceinline__ f3 mulRtv(const float* R, f3 v) {
    return mk3(R[0] * v.x + R[3] * v.y + R[6] * v.z, R[1] * v.x + R[4] * v.y + R[7] * v.z,
               R[2] * v.x + R[5] * v.y + R[8] * v.z);
}
// R (row-major, body -> world) of the quaternion (x, y, z, w), which need not be normalised: THE definition of the
// rotation every kernel forms from a quaternion.  QT: the arithmetic, rounded to float32 at the end -- float everywhere
// but in the ray test's table (snk_render.hpp: scene_prims), whose records carry a column of this matrix as a hit's normal.
template <typename QT = float>
__device__ __forceinline__ void quat_rot(QT qx, QT qy, QT qz, QT qw, float* R) {
    const QT s2 = QT(2) / (qx * qx + qy * qy + qz * qz + qw * qw);
    const QT xs = qx * s2, ys = qy * s2, zs = qz * s2;
    const QT wx = qw * xs, wy = qw * ys, wz = qw * zs;
    const QT xx = qx * xs, xy = qx * ys, xz = qx * zs, yy = qy * ys, yz = qy * zs, zz = qz * zs;
    R[0] = (float)(1 - (yy + zz)); R[1] = (float)(xy - wz); R[2] = (float)(xz + wy);
    R[3] = (float)(xy + wz); R[4] = (float)(1 - (xx + zz)); R[5] = (float)(yz - wx);
    R[6] = (float)(xz - wy); R[7] = (float)(yz + wx); R[8] = (float)(1 - (xx + yy));
}
// symmetric 3x3 stored xx xy xz yy yz zz
__device__ __forceinline__ f3 mulSv(const float* S, f3 v) {
    return mk3(S[0] * v.x + S[1] * v.y + S[2] * v.z, S[1] * v.x + S[3] * v.y + S[4] * v.z,
               S[2] * v.x + S[4] * v.y + S[5] * v.z);
}
// W = R S R^T for symmetric S (body -> world), result symmetric
__device__ __forceinline__ void rotSym(const float* R, const float* S, float* W) {
    float T[9];   // T = R S
#pragma unroll
    for (int i = 0; i < 3; i++) {
        T[3 * i + 0] = R[3 * i] * S[0] + R[3 * i + 1] * S[1] + R[3 * i + 2] * S[2];
        T[3 * i + 1] = R[3 * i] * S[1] + R[3 * i + 1] * S[3] + R[3 * i + 2] * S[4];
        T[3 * i + 2] = R[3 * i] * S[2] + R[3 * i + 1] * S[4] + R[3 * i + 2] * S[5];
    }
    W[0] = T[0] * R[0] + T[1] * R[1] + T[2] * R[2];
    W[1] = T[0] * R[3] + T[1] * R[4] + T[2] * R[5];
    W[2] = T[0] * R[6] + T[1] * R[7] + T[2] * R[8];
    W[3] = T[3] * R[3] + T[4] * R[4] + T[5] * R[5];
    W[4] = T[3] * R[6] + T[4] * R[7] + T[5] * R[8];
    W[5] = T[6] * R[6] + T[7] * R[7] + T[8] * R[8];
}

// ----------------------------------------------------------------------------------
// wave primitives (wave64, DPP; gfx9 row_shr / row_bcast forms)
// ----------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float x) {
    // x + (x moved by the DPP pattern; lanes with no source or masked rows add 0)
    int y = __builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROW_MASK, 0xf, true);
    return x + __int_as_float(y);
}
// Sum over lanes 0..W-1 (W = 32 or 64), returned wave-uniform.
template <int W>
__device__ __forceinline__ float wave_sum(float x) {
    x = dpp_add<0xB1, 0xf>(x);    // quad_perm [1,0,3,2]
    x = dpp_add<0x4E, 0xf>(x);    // quad_perm [2,3,0,1]
    x = dpp_add<0x114, 0xf>(x);   // row_shr:4
    x = dpp_add<0x118, 0xf>(x);   // row_shr:8   -> lane 15 of each row = row total
    x = dpp_add<0x142, 0xa>(x);   // row_bcast:15 into rows 1,3 -> lane 31 = sum 0..31
    if (W == 64) {
        x = dpp_add<0x143, 0xc>(x);   // row_bcast:31 into rows 2,3 -> lane 63 = sum 0..63
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
    }
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 31));
}
// Sum over the active lanes 0 .. LAST (32 <= LAST < 48) of a wave running with exactly those lanes enabled, returned
// wave-uniform: the same DPP steps; lane LAST collects its own row's partial sum and the total of lanes 0 .. 31.
template <int LAST>
__device__ __forceinline__ float cols_sum(float x) {
    static_assert(LAST >= 32 && LAST < 48, "lane LAST must sit in row 2");
    x = dpp_add<0xB1, 0xf>(x);
    x = dpp_add<0x4E, 0xf>(x);
    x = dpp_add<0x114, 0xf>(x);
    x = dpp_add<0x118, 0xf>(x);
    x = dpp_add<0x142, 0xa>(x);
    x = dpp_add<0x143, 0xc>(x);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), LAST));
}
// ... and the maximum of non-negative values, same lanes
template <int LAST>
__device__ __forceinline__ float cols_max(float x) {
    static_assert(LAST >= 32 && LAST < 48, "lane LAST must sit in row 2");
    auto step = [](float v, auto ctrl, auto rows) {
        return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), decltype(ctrl)::value, decltype(rows)::value, 0xf, true)));
    };
    x = step(x, std::integral_constant<int, 0xB1>{}, std::integral_constant<int, 0xf>{});
    x = step(x, std::integral_constant<int, 0x4E>{}, std::integral_constant<int, 0xf>{});
    x = step(x, std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});
    x = step(x, std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});
    x = step(x, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});
    x = step(x, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), LAST));
}
// the lane's index within its wave (= threadIdx.x of the one-wave workgroups here), recomputed instead of kept
__device__ __forceinline__ int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// The lane index as a value the compiler cannot see through: per-lane addresses built from it are computed where they
// are used.  (Built from the kernel's own threadIdx.x they are loop-invariant, get hoisted in front of the servo loop and
// stay live across it -- twenty VGPRs in round 3's first build, which the solve's row registers then paid for with
// reloads from scratch memory inside the Gauss-Seidel loop.)
__device__ __forceinline__ int launder_lane(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}
__device__ __forceinline__ float lane_bcast(float x, int src_lane_uniform) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), src_lane_uniform));
}

// a wave-uniform condition as a scalar the compiler knows to be uniform (keeps the scheduler's loops out of
// exec-mask control flow)
__device__ __forceinline__ bool uni(bool c) { return __builtin_amdgcn_readfirstlane(c ? 1 : 0) != 0; }

struct swap2 {
    float a, b;
};
// v_permlane32_swap: returns a = [x.lo, y.lo], b = [x.hi, y.hi] (32-lane halves)
__device__ __forceinline__ swap2 half_swap(float x, float y) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    swap2 o;
    o.a = __uint_as_float(r[0]);
    o.b = __uint_as_float(r[1]);
    return o;
}
// sum over each 32-lane half; result valid in lane 31 (lower half) and lane 63 (upper half)
__device__ __forceinline__ float half_reduce(float t) {
    t = dpp_add<0xB1, 0xf>(t);
    t = dpp_add<0x4E, 0xf>(t);
    t = dpp_add<0x114, 0xf>(t);
    t = dpp_add<0x118, 0xf>(t);
    t = dpp_add<0x142, 0xa>(t);
    return t;
}
__device__ __forceinline__ float rdlane(float x, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}
// old with lane l replaced by a wave-uniform value (once per substep: a select is fine)
__device__ __forceinline__ float wrlane(float old, float v_uniform, int l) {
    return ((int)threadIdx.x == l) ? v_uniform : old;
}

// What this wave stored to its own block of global memory (constraint rows, contact geometry: written lane = row, read
// lane = column) becomes visible to its own later loads: the stores have left the wave (vmcnt) and this CU's vector L1
// holds no line from before them (buffer_inv sc1).  The XCD's L2 is the point of coherence for writer and reader alike --
// the same wave -- so nothing has to be written back: __threadfence() here (rounds 1-4) also ran buffer_wbl2, a
// write-back of every dirty line of the XCD's L2, two to three times per streamed-row substep.
//
// THE INVARIANT THIS RELIES ON (load-bearing since round 4; DESIGN.md 4 has the full producer -> consumer table): nothing
// a wave stores with PLAIN stores is ever read by ANOTHER wave inside the same launch.  Every byte that crosses waves
// in a launch -- the state record, the contact cache block, the free box's record, the substep counter at a hand-off;
// the queue entry, tickets, counters -- is stored write-through (sc1 / dwordx4 sc1) or by an agent-scope atomic, and
// ordered by s_waitcnt vmcnt(0) in front of the queue entry (sched_push).  The L2 write-back that __threadfence() did
// here as a side effect is therefore not needed by any reader; a new cross-wave datum must come with its own
// write-through stores, not lean on this function.
// gfx942 / gfx950 ISA only: `vmcnt` counts stores there, and `buffer_inv sc1` is this family's L1 invalidate.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__)
#error "own_stores_visible(): written for gfx942 / gfx950 (vmcnt covers stores, buffer_inv sc1); other targets need __threadfence()"
#endif
__device__ __forceinline__ void own_stores_visible() {
    asm volatile("s_waitcnt vmcnt(0)\n\tbuffer_inv sc1\n\ts_waitcnt vmcnt(0)" ::: "memory");
}

// one DPP step of six independent reductions (operands a .. f)
#define SNK_RED64x6_STEP(MODE)                              \
    "v_add_f32_dpp %[a], %[a], %[a] " MODE "\n\t"            \
    "v_add_f32_dpp %[b], %[b], %[b] " MODE "\n\t"            \
    "v_add_f32_dpp %[c], %[c], %[c] " MODE "\n\t"            \
    "v_add_f32_dpp %[d], %[d], %[d] " MODE "\n\t"            \
    "v_add_f32_dpp %[e], %[e], %[e] " MODE "\n\t"            \
    "v_add_f32_dpp %[f], %[f], %[f] " MODE "\n\t"
// (seven: operand g as well)
#define SNK_RED64x7_STEP(MODE) SNK_RED64x6_STEP(MODE) "v_add_f32_dpp %[g], %[g], %[g] " MODE "\n\t"

// one 64-lane sum of register T, with the wait states a dependent DPP read needs
#define SNK_RED64(T)                                                                                   \
    "v_add_f32_dpp " T ", " T ", " T " quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"  \
    "s_nop 1\n\t"                                                                                      \
    "v_add_f32_dpp " T ", " T ", " T " quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"  \
    "s_nop 1\n\t"                                                                                      \
    "v_add_f32_dpp " T ", " T ", " T " row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"          \
    "s_nop 1\n\t"                                                                                      \
    "v_add_f32_dpp " T ", " T ", " T " row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"          \
    "s_nop 1\n\t"                                                                                      \
    "v_add_f32_dpp " T ", " T ", " T " row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"                    \
    "s_nop 1\n\t"                                                                                      \
    "v_add_f32_dpp " T ", " T ", " T " row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
// one DPP step of two independent reductions: each instruction is the other's wait state
#define SNK_RED64x2_STEP(A, B, MODE)                    \
    "v_add_f32_dpp " A ", " A ", " A " " MODE "\n\t"      \
    "v_add_f32_dpp " B ", " B ", " B " " MODE "\n\t"      \
    "s_nop 0\n\t"

}  // namespace snk
