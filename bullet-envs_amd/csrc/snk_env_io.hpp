// snk_env_io.hpp -- an environment's way between global memory and the LDS image: the state record, the contact cache
// and the free box (plain or write-through, for a hand-off between waves), the per-workgroup / per-environment blocks,
// the observation row, the reset-pose table and the soft reset.
#pragma once
#include "snk_contacts.hpp"
#include "snk_lds.hpp"
#include "snk_wave.hpp"

namespace snk {

// ----------------------------------------------------------------------------------
// record <-> LDS, observation packing (snake.py:209-217)
// ----------------------------------------------------------------------------------
template <class LT>
__device__ __forceinline__ void load_rec(LT& L, const float* __restrict__ rec, int lane) {
    lane = launder_lane(lane);
    for (int i = lane; i < LT::REC; i += 64) L.rec[i] = rec[i];
    lds_sync();
}
// THROUGH: the same store, write-through (sc1): the record leaves this XCD's L2 for memory at once, so a wave on another
// XCD can take the env-step over after an agent-scope acquire without this wave writing its whole L2 back
// (MI355X_MICROARCH.md, inter-workgroup visibility: every handed-off byte stored sc1 and drained with
// s_waitcnt vmcnt(0) before the flag needs no agent release).  One 16-byte store per lane.
template <class LT, bool THROUGH = false>
__device__ __forceinline__ void store_rec(LT& L, float* __restrict__ rec, int lane) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    lane = launder_lane(lane);
    lds_sync();
    if constexpr (THROUGH) {
        if (lane < LT::REC / 4) {
            const v4f v = reinterpret_cast<const v4f*>(L.rec)[lane];
            asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(rec + 4 * lane), "v"(v) : "memory");
        }
    } else {
        for (int i = lane; i < LT::REC; i += 64) rec[i] = L.rec[i];
    }
}
// The register-resident kernels keep an environment's contact manifolds (contact_model 1) in LDS while a wave holds
// it (Lds<N, true>::mfl); these move them from / to the environment's block of global memory
// ([2n][kMfFloats] = per cylinder [count, 3 pad, 4 x (a3, b.x, b.y, lambda)]) together with the state record.
// An environment's cache is one contiguous block: 2n cylinders x kMfFloats = 28 floats = 224 quads of 16 bytes (3.5 KB for 16
// links).  It travels in four wave-wide dwordx4 instructions, instruction k moving quads 64 k .. 64 k + 63: 1 KB of
// consecutive bytes, so every 128-byte line is written WHOLE by one store instruction -- the form MI355X_MICROARCH.md's
// hand-off table lists for write-through stores another XCD's wave then loads (a first version gave every lane the quads
// of "its" cylinder: lines assembled from four instructions' pieces, and results began to depend on where a launch
// handed env-steps over).  Quad Q holds floats 4 (Q % 7) .. + 3 of cylinder Q / 7's block [count, 3 pad, 4 x 6].
// (Round 3 moved only the LIVE floats, one write-through dword per lane and instruction: less payload, but every such store
// is a memory request of its own -- ~240 per hand-off, counted at 64 bytes each: 53 of the 82 MB that WRITE_SIZE showed per
// launch, and 42 of the 66 MB of FETCH_SIZE, were this (profiles/r04_write_size_suspects.txt).)  Slots beyond a
// cylinder's count are written as zeros, by every store alike, so what the block holds does not depend on the schedule.
template <class LT>
__device__ __forceinline__ void load_mf(LT& L, const float* __restrict__ mf, int lane) {
    if constexpr (LT::kV2) {
        if (mf) {
            lane = launder_lane(lane);
            typedef float v4f __attribute__((ext_vector_type(4)));
            constexpr int kQuads = 2 * LT::kN * kMfFloats / 4;
#pragma unroll
            for (int k = 0; k < (kQuads + 63) / 64; k++) {
                const int Q = 64 * k + lane;
                if (Q < kQuads) {
                    const v4f q = reinterpret_cast<const v4f*>(mf)[Q];
                    const int c = Q / 7, part = Q - 7 * c;
                    const float f[4] = {q.x, q.y, q.z, q.w};
                    if (part == 0) L.mfn[c] = (unsigned char)(f[0] < 0.f ? 0.f : (f[0] > 4.f ? 4.f : f[0]));
                    else {
#pragma unroll
                        for (int e = 0; e < 4; e++) L.mfl[4 * part - 4 + e][c] = f[e];
                    }
                }
            }
            lds_sync();
        }
    }
}
template <class LT, bool THROUGH>
__device__ __forceinline__ void store_mf(LT& L, float* __restrict__ mf, int lane) {
    if constexpr (LT::kV2) {
        if (mf) {
            lane = launder_lane(lane);
            lds_sync();
            typedef float v4f __attribute__((ext_vector_type(4)));
            constexpr int kQuads = 2 * LT::kN * kMfFloats / 4;
#pragma unroll
            for (int k = 0; k < (kQuads + 63) / 64; k++) {
                const int Q = 64 * k + lane;
                if (Q < kQuads) {
                    const int c = Q / 7, part = Q - 7 * c;
                    const int cnt = (int)L.mfn[c];
                    v4f v;
                    if (part == 0) {
                        v.x = (float)cnt; v.y = 0.f; v.z = 0.f; v.w = 0.f;
                    } else {
                        const int f0 = 4 * part - 4;          // first of the four floats of mfl this quad holds
                        v.x = f0 < 6 * cnt ? L.mfl[f0][c] : 0.f;
                        v.y = f0 + 1 < 6 * cnt ? L.mfl[f0 + 1][c] : 0.f;
                        v.z = f0 + 2 < 6 * cnt ? L.mfl[f0 + 2][c] : 0.f;
                        v.w = f0 + 3 < 6 * cnt ? L.mfl[f0 + 3][c] : 0.f;
                    }
                    float* dst = mf + 4 * Q;
                    if (THROUGH) asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(dst), "v"(v) : "memory");
                    else *reinterpret_cast<v4f*>(dst) = v;
                }
            }
        }
    }
}
// obstacle 2: the free box of the environment (state 13, point count, manifold 24: kBoxFloats per env in d_box) travels
// with the state record, like the contact cache
// (64 floats = 256 bytes per environment: two 128-byte lines of its own, written whole by the one store instruction of a
//  hand-off -- MI355X_MICROARCH.md's form for write-through stores another XCD's wave loads; at 40 floats an env's tail shared
//  a line with its neighbour's head)
constexpr int kBoxFloats = 64;
template <class LT>
__device__ __forceinline__ void load_box(LT& L, const float* __restrict__ bx, int lane) {
    if constexpr (!LT::kV2) {
        if (bx) {
            lane = launder_lane(lane);
            if (lane < 13) L.box[lane] = bx[lane];
            else if (lane == 13) L.bmn = (int)bx[13];
            else if (lane < 38) L.bman[lane - 14] = bx[lane];
            lds_sync();
        }
    }
}
template <class LT, bool THROUGH>
__device__ __forceinline__ void store_box(LT& L, float* __restrict__ bx, int lane) {
    if constexpr (!LT::kV2) {
        if (bx) {
            lane = launder_lane(lane);
            lds_sync();
            {
                const float v = lane < 13 ? L.box[lane] : (lane == 13 ? (float)L.bmn : (lane < 38 ? L.bman[lane - 14] : 0.f));
                if (THROUGH) asm volatile("global_store_dword %0, %1, off sc1" : : "v"(bx + lane), "v"(v) : "memory");
                else bx[lane] = v;
            }
        }
    }
}
// obstacle 2: the plane's coefficient of the environment a wave has just loaded, for find_box_ground_v1 (nothing without a
// free box: box_all is null)
template <class LT>
__device__ __forceinline__ void set_box_plane_mu(LT& L, const float* __restrict__ box_all, float mu_plane, int lane) {
    if constexpr (!LT::kV2 && LT::kN <= 16) {
        if (box_all && lane == 0) L.bmu = mu_plane;
    }
}
// the workgroup's block of streamed constraint rows (one per resident wave): the streamed-row solve's, and behind the
// register-resident one, for the substeps whose contacts outgrow its slots (substep())
template <int N>
__device__ __forceinline__ float* rows_of(float* __restrict__ rows_all) {
    return rows_all + (size_t)blockIdx.x * Lds<N, false>::kRowFloats;
}
// env's block of the contact caches (null under contact_model 0) and of the free boxes (null without obstacle 2)
template <int N>
__device__ __forceinline__ float* cache_of(float* __restrict__ mf_all, int env) {
    return mf_all ? mf_all + (size_t)env * (2 * N * kMfFloats) : nullptr;
}
__device__ __forceinline__ float* box_of(float* __restrict__ box_all, int env) {
    return box_all ? box_all + (size_t)env * kBoxFloats : nullptr;
}
// everything of env that a wave holds in LDS while it runs the env: record, contact cache, free box.  THROUGH: stored
// write-through, for a hand-off to a wave on another XCD (store_rec)
template <class LT>
__device__ __forceinline__ void load_env(LT& L, const float* __restrict__ recs, float* __restrict__ mf_all,
                                         float* __restrict__ box_all, int env, int lane) {
    load_rec(L, recs + (size_t)env * LT::REC, lane);
    load_mf(L, cache_of<LT::kN>(mf_all, env), lane);
    load_box(L, box_of(box_all, env), lane);
}
template <class LT, bool THROUGH>
__device__ __forceinline__ void store_env(LT& L, float* __restrict__ recs, float* __restrict__ mf_all,
                                          float* __restrict__ box_all, int env, int lane) {
    store_rec<LT, THROUGH>(L, recs + (size_t)env * LT::REC, lane);
    store_mf<LT, THROUGH>(L, cache_of<LT::kN>(mf_all, env), lane);
    store_box<LT, THROUGH>(L, box_of(box_all, env), lane);
}
template <class LT>
__device__ __forceinline__ void write_obs(LT& L, float* __restrict__ obs, int lane) {
    constexpr int N = LT::kN;
    lane = launder_lane(lane);
    // obs = [q, qd, tau_motor | pos3 quat4 | fz]; rec = [pos3 quat4 w3 v3 | q qd taum | fz px]
    for (int i = lane; i < 3 * N + 8; i += 64) {
        float x;
        if (i < 3 * N) x = L.rec[13 + i];
        else if (i < 3 * N + 7) x = L.rec[i - 3 * N];
        else x = L.rec[13 + 3 * N];
        obs[i] = x;
    }
}
// The reset-pose table (snk_set_reset_pose): one row per environment, [pos 3 | quat xyzw 4 | q n | padding], kResetRow
// floats = whole 128-byte lines (32 floats for 16 links, 64 for 32).  What Snake.initPosition, initOrientation and
// initState are to the reference's soft reset (snake.py:22-24).
template <int N>
constexpr int kResetRow = (7 + N + 31) / 32 * 32;
template <int N>
__device__ __forceinline__ const float* reset_row_of(const float* __restrict__ reset_all, int env) {
    return reset_all + (size_t)env * kResetRow<N>;
}
// `row`: the environment's row of the reset-pose table.  Only the wave that ends the episode reads it, and nothing
// writes the table inside a launch: plain loads.
template <class LT>
__device__ __forceinline__ void soft_reset(LT& L, const float* __restrict__ row, int lane) {
    constexpr int N = LT::kN;
    lane = launder_lane(lane);
    // snake.py:96-99,119-127: resetBasePositionAndOrientation(initPosition, initOrientation) -- which zeroes the base
    // twist [U] -- and resetJointState(initState[j]) for every motor (qd = 0); motor-torque and sensor caches persist [U]
    for (int i = lane; i < 13 + 2 * N; i += 64) {
        float v = 0.0f;
        if (i < 7) v = row[i];
        else if (i >= 13 && i < 13 + N) v = row[i - 6];
        L.rec[i] = v;
    }
}

}  // namespace snk
