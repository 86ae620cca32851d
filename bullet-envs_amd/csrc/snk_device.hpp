// snk_device.hpp -- gfx950 device code of the batched snake stepper.
//
// ONE WAVEFRONT (64 lanes) PER ENVIRONMENT, one wave per workgroup.  The env's state
// record is loaded coalesced from HBM into LDS once per env-step and written back once;
// every physics substep (0..41 per env-step, snake.py:284-304) runs on chip.
//
// Formulation (differs on purpose from oracle/): the chain of n+1 composite bodies is
// described in WORLD-ALIGNED axes with each body's quantities referenced to its own joint
// origin o_b, and classical accelerations [alpha_b ; a(o_b)].  Transfers between
// neighbouring bodies are then pure translations by r_b = o_b - o_{b-1}; the joint
// subspace is S_b = [axis_b ; 0].  Articulated-body algorithm = Featherstone's three
// sweeps in those coordinates.
//
// What replaces what (reference call sites):
//   env_step_kernel      SnakeGymEnv.step (SnakeGymEnv.py:33-50) + Snake.step servo loop
//                        (snake.py:274-306) + worker auto-reset (multiprocessing_env.py:13-15)
//   substep()            pybullet.stepSimulation (snake.py:286) after
//                        setJointMotorControlArray(POSITION_CONTROL) (snake.py:221)
//   write_obs()          Snake.getObservation (snake.py:209-217)
//   mean_height()        Snake.checkSnakeHeight (snake.py:237-245)
//
// Layers, bottom to top (each header includes what it uses, nothing that comes later):
//   snk_wave.hpp      f3 / 3x3 helpers, wave64 primitives, own_stores_visible, DPP reduction steps
//   snk_lds.hpp       the LDS images Lds<N, V2>, the solver-rules variants, the -D knobs
//   snk_dynamics.hpp  FK, bias forces, ABA, sensor_pass_needed, step_base_pose
//   snk_contacts.hpp  rim point, friction directions, persistent manifolds: shared by both solves
//   snk_selfcol.hpp   link-link and obstacle contacts (GJK)
//   snk_freebox.hpp   obstacle 2, the free box
//   snk_pgs_v1.hpp    the streamed-row solve and its substep
//   snk_pgs_v2.hpp    the register-resident solve and its substep
//   snk_env_io.hpp    record / contact cache / box movers, write_obs, soft_reset
//   snk_sched.hpp     launch plan, in-launch scheduler
//   this file         the dispatch between the two solves, StepArgs, the kernels, the self test
#pragma once
#include <hip/hip_runtime.h>

#include "snk_model.hpp"
#include "snk_wave.hpp"
#include "snk_lds.hpp"
#include "snk_dynamics.hpp"
#include "snk_contacts.hpp"
#include "snk_selfcol.hpp"
#include "snk_freebox.hpp"
#include "snk_pgs_v1.hpp"
#include "snk_pgs_v2.hpp"
#include "snk_env_io.hpp"
#include "snk_sched.hpp"

namespace snk {

// snk_contact_overflow's three counters, then the histogram of contact points per physics substep (kHistBins values;
// a 32-link snake's manifolds hold 256 ground points at most, plus 32 link-link / obstacle contacts)
constexpr int kOvfCounters = 3;
constexpr int kHistBins = 320;

// One out-of-line copy of the streamed-row substep for the register-resident kernels' rare substeps (below): inlined
// there it would double those kernels; the streamed-row kernels themselves inline it (as a called function its LDS
// accesses go through flat addresses: -10 % on those kernels when the compiler chose that by itself, round 3).
#ifdef SNK_V1_INLINE
#define SNK_V1_CALL_ATTR __forceinline__
#else
#define SNK_V1_CALL_ATTR __noinline__
#endif
template <class LT>
__device__ SNK_V1_CALL_ATTR void substep_v1_call(LT& L, const DevModel& M, int lane, float mu, int& iters, int& ncontacts,
                                             float* __restrict__ rows, const SensorHint& hint, float* __restrict__ mf,
                                             unsigned long long* __restrict__ ovf) {
    substep_v1<LT, true>(L, M, lane, mu, iters, ncontacts, rows, hint, mf, ovf);
}

template <class LT>
__device__ __forceinline__ void substep(LT& L, const DevModel& M0, int lane_in, float mu, int& iters, int& ncontacts,
                                        const SensorHint& hint, float* __restrict__ rows, float* __restrict__ mf,
                                        unsigned long long* __restrict__ ovf) {
    int lane = lane_in;
    // Launder the model pointer once per substep: otherwise ~100 per-lane model constants are
    // hoisted out of the substep loop and stay live (or spilled) across the whole solve.
    const DevModel* Mq = &M0;
    asm volatile("" : "+s"(Mq));
    const DevModel& M = *Mq;
    // ... and the lane id: hundreds of per-lane LDS addresses are loop-invariant and would
    // otherwise be computed in the kernel prologue and spilled.
    asm volatile("" : "+v"(lane));
    if constexpr (LT::kV2) {
        substep_v2(L, M, lane, mu, iters, ncontacts, hint, ovf);
        if (ncontacts < 0) {
            // The contacts of this pose do not fit the register-resident solve's 64 slots (a snake at rest gathers up to
            // four points per cylinder: 128; Bullet has no limit).  Nothing has been touched yet: THIS substep goes through
            // the streamed-row solve of the same chain instead (128 + 32 slots: every point a 16-link snake's manifolds
            // can hold), in place -- the two LDS images share their first members (record, poses, ABA workspace), the
            // contact cache travels through its block of global memory, where the streamed-row kernels keep it.  The
            // rule is per substep and a function of the state alone, so results do not depend on the schedule, and the
            // single-substep API takes the same path.  Counted (snk_contact_overflow[0]), never silent.
            using L1 = LdsFor<LT::kN, false, LT::kNCO ? 2 : (LT::kERP ? 1 : 0)>;
            static_assert(sizeof(L1) <= sizeof(LT), "the streamed-row image must fit the register-resident one's allocation");
            L1& Lx = *reinterpret_cast<L1*>(&L);
            // The cache goes out with plain stores and this CU's vector L1 is invalidated behind them (what an agent-scope
            // acquire does: s_waitcnt vmcnt(0), buffer_inv sc1) before the streamed-row substep loads it, and again before it
            // comes back.  Round 4: with write-through (sc1) stores and no invalidate, the loads that followed could hit
            // lines this CU had cached when the environment was loaded -- an sc1 store does not refresh the storing CU's
            // own L1 -- and a few cylinders' manifolds came back one substep old: 64 against 65 contacts among replicas of
            // one state, whenever the line had survived (tools/dbg/replica_sub.py; it took other ring sizes in the
            // streamed solve, i.e. other timing, to show in test_schedule_does_not_change_results).
            store_mf<LT, false>(L, mf, lane);
            own_stores_visible();
            if (M.poison) { lds_sync(); Lx.poison_own(lane); lds_sync(); }
            substep_v1_call(Lx, M, launder_lane(lane), mu, iters, ncontacts, rows, hint, mf, ovf);
            own_stores_visible();
            load_mf(L, mf, lane);
        }
    } else {
        substep_v1(L, M, lane, mu, iters, ncontacts, rows, hint, mf, ovf);
    }
    // contact points of this substep, counted per value (snk_contact_histogram): what decides how many row slots a
    // register-resident solve needs.  One fire-and-forget atomic per substep (every lane with its own operand, folded
    // into one memory operation: see sched_pop for why there is no `if (lane == 0)`).
    // Off unless snk_contact_histogram_enable asked for it: always on it cost 0.7 % of the headline (A/B on one box, three
    // runs each: 361.1-362.1 k against 363.8-364.0 k env-steps/s).
#ifndef SNK_HIST_MODE
#define SNK_HIST_MODE 2
#endif
#if SNK_HIST_MODE == 2
    if (M.hist)
#elif SNK_HIST_MODE == 0
    if (false)
#endif
    {
        int bin = __builtin_amdgcn_readfirstlane(ncontacts);
        bin = bin < 0 ? 0 : (bin > kHistBins - 1 ? kHistBins - 1 : bin);
        atomicAdd(ovf + kOvfCounters + bin, lane_id() == 0 ? 1ull : 0ull);
    }
}

// ----------------------------------------------------------------------------------
// kernels
// ----------------------------------------------------------------------------------
template <int N, bool V2, int RULES = 0>
__global__ __launch_bounds__(64, 2) void substep_kernel(const DevModel* __restrict__ Mp, float* __restrict__ recs,
                                                     const float* __restrict__ mu_plane,
                                                     const float* __restrict__ targets, int k,
                                                     int32_t* __restrict__ info, int n_envs, float* __restrict__ rows_all,
                                                     float* __restrict__ mf_all, unsigned long long* __restrict__ ovf,
                                                     float* __restrict__ box_all,
                                                     const uint8_t* __restrict__ active) {
    extern __shared__ float4 smem_raw[];
    using LT = LdsFor<N, V2, RULES>;
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    const DevModel& M = *Mp;
    const int lane = threadIdx.x;
    for (int env = blockIdx.x; env < n_envs; env += gridDim.x) {      // (the block of streamed rows belongs to the workgroup)
    // snk_substep's mask (null: every env): an env whose byte is 0 is neither loaded nor stored -- record, contact cache,
    // free box and info row keep their bits
    if (active && !active[env]) continue;
    if (M.poison) { L.poison(lane); lds_sync(); }
    load_env(L, recs, mf_all, box_all, env, lane);
    if (lane < N) L.targets[lane] = targets[(size_t)env * N + lane];
    lds_sync();
    const float mup = mu_plane[env];
    float mu = fminf(M.mu_link * mup, 10.0f);
    set_box_plane_mu(L, box_all, mup, lane);
    fk_vel(L, M, lane);
    int iters = 0, nc = 0;
    SensorHint hint;
    hint.always = true; hint.counter_next = 0; hint.h_prev = 0.f;
    float* env_rows = rows_of<N>(rows_all);
    float* env_mf = cache_of<N>(mf_all, env);
    for (int s = 0; s < k; s++) substep(L, M, lane, mu, iters, nc, hint, env_rows, env_mf, ovf);
    if (info && lane == 0) { info[2 * env] = iters; info[2 * env + 1] = nc; }
    store_env<LT, false>(L, recs, mf_all, box_all, env, lane);
    lds_sync();
    }
}

template <int N, bool V2>
__global__ __launch_bounds__(64) void reset_kernel(float* __restrict__ recs, const uint8_t* __restrict__ mask,
                                                   float* __restrict__ obs, const float* __restrict__ reset_all, int hard,
                                                   int n_envs) {
    extern __shared__ float4 smem_raw[];
    using LT = Lds<N, V2>;
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    const int env = blockIdx.x;
    const int lane = threadIdx.x;
    if (env >= n_envs) return;
    if (mask && !mask[env]) return;
    load_rec(L, recs + (size_t)env * LT::REC, lane);
    soft_reset(L, reset_row_of<N>(reset_all, env), lane);
    lds_sync();
    if (hard) {
        for (int i = 13 + 2 * N + lane; i < LT::REC; i += 64) L.rec[i] = 0.f;
        lds_sync();
    }
    if (lane == 0) L.prev_x() = L.rec[0];   // _observation = reset obs (SnakeGymEnv.py:30): the pose's x
    lds_sync();
    if (obs) write_obs(L, obs + (size_t)env * (3 * N + 8), lane);
    store_rec(L, recs + (size_t)env * LT::REC, lane);
}

// snk_set_reset_pose_dev: rows of the caller's dense [n_envs][7 + N] device buffer into the padded table, for the envs
// whose mask byte is set (null: all).  One thread per float of the payload; a row's padding is never touched.
template <int N>
__global__ __launch_bounds__(256) void reset_pose_copy_kernel(float* __restrict__ reset_all, const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ pose, int n_envs) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t env = t / (7 + N);
    const int i = (int)(t - env * (7 + N));
    if (env >= (size_t)n_envs) return;
    if (mask && !mask[env]) return;
    reset_all[env * kResetRow<N> + i] = pose[t];
}

template <int N, bool V2>
__global__ __launch_bounds__(64) void obs_kernel(const DevModel* __restrict__ Mp, const float* __restrict__ recs,
                                                 float* __restrict__ obs, float* __restrict__ height,
                                                 float* __restrict__ linkpos, int n_envs) {
    extern __shared__ float4 smem_raw[];
    using LT = Lds<N, V2>;
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    const DevModel& M = *Mp;
    const int env = blockIdx.x;
    const int lane = threadIdx.x;
    if (env >= n_envs) return;
    load_rec(L, recs + (size_t)env * LT::REC, lane);
    if (obs) write_obs(L, obs + (size_t)env * (3 * N + 8), lane);
    if (height || linkpos) {
        fk_vel(L, M, lane);
        if (height) {
            float h = mean_height(L, M, lane);
            if (lane == 0) height[env] = h;
        }
        if (linkpos && lane <= N) {
            // getLinkPositions (snake.py:138-146): COM of Bullet links 0,3,...,3n -- the `base` link and
            // the OUTPUT_BODY links (COM at their joint origin) -- as [x.., y.., z..]
            f3 c = ld3(L.o[lane]);
            if (lane == 0) c = c + mulRv(L.R[0], ld3(M.hbase));
            float* out = linkpos + (size_t)env * 3 * (N + 1);
            out[lane] = c.x; out[(N + 1) + lane] = c.y; out[2 * (N + 1) + lane] = c.z;
        }
    }
}

// Arguments of the scheduled step kernel: ONE struct, passed by value -- i.e. it IS the kernel-argument segment -- and
// read through step_args(), a pointer to that segment the compiler cannot see through, at the place of use.  Passed
// as ordinary kernel arguments these twenty pointers are loaded once at kernel entry and then sit in scalar registers
// for the whole launch; the register-resident solve has none to spare, so ~190 of them were spilled into lanes of FOUR
// vector registers, which the solve's row registers then paid for with reloads from scratch memory inside the
// Gauss-Seidel loop (round-3 ISA).  Read where needed, a pointer lives for a few instructions.
struct StepArgs {
    float* recs;
    const float* mu_plane;
    float* actions;
    float* obs;
    float* rew;
    uint8_t* done;
    int32_t* substeps;
    float* rows_all;
    float* mf_all;
    unsigned long long* ovf;
    float* box_all;
    Sched sc;
    int32_t model_slot, vec_mode, n_envs;
    // obs row stride in floats (3n + 8 for the dense [n_envs x obs_dim] output).  packed != 0 (snk_step_packed): reward
    // and done flag of env e go into its obs row, at float index obs_dim (f32) and obs_dim + 1 (u32 0 / 1), instead of
    // rew[] / done[]: one [n_envs x stride] buffer that a sharded vector env gathers as it is (device_env.py)
    int32_t obs_stride, packed, pad_;
    // the unscheduled kernel (env_step_kernel) only: its model, and plan_kernel's order (null: launch order).  Appended,
    // so that the scheduled kernel's offsets stay as they were
    const DevModel* model;
    const int32_t* order;
    // the TRACE kernels only (snk_step_traced): one row per physics substep of every env-step, row s of env e at
    // trace[(e * trace_rows + s) * trace_stride] (write_trace_row).  Appended, like the two above
    float* trace;
    int32_t trace_rows, trace_stride;
    // the reset-pose table (snk_set_reset_pose): [n_envs][kResetRow<N>], read by finish_env_step when an episode ends.
    // Appended, like the three above
    const float* reset_all;
};
typedef const StepArgs __attribute__((address_space(4))) * StepArgPtr;
__device__ __forceinline__ StepArgPtr step_args() {
    StepArgPtr p = (StepArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
__device__ __forceinline__ Sched load_sched(StepArgPtr p) {
    Sched sc;
    sc.head = p->sc.head; sc.tail = p->sc.tail; sc.ent = p->sc.ent; sc.waiting = p->sc.waiting;
    sc.counter = p->sc.counter; sc.finished = p->sc.finished; sc.alarm = p->sc.alarm;
    sc.cap = p->sc.cap; sc.quantum = p->sc.quantum; sc.hyst = p->sc.hyst; sc.wstat = p->sc.wstat;
    return sc;
}

// Start of an env-step: checkBound (SnakeGymEnv.py:82-88) clips the caller's array in place, createAction
// (snake.py:247-269) + convertActionToJointCommand (snake.py:223-225) set the joint targets.
template <class LT>
__device__ __forceinline__ void set_targets(LT& L, const DevModel& M, float* __restrict__ actions, int env, int lane) {
    constexpr int N = LT::kN;
    const int A = M.act_dim;
    float act = 0.f;
    if (lane < A) {
        act = actions[(size_t)env * A + lane];
        float cl = fminf(fmaxf(act, -1.0f), 1.0f);
        if (cl != act) actions[(size_t)env * A + lane] = cl;
        act = cl;
    }
    if (lane < N) L.targets[lane] = 0.f;
    lds_sync();
    if (lane < A) {
        int slot = (M.gait == 0) ? 2 * lane : ((M.gait == 1) ? 2 * lane + 1 : lane);
        L.targets[slot] = act * M.scaling;
    }
    lds_sync();
}

// End of an env-step whose servo loop ran `counter` substeps: SnakeGymEnv.step (SnakeGymEnv.py:36-42).  The outputs
// are read through `af` here, at the place of use (StepArgs).
template <class LT>
__device__ __forceinline__ void finish_env_step(LT& L, const DevModel& M, StepArgPtr af, int env, int lane, int counter,
                                                bool end_height) {
    constexpr int N = LT::kN;
    float en = (lane < N) ? L.qd()[lane] * L.taum()[lane] * M.energy_dt : 0.f;   // snake.py:336-341
    float energy = wave_sum<64>(en);
    float x = L.rec[0], y = L.rec[1], fzv = L.fz();
    float r = M.alpha * (x - L.prev_x()) + (fabsf(fzv) > M.coll_force ? M.coll_pen : 0.f) - M.beta * fabsf(y) -
              M.gamma * energy;
    bool dn = uni(fabsf(L.rec[13 + M.term_index]) > M.term_angle);
    if (!dn) dn = uni(mean_height(L, M, lane) > M.height_thr);
    if (!dn) dn = end_height;
    if (dn) r += M.done_pen;
    const int vec_mode = af->vec_mode;
    float* ob = af->obs + (size_t)env * af->obs_stride;
    if (!(dn && vec_mode)) write_obs(L, ob, lane);
    lds_sync();
    if (dn) {
        soft_reset(L, reset_row_of<N>(af->reset_all, env), lane);
        lds_sync();
        if (vec_mode) write_obs(L, ob, lane);   // worker returns env.reset()'s obs
    }
    lds_sync();
    if (lane == 0) {
        // _observation = terminal obs (SnakeGymEnv.py:42); the worker's reset() refreshes it (the reset pose's x, which
        // soft_reset has just put into the record)
        L.prev_x() = (dn && vec_mode) ? L.rec[0] : x;
        if (af->packed) {       // snk_step_packed: [obs | reward | done] rows (StepArgs::packed)
            ob[3 * N + 8] = r;
            reinterpret_cast<uint32_t*>(ob)[3 * N + 9] = dn ? 1u : 0u;
        } else {
            af->rew[env] = r;
            af->done[env] = dn ? 1 : 0;
        }
        int32_t* substeps = af->substeps;
        if (substeps) substeps[env] = counter;
    }
}

// Test-mode telemetry (snake.py:292-293: step_internal_observations.append(getObservation()),
// link_positions.append(getLinkPositions()) after every stepSimulation; SnakeGymEnv.py:43-44 hands the lists out as
// info): the TRACE kernels write row `row` = counter - 1 of env after each substep,
//   [ obs (3n + 8, write_obs's) | link positions 3 (n + 1) as x_0..x_n, y_0..y_n, z_0..z_n (obs_kernel's formula) | padding ].
// Both substeps end in fk_vel (snk_pgs_v1.hpp, snk_pgs_v2.hpp; the streamed-row substep a register-resident wave calls
// for its rare substeps works on the same first members of the image), whose closing lds_sync leaves L.rec, L.o and
// L.R[0] current: what mean_height reads right behind this.  The row stride is a whole number of 128-byte lines and the
// buffer is aligned to one (snk_step_traced checks both), so a row's lines are written by the one wave that ran its
// substep, whoever ran the substeps before and after a hand-off (a wave owns whole lines).  Plain stores:
// nothing reads a row inside the launch.  The padding and the rows from the env's count on are never touched.
template <class LT>
__device__ __forceinline__ void write_trace_row(LT& L, const DevModel& M, StepArgPtr a, int env, int row, int lane) {
    constexpr int N = LT::kN;
    const int rows = a->trace_rows;
    if (row < 0 || row >= rows) return;        // never: counter <= max_counter + 1 <= trace_rows (snk_step_traced)
    float* out = a->trace + ((size_t)env * rows + row) * a->trace_stride;
    write_obs(L, out, lane);
    lane = launder_lane(lane);
    if (lane <= N) {
        f3 c = ld3(L.o[lane]);
        if (lane == 0) c = c + mulRv(L.R[0], ld3(M.hbase));
        float* lp = out + (3 * N + 8);
        lp[lane] = c.x; lp[(N + 1) + lane] = c.y; lp[2 * (N + 1) + lane] = c.z;
    }
}

// Whole env-steps in launch order, without the scheduler: SNK_QUANTUM=0, and the handles that find no model slot.
// TRACE (snk_step_traced): a trace row after every substep, and the sensor pass on every substep (hint.always, as
// substep_kernel has it), so that every row's obs[3n + 7] and motor torques are that substep's own.
template <int N, bool V2, int RULES = 0, bool TRACE = false>
__global__ __launch_bounds__(64, 2) void env_step_kernel(StepArgs args_by_value) {
    (void)args_by_value;            // read through step_args() only
    extern __shared__ float4 smem_raw[];
    using LT = LdsFor<N, V2, RULES>;
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    const DevModel& M = *step_args()->model;
    // longest-first schedule: workgroup b takes the envs with the b-th, (b + G)-th, ... largest predicted work (G
    // workgroups: as many as the chip holds at once; the block of streamed constraint rows belongs to the WORKGROUP)
    for (int slot_ = blockIdx.x; slot_ < step_args()->n_envs; slot_ += gridDim.x) {
    const StepArgPtr ap = step_args();
    const int32_t* order = ap->order;
    const int env = order ? __builtin_amdgcn_readfirstlane(order[slot_]) : slot_;
    const int lane = threadIdx.x;
    if (M.poison) { L.poison(lane); lds_sync(); }
    load_env(L, ap->recs, ap->mf_all, ap->box_all, env, lane);
    set_targets(L, M, ap->actions, env, lane);
    const float mup = ap->mu_plane[env];
    float mu = fminf(M.mu_link * mup, 10.0f);
    set_box_plane_mu(L, ap->box_all, mup, lane);
    float* env_rows = rows_of<N>(ap->rows_all);
    float* env_mf = cache_of<N>(ap->mf_all, env);
    unsigned long long* ovf = ap->ovf;
    fk_vel(L, M, lane);
    // Snake.step servo loop (snake.py:283-304)
    int counter = 0;
    bool end_height = false;
    int it_dummy = 0, nc_dummy = 0;
    SensorHint hint;
    hint.always = TRACE;
    hint.h_prev = mean_height(L, M, lane);
    while (true) {
        float e = (lane < N) ? (L.targets[lane] - L.q()[lane]) : 0.f;
        float nrm = sqrtf(wave_sum<64>(e * e));
        if (!(nrm > M.servo_tol)) break;
        hint.counter_next = counter + 1;
        substep(L, M, lane, mu, it_dummy, nc_dummy, hint, env_rows, env_mf, ovf);
        counter++;
        if constexpr (TRACE) write_trace_row(L, M, step_args(), env, counter - 1, lane_id());
        hint.h_prev = mean_height(L, M, lane);
        if (hint.h_prev > M.height_thr) { end_height = true; break; }
        if (counter > M.max_counter) break;
    }
    const StepArgPtr af = step_args();
    finish_env_step(L, M, af, env, lane, counter, end_height);
    store_env<LT, false>(L, af->recs, af->mf_all, af->box_all, env, lane);
    lds_sync();
    }
}

// TRACE: as in env_step_kernel.  The row index is `counter`, which already travels with a handed-off env-step
// (Sched::counter): no new queue state.
template <int N, bool V2, int RULES = 0, bool TRACE = false>
__global__ __launch_bounds__(64, SNK_LB) void env_step_sched_kernel(StepArgs args_by_value) {
    (void)args_by_value;            // read through step_args() only
    extern __shared__ float4 smem_raw[];
    using LT = LdsFor<N, V2, RULES>;
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    int lane = threadIdx.x;
#ifdef SNK_SCHED_DEBUG
    long long t_wait = 0, n_slices = 0, n_sub = 0, n_chk = 0, n_req = 0, s_top = 0, s_rem = 0;
    const long long t_birth = wall_clock64();
#endif
    for (;;) {
#ifdef SNK_SCHED_DEBUG
        const long long t_p0 = wall_clock64();
#endif
        const StepArgPtr ap = step_args();
        const DevModel& M = g_models[ap->model_slot];
        const int n_envs = ap->n_envs;
        int env;
        {
            const Sched sc = load_sched(ap);
            if (__builtin_amdgcn_readfirstlane((int)__popcll(__ballot(1))) != 64) {   // the 64 lanes stay together (see sched_pop)
                sched_alarm(sc, lane);
                break;
            }
            env = __builtin_amdgcn_readfirstlane(sched_pop(sc, lane, n_envs));
#ifdef SNK_SCHED_DEBUG
            if (env >= 0) { t_wait += wall_clock64() - t_p0; n_slices++; }
            else if (lane == 0) {
                long long* w = sc.wstat + 8 * (size_t)blockIdx.x;
                w[0] = t_wait; w[1] = t_p0 - t_birth; w[2] = n_slices; w[3] = n_sub;
                w[4] = n_chk; w[5] = n_req; w[6] = s_top; w[7] = s_rem;
            }
#endif
        }
        if (env < 0) break;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (M.poison) { L.poison(lane); lds_sync(); }
        // what load_env loads, split around the counter check and the targets: loaded in one go they change this kernel's
        // spill code
        load_rec(L, ap->recs + (size_t)env * LT::REC, lane);
        int counter = __builtin_amdgcn_readfirstlane(ap->sc.counter[env]);
        if (counter < 0 || counter > M.max_counter + 1 || env >= n_envs) {     // never, unless a hand-off went wrong
            sched_alarm(load_sched(ap), lane);
            break;
        }
        set_targets(L, M, ap->actions, env, lane);
        const float mup = ap->mu_plane[env];
        const float mu = fminf(M.mu_link * mup, 10.0f);
        load_mf(L, cache_of<N>(ap->mf_all, env), lane);
        load_box(L, box_of(ap->box_all, env), lane);
        set_box_plane_mu(L, ap->box_all, mup, lane);
        fk_vel(L, M, lane);
        // Snake.step servo loop (snake.py:283-304), `quantum` substeps at a time
        bool end_height = false, complete = false;
        int it_dummy = 0, nc_dummy = 0, in_slice = 0;
        SensorHint hint;
        hint.always = TRACE;
        hint.h_prev = mean_height(L, M, lane);
        while (true) {
            float e = (lane < N) ? (L.targets[lane] - L.q()[lane]) : 0.f;
            float nrm = sqrtf(wave_sum<64>(e * e));
            if (uni(!(nrm > M.servo_tol))) { complete = true; break; }
            const StepArgPtr aq = step_args();
            if (in_slice >= aq->sc.quantum) {
                // slice boundary: carry on unless an env with more work left is waiting
                const Sched sc = load_sched(aq);
                const int remaining = predict_remaining(M, __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(nrm))), counter);
                const int top = sched_top(sc, lane);
#ifdef SNK_SCHED_DEBUG
                n_chk++; s_top += top; s_rem += remaining; if (top > remaining) n_req++;
#endif
                if (top >= remaining + sc.hyst) {
                    // the contact cache and the box travel with the record
                    store_env<LT, true>(L, aq->recs, aq->mf_all, aq->box_all, env, lane);
                    __hip_atomic_store(&sc.counter[env], counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    sched_push(sc, lane, env, remaining);
                    break;
                }
                in_slice = 0;
            }
            hint.counter_next = counter + 1;
            substep(L, M, lane, mu, it_dummy, nc_dummy, hint, rows_of<N>(aq->rows_all), cache_of<N>(aq->mf_all, env), aq->ovf);
            lane = lane_id();       // (not kept in a register across the solve)
#ifdef SNK_SCHED_DEBUG
            n_sub++;
#endif
            counter++;
            in_slice++;
            if constexpr (TRACE) write_trace_row(L, M, step_args(), env, counter - 1, lane);
            hint.h_prev = mean_height(L, M, lane);
            if (uni(hint.h_prev > M.height_thr)) { end_height = true; complete = true; break; }
            if (counter > M.max_counter) { complete = true; break; }
        }
        if (!complete) continue;
        const StepArgPtr af = step_args();
        finish_env_step(L, M, af, env, lane, counter, end_height);
        store_env<LT, false>(L, af->recs, af->mf_all, af->box_all, env, lane);
        atomicAdd(af->sc.finished, lane == 0 ? 1 : 0);
    }
}

// self test of wave_sum / lane_bcast: out[0] = sum32, out[1] = sum64, out[2] = bcast
__global__ __launch_bounds__(64) void selftest_kernel(float* out) {
    const int lane = threadIdx.x;
    float x = (float)(lane + 1);
    float s32 = wave_sum<32>(lane < 22 ? x : 0.f);
    float s64 = wave_sum<64>(x);
    float s64b = wave_sum<64>(lane < 38 ? x * 0.5f : 0.f);
    float b = lane_bcast(x, 17);
    if (lane == 5) { out[0] = s32; out[1] = s64; out[2] = b; out[3] = s64b; }
    // v2 primitives: per-half sums at lanes 31 / 63, and the half swap
    float hr = half_reduce(x);
    if (lane == 31) out[4] = hr;
    if (lane == 63) out[5] = hr;
    swap2 sw = half_swap(x, x * 100.f);
    out[8 + lane] = sw.a;        // expect [x.lo, (100x).lo]
    out[8 + 64 + lane] = sw.b;   // expect [x.hi, (100x).hi]
}

}  // namespace snk
