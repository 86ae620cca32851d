// snk_sched.hpp -- which wave runs which env-step: the launch plan of the unscheduled step kernel, and the in-launch
// queue of the scheduled one (its state, pop / push, the predicted substeps left, the kernel that fills it).
#pragma once
#include <hip/hip_runtime.h>

#include "snk_model.hpp"
#include "snk_wave.hpp"

namespace snk {

// ----------------------------------------------------------------------------------
// Launch planning.  An env-step costs 0..41 substeps depending on how far the joints are
// from their targets (snake.py:228-235), and a substep is a latency-bound ~0.5 ms chain, so
// the launch time is set by envs with many substeps that start late.  This one-block kernel
// sorts the envs by their initial servo error, largest first (counting sort on a 256-bin
// key); env_step_kernel's workgroup b then runs order[b].  Pure scheduling: results do not
// depend on the order.
// ----------------------------------------------------------------------------------
// squared servo error of env e before its env-step: the targets the env-step will set from the caller's actions (clipped,
// mapped to joints by the gait: set_targets) against the joint angles of the env's record
template <int N>
__device__ __forceinline__ float servo_err2(const DevModel& M, int A, const float* __restrict__ recs,
                                            const float* __restrict__ actions, int e) {
    constexpr int REC = (N <= 16) ? 64 : 128;
    const float* q = recs + (size_t)e * REC + 13;
    float err2 = 0.f;
    for (int j = 0; j < N; j++) {
        int k = (M.gait == 0) ? ((j & 1) ? -1 : j / 2) : ((M.gait == 1) ? ((j & 1) ? j / 2 : -1) : j);
        float t = 0.f;
        if (k >= 0 && k < A) t = fminf(fmaxf(actions[(size_t)e * A + k], -1.f), 1.f) * M.scaling;
        float d = t - q[j];
        err2 += d * d;
    }
    return err2;
}

template <int N>
__global__ __launch_bounds__(1024) void plan_kernel(const DevModel* __restrict__ Mp, const float* __restrict__ recs,
                                                    const float* __restrict__ actions, int32_t* __restrict__ order,
                                                    int n_envs) {
    constexpr int NBIN = 256;
    __shared__ int hist[NBIN];
    __shared__ int base[NBIN];
    const DevModel& M = *Mp;
    const int tid = threadIdx.x;
    for (int i = tid; i < NBIN; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    const int A = M.act_dim;
    auto key_of = [&](int e) {
        const float err2 = servo_err2<N>(M, A, recs, actions, e);
        // larger error -> smaller bin index -> earlier workgroup.  log scale, 256 bins.
        float l = __log2f(fmaxf(err2, 1e-12f));          // about [-40, 8]
        int b = (int)((8.0f - l) * 5.0f);
        return b < 0 ? 0 : (b > NBIN - 1 ? NBIN - 1 : b);
    };
    for (int e = tid; e < n_envs; e += blockDim.x) atomicAdd(&hist[key_of(e)], 1);
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < NBIN; i++) { base[i] = run; run += hist[i]; }
    }
    __syncthreads();
    for (int e = tid; e < n_envs; e += blockDim.x) {
        int pos = atomicAdd(&base[key_of(e)], 1);
        order[pos] = e;
    }
}

// ----------------------------------------------------------------------------------
// In-launch scheduling of env-steps (env_step_sched_kernel).
//
// An env-step is 0..41 sequential substeps (snake.py:283-304); a launch of E env-steps on G
// resident waves ends when the slowest wave does.  With whole env-steps as the unit, that is
// (longest + shortest) substeps when E = 2 G -- 45 for the bench workload whose mean load is 35.5
// per wave (tools/balance_dump.py) -- because the jobs are too coarse to level.  An env-step can be
// cut at any substep boundary, though: its whole state is the env's record (plus the substep
// counter).  So G persistent waves pull env-steps from a queue, run them for `quantum` substeps
// and put them back at the end of the queue -- unless no waiting env has more work left than
// this one, in which case the wave just carries on ("longest remaining time first", which
// levels the finish times to within about a quantum).  The remaining work is known almost
// exactly: the position motors shrink the servo error by (1 - kp) per substep [U], so
// remaining = log(err / tol) / -log(1 - kp), capped by the substep counter's limit.
//
// Queue: one ring of {ticket, remaining, env} entries.  A pop is ONE returning atomic add on
// `head` (a ticket), then a wait for that ticket's entry; a push is one atomic add on `tail` and
// one 8-byte agent-scope store (the slot is a tagged granule, read back with a returning atomic: sched_pop).  (A compare-and-swap pop costs O(G^2) attempts when G waves reach
// a slice boundary together: 14 ms per launch, measured.)  Tickets are never reset; unsigned
// wrap-around is harmless because the ring size is a power of two (tests preset head/tail just below 2^32).  Pops in excess of pushes wait for an entry that may never come; they
// leave when `finished` says every env-step is complete, and the next launch starts its tickets at
// `head`.  waiting[r] counts queued env-steps with r substeps left (the carry-on test).
// The record hand-off between waves follows MI355X_MICROARCH.md "inter-workgroup visibility":
// every handed-off byte stored write-through (sc1), s_waitcnt vmcnt(0), then the queue entry;
// consumer: entry seen, agent acquire, wait, plain loads.  Results do not depend on the schedule: a slice boundary
// stores and reloads exactly the floats a continuing wave keeps (the property test-mode telemetry
// relies on, tests/test_gpu_env.py).
//
// Every wait is bounded in wall-clock time (kWaitTicks): a wave that gives up raises the
// host-visible word `alarm` and leaves; the others follow, so the grid always drains.
// ----------------------------------------------------------------------------------
constexpr int kBuckets = 64;
constexpr long long kWaitTicks = 200000000;    // wall_clock64() runs at 100 MHz: 2 s (an env-step is < 50 ms)

// The model of the scheduled kernel lives in constant memory: its queue atomics and fences make the
// compiler treat every load through a global pointer as clobbered (vector loads where the plain
// kernel has scalar ones); loads from __constant__ stay scalar.  One slot per live handle
// (snk_api.hip hands them out).
constexpr int kModelSlots = 32;
__constant__ DevModel g_models[kModelSlots];

struct Sched {
    uint32_t* head;             // tickets claimed
    uint32_t* tail;             // tickets issued
    unsigned long long* ent;    // [cap]: (ticket << 32) | (remaining << 24) | env; all-ones when never written
    int32_t* waiting;           // [kBuckets] queued env-steps by substeps left
    int32_t* counter;           // [n_envs] substeps done so far in this env-step
    int32_t* finished;          // env-steps completed in this launch
    int32_t* alarm;             // host-mapped: set when a bounded wait ran out
    uint32_t cap;               // ring size: a power of two >= 2 n_envs (an env is queued at most once), so that the
                                // slot of a ticket, tk & (cap - 1), stays consistent when the 32-bit tickets wrap
    int32_t quantum;            // substeps per slice
    int32_t hyst;               // a slice's env-step is handed off when a waiting one has at least this many more substeps
                                // left.  1 = strict longest-remaining-first: two env-steps of equal length then swap places
                                // after every substep (each hand-off moves the record and the contact cache through
                                // memory); 3 levels the finish times as well and hands off a third as often: measured
                                // 336.6 k -> 342.7 k env-steps/s (1, 3, 4, 6, 8: 336.6 / 342.7 / 341.6 / 341.4 / 322.9)
    long long* wstat;           // SNK_SCHED_DEBUG: [grid][4] ticks waiting, ticks alive, slices, substeps
};

__device__ __forceinline__ int predict_remaining(const DevModel& M, float err, int counter) {
    if (!(err > M.servo_tol)) return 0;
    const float decay = fmaxf(-__log2f(fminf(fmaxf(1.0f - M.kp, 1e-6f), 0.999f)), 1e-3f);
    const float r = ceilf(__log2f(err / M.servo_tol) / decay);
    const int cap = M.max_counter + 1 - counter;
    int R = (int)fminf(r, (float)cap);
    R = R < 1 ? 1 : R;
    return R > kBuckets - 1 ? kBuckets - 1 : R;
}

// most substeps left among the queued env-steps (-1: queue empty)
__device__ __forceinline__ int sched_top(const Sched& sc, int lane) {
    const int w = __hip_atomic_load(&sc.waiting[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long m = __ballot(w > 0);
    return m ? 63 - __clzll(m) : -1;
}

__device__ __forceinline__ void sched_alarm(const Sched& sc, int lane) {
    (void)lane;
    __hip_atomic_store(sc.alarm, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // every lane, same word
}

// next env for this wave, or -1 when every env-step of the launch is complete (or on alarm).
// Two waits.  (1) `tail` -- a word only agent-scope atomic adds touch -- is polled with a 4-byte sc1 load until
// ticket tk has been issued (MI355X_MICROARCH.md, hand-off table, row 3: "agent-scope atomic adds ... a
// global_load_dword sc1 poll of that counter").  (2) A producer takes its ticket BEFORE it stores the entry
// (sched_push), so the slot may still hold the entry of ticket tk - cap: the slot is a tagged 8-byte granule
// {ticket, remaining|env} and is re-read until the tag matches.  That re-read is a RETURNING ATOMIC (an add of a
// zero the compiler cannot see through): it executes where agent-scope atomics execute, beyond the per-XCD L2s,
// so no cached copy of the slot -- in this CU's L1 or in this XCD's L2 -- can answer it.  (Round 1 read the slot
// with `__hip_atomic_load`, i.e. `global_load_dwordx2 sc1`, which is served by the XCD's own L2; the guide lists
// that as observed-fresh for granules, not as guaranteed, and its row 3 excludes dwordx2 loads outright.  The one
// hang on record, gpurun_out/d3000.log, predates the first committed scheduler and had the lane-threaded back edge
// described below as its cause; the atomic read removes the remaining reliance on an observed behaviour.)
__device__ __forceinline__ int sched_pop(const Sched& sc, int lane, int n_envs) {
    // NO `if (lane == 0)` around the queue operations of this file: with a lane-dependent branch at the top of the
    // scheduling loop the compiler threads the loop's back edge per lane, lane 0 and lanes 1..63 then run the loop
    // body in separate passes, and every cross-lane operation of the solver breaks (observed: a wave that
    // re-processes one env for ever).  Every lane issues the atomic with its own operand instead (the atomic
    // optimizer folds the 64 into one memory operation).
    uint32_t tk = atomicAdd(sc.head, lane == 0 ? 1u : 0u);
    tk = (uint32_t)__builtin_amdgcn_readfirstlane((int)tk);
    const long long t_start = wall_clock64();
    int nap = 1;
    for (;;) {
        const uint32_t t = __hip_atomic_load(sc.tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((int32_t)((uint32_t)__builtin_amdgcn_readfirstlane((int)t) - tk) > 0) break;    // ticket tk has been issued
        const int fin = __hip_atomic_load(sc.finished, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__builtin_amdgcn_readfirstlane(fin) >= n_envs) return -1;
        if (uni(wall_clock64() - t_start > kWaitTicks)) {
            // give up once nobody can still be working, or when somebody else already has
            if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(sc.alarm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) ||
                uni(wall_clock64() - t_start > 4 * kWaitTicks)) {
                sched_alarm(sc, lane);
                return -1;
            }
        }
        for (int i = 0; i < nap; i++) __builtin_amdgcn_s_sleep(16);      // ~0.5 us, backing off to ~7 us
        if (nap < 16) nap++;
    }
    unsigned long long* e = sc.ent + (tk & (sc.cap - 1u));
    unsigned long long zero = 0ull;
    asm volatile("" : "+v"(zero));      // opaque: an add of a literal 0 would be folded into a plain atomic load
    for (;;) {
        // every lane adds 0 to the same slot (the atomic optimizer folds the 64 into one memory operation)
        const unsigned long long v = __hip_atomic_fetch_add(e, zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
        if (hi == tk) {
            atomicAdd(&sc.waiting[lo >> 24], lane == 0 ? -1 : 0);
            return (int)(lo & 0xFFFFFFu);
        }
        if (uni(wall_clock64() - t_start > 4 * kWaitTicks)) break;
        __builtin_amdgcn_s_sleep(4);
    }
    sched_alarm(sc, lane);
    return -1;
}

// hand an unfinished env-step (record and counter already stored write-through by this wave) to whoever pops it
__device__ __forceinline__ void sched_push(const Sched& sc, int lane, int env, int remaining) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the write-through stores have left before the entry does
    atomicAdd(&sc.waiting[remaining], lane == 0 ? 1 : 0);
    const uint32_t tk = (uint32_t)__builtin_amdgcn_readfirstlane((int)atomicAdd(sc.tail, lane == 0 ? 1u : 0u));
    __hip_atomic_store(sc.ent + (tk & (sc.cap - 1u)),        // every lane stores the same 8 bytes
                       ((unsigned long long)tk << 32) | ((unsigned long long)remaining << 24) |
                           (unsigned long long)(uint32_t)env,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One block: the queue of a launch, env-steps with the most predicted substeps first (counting sort).
template <int N>
__global__ __launch_bounds__(1024) void plan_sched_kernel(const DevModel* __restrict__ Mp, const float* __restrict__ recs,
                                                          const float* __restrict__ actions, Sched sc, int n_envs) {
    __shared__ uint32_t hist[kBuckets], base[kBuckets];
    const DevModel& M = *Mp;
    const int tid = threadIdx.x;
    if (tid < kBuckets) hist[tid] = 0;
    __syncthreads();
    const int A = M.act_dim;
    auto key_of = [&](int e) { return predict_remaining(M, sqrtf(servo_err2<N>(M, A, recs, actions, e)), 0); };
    constexpr int kKeep = 8;                 // keys of the first 8 envs of a thread stay in registers for the second pass
    int keys[kKeep];
#pragma unroll
    for (int i = 0; i < kKeep; i++) {
        const int e = tid + i * 1024;
        keys[i] = e < n_envs ? key_of(e) : 0;
        if (e < n_envs) atomicAdd(&hist[keys[i]], 1u);
    }
    for (int e = tid + kKeep * 1024; e < n_envs; e += 1024) atomicAdd(&hist[key_of(e)], 1u);
    __syncthreads();
    const uint32_t t0 = *sc.head;       // tickets the previous launch's leaving waves took are skipped
    if (tid == 0) {
        uint32_t run = t0;
        for (int b = kBuckets - 1; b >= 0; b--) { base[b] = run; run += hist[b]; }
        *sc.tail = run;
        *sc.finished = 0;
    }
    if (tid < kBuckets) sc.waiting[tid] = (int32_t)hist[tid];
    __syncthreads();
    auto enqueue = [&](int e, int b) {
        const uint32_t tk = atomicAdd(&base[b], 1u);
        sc.ent[tk & (sc.cap - 1u)] = ((unsigned long long)tk << 32) | ((unsigned long long)b << 24) | (unsigned long long)(uint32_t)e;
        sc.counter[e] = 0;
    };
#pragma unroll
    for (int i = 0; i < kKeep; i++) {
        const int e = tid + i * 1024;
        if (e < n_envs) enqueue(e, keys[i]);
    }
    for (int e = tid + kKeep * 1024; e < n_envs; e += 1024) enqueue(e, key_of(e));
}

}  // namespace snk
