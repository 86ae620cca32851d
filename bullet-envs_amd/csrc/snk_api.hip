// snk_api.hip -- C ABI (include/snk.h) over the HIP kernels of snk_device.hpp.
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC snk_api.hip -o libsnk.so
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <memory>
#include <string>
#include <mutex>
#include <vector>

#include "../../include/snk.h"
#include "snk_device.hpp"
#include "snk_seam.hpp"

namespace {

thread_local std::string g_err;

int fail(const std::string& msg) {
    g_err = msg;
    return 1;
}
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess)                                                                 \
            return fail(std::string(#expr) + ": " + hipGetErrorString(e__));                   \
    } while (0)

}  // namespace

struct snk_handle {
    snk_params P;
    snk::HostModel H;
    snk::DevModel D;
    int n_envs, device, n, rec;
    bool v2 = true;               // register-resident solve (16 links without an obstacle); else streamed rows
    snk::DevModel* d_model = nullptr;
    float* d_recs = nullptr;
    float* d_mu = nullptr;
    void* d_stage = nullptr;      // the staging arena of every host form (snk::stage_arena), made on the first such call
    float* d_mf = nullptr;        // contact_model 1: the persistent contact manifolds, [n_envs][2n][kMfFloats]
    float* d_rows = nullptr;      // 32-link chains: constraint rows streamed from global memory (snk_device.hpp: pgs_v1)
    unsigned long long* d_ovf = nullptr;   // contacts the solves had no room for (snk_contact_overflow): 3 counters
    float* d_box = nullptr;       // obstacle 2: the free box of every env, [n_envs][kBoxFloats] (state 13, count, manifold 24)
    float* d_reset = nullptr;     // the reset-pose table, [n_envs][reset_row_floats(n)] = [pos 3 | quat xyzw 4 | q n | padding]
    int32_t* d_order = nullptr;
    float* d_links = nullptr;     // the link table of the unmerged tree (snk_model.hpp: build_link_table), for snk_link_states
    float* d_render = nullptr;    // snk_render's per-image primitive and camera tables (snk::render_scratch), made on first use
    bool plan = true;
    // in-launch scheduler of env_step_sched_kernel (snk_device.hpp): rings, counters, the host-mapped alarm word
    snk::Sched sched = {};
    int32_t* h_alarm = nullptr;
    int grid_waves = 0;           // resident waves of the step kernel
    // snk_debug_rows: the last launch on this handle was substep_kernel over every env (launch_substep sets it, every other launch of this
    // file and every entry of the other objects, which come through render_view, clears it)
    bool rows_of_substep = false;
    int model_slot = -1;          // index into snk::g_models (constant memory); -1: none free, unscheduled kernel
    bool use_sched = true;
    size_t lds_bytes = 0;
    // timing: pool of event pairs, one pair per snk_step launch, read back in one go
    std::vector<hipEvent_t> ev;
    int ev_used = 0;
    // THE OWNER of the handle's device memory: every d_* pointer above and every pointer of `sched` is one of these slots
    // (ensure, below, is the only place that allocates one; snk_destroy frees the list)
    struct Owned { void** slot; size_t bytes; };
    std::vector<Owned> owned;
};

namespace {

// The kernel variant of a handle: chain length, solve (V2: register-resident) and solver-rules variant (snk_device.hpp:
// LdsFor, rules_variant), as compile-time constants.  Instantiated for 16 links with the register-resident solve, 16 and
// 32 links with the streamed-row solve (32: always; 16: when the world holds an obstacle, whose contacts need it).
template <int N_, bool V2_, int RULES_>
struct Variant {
    static constexpr int N = N_;
    static constexpr bool V2 = V2_;
    static constexpr int RULES = RULES_;
};
template <int N, bool V2, class F>
int with_rules(int rules, F& fn) {
    return rules == 2 ? fn(Variant<N, V2, 2>{}) : (rules == 1 ? fn(Variant<N, V2, 1>{}) : fn(Variant<N, V2, 0>{}));
}
// fn(Variant<...>{}) for h's variant.  (Only the solving kernels take RULES: the reset and obs kernels of the three
// variants of one (N, V2) are one instantiation.)
template <class F>
int dispatch(const snk_handle* h, F&& fn) {
    const int rules = snk::rules_variant(h->D);
    const int rc = snk::for_variant(h->n, h->v2, [&](auto n, auto v2) {
        return with_rules<decltype(n)::value, decltype(v2)::value>(rules, fn);
    });
    return rc == snk::kUnsupported ? fail("unsupported n_modules (16 or 32)") : rc;
}

// floats per row of the trace buffer (snk_trace_row_floats): the payload [obs | link positions] in whole 128-byte lines
int trace_row_floats(int n) { return (3 * n + 8 + 3 * (n + 1) + 31) / 32 * 32; }
// floats per row of the reset-pose table (snk::kResetRow): the payload [pos 3 | quat 4 | q n] in whole 128-byte lines
int reset_row_floats(int n) { return (7 + n + 31) / 32 * 32; }

// ensure: THE place where a handle gets device memory.  Afterwards *slot -- a member of *h or of h->sched: the list keeps
// its address -- holds at least `bytes`: made now if it did not exist, replaced (contents NOT kept) if it was too small,
// and a new buffer has every byte set to `fill` (kNoFill: left as it comes).  The device is idle before an old buffer
// goes: nothing enqueued still reads it.
constexpr int kNoFill = -1;
template <class T>
int ensure(snk_handle* h, T** slot, size_t bytes, int fill = kNoFill) {
    snk_handle::Owned* o = nullptr;
    for (snk_handle::Owned& x : h->owned)
        if (x.slot == reinterpret_cast<void**>(slot)) o = &x;
    if (o && o->bytes >= bytes) return 0;
    if (!o) { h->owned.push_back({reinterpret_cast<void**>(slot), 0}); o = &h->owned.back(); }
    if (*slot) { HIP_TRY(hipDeviceSynchronize()); (void)hipFree(*slot); *slot = nullptr; o->bytes = 0; }
    HIP_TRY(hipMalloc(slot, bytes));
    o->bytes = bytes;
    if (fill != kNoFill) HIP_TRY(hipMemset(*slot, fill, bytes));
    return 0;
}

// packed_stride > 0 (snk_step_packed): obs rows of that stride, reward and done flag behind each row's observation.
// TRACE (snk_step_traced): the kernels that also write `trace`, trace_rows rows per env.
template <bool TRACE, class K>
int launch_step(K, snk_handle* h, float* act, float* obs, float* rew, uint8_t* done, int32_t* sub, int vec_mode,
                hipStream_t st, int packed_stride, float* trace, int trace_rows) {
    snk::StepArgs a;
    a.recs = h->d_recs; a.mu_plane = h->d_mu; a.actions = act; a.obs = obs; a.rew = rew; a.done = done; a.substeps = sub;
    a.rows_all = h->d_rows; a.mf_all = h->d_mf; a.ovf = h->d_ovf; a.box_all = h->d_box; a.sc = h->sched;
    a.model_slot = h->model_slot; a.vec_mode = vec_mode; a.n_envs = h->n_envs;
    a.obs_stride = packed_stride > 0 ? packed_stride : h->D.obs_dim; a.packed = packed_stride > 0 ? 1 : 0; a.pad_ = 0;
    a.model = h->d_model; a.order = h->plan ? h->d_order : nullptr;
    a.trace = trace; a.trace_rows = trace_rows; a.trace_stride = trace_row_floats(h->n);
    a.reset_all = h->d_reset;
    h->rows_of_substep = false;
    if (h->use_sched) {
        hipLaunchKernelGGL((snk::plan_sched_kernel<K::N>), dim3(1), dim3(1024), 0, st, h->d_model, h->d_recs, act, h->sched,
                           h->n_envs);
        hipLaunchKernelGGL((snk::env_step_sched_kernel<K::N, K::V2, K::RULES, TRACE>), dim3(h->grid_waves), dim3(64),
                           h->lds_bytes, st, a);
        return 0;
    }
    if (h->plan)
        hipLaunchKernelGGL((snk::plan_kernel<K::N>), dim3(1), dim3(1024), 0, st, h->d_model, h->d_recs, act, h->d_order,
                           h->n_envs);
    hipLaunchKernelGGL((snk::env_step_kernel<K::N, K::V2, K::RULES, TRACE>), dim3(h->grid_waves), dim3(64), h->lds_bytes, st, a);
    return 0;
}
template <class K>
int launch_substep(K, snk_handle* h, const float* tgt, int k, int32_t* info, const uint8_t* active, hipStream_t st) {
    hipLaunchKernelGGL((snk::substep_kernel<K::N, K::V2, K::RULES>), dim3(h->grid_waves), dim3(64), h->lds_bytes, st,
                       h->d_model, h->d_recs, h->d_mu, tgt, k, info, h->n_envs, h->d_rows, h->d_mf, h->d_ovf, h->d_box, active);
    h->rows_of_substep = active == nullptr;      // (a masked launch leaves the blocks of the envs it skips as they were)
    return 0;
}
template <class K>
int launch_reset(K, snk_handle* h, const uint8_t* mask, float* obs, int hard, hipStream_t st) {
    hipLaunchKernelGGL((snk::reset_kernel<K::N, K::V2>), dim3(h->n_envs), dim3(64), h->lds_bytes, st, h->d_recs, mask, obs,
                       h->d_reset, hard, h->n_envs);
    h->rows_of_substep = false;
    return 0;
}
// Waves of the step kernel a CU holds: __launch_bounds__(64, 2) = 2 per SIMD, 4 SIMDs, and the CU's LDS (160 KB on
// gfx950; hipOccupancyMaxActiveBlocksPerMultiprocessor assumes 64 KB and under-counts).  Too many is harmless (late
// blocks find the queue drained), too few idles the chip.
int resident_waves(size_t bytes, int device, int* out) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    size_t lds = prop.maxSharedMemoryPerMultiProcessor;
    if (lds < 160 * 1024) lds = 160 * 1024;
    int per_cu = (int)(lds / (bytes ? bytes : 1));
    if (per_cu > 4 * SNK_LB) per_cu = 4 * SNK_LB;        // (the step kernels' launch bounds: SNK_LB waves per SIMD)
    if (const char* w = getenv("SNK_WAVES_PER_CU")) {       // occupancy experiments only (fewer resident waves than fit)
        const int v = atoi(w);
        if (v >= 1 && v < per_cu) per_cu = v;
    }
    if (per_cu < 1) per_cu = 1;
    *out = per_cu * prop.multiProcessorCount;
    return 0;
}
// (every solver-rules variant has the same LDS image: the rules are compile-time constants only)
template <class K>
int set_lds_attr(K, size_t bytes) {
    const void* kernels[] = {reinterpret_cast<const void*>(&snk::env_step_kernel<K::N, K::V2, K::RULES>),
                             reinterpret_cast<const void*>(&snk::env_step_sched_kernel<K::N, K::V2, K::RULES>),
                             reinterpret_cast<const void*>(&snk::env_step_kernel<K::N, K::V2, K::RULES, true>),
                             reinterpret_cast<const void*>(&snk::env_step_sched_kernel<K::N, K::V2, K::RULES, true>),
                             reinterpret_cast<const void*>(&snk::substep_kernel<K::N, K::V2, K::RULES>),
                             reinterpret_cast<const void*>(&snk::reset_kernel<K::N, K::V2>),
                             reinterpret_cast<const void*>(&snk::obs_kernel<K::N, K::V2>)};
    for (const void* f : kernels) HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

// slots of snk::g_models, shared by the handles of this process
std::mutex g_slot_mutex;
bool g_slot_used[snk::kModelSlots] = {};
int take_model_slot() {
    std::lock_guard<std::mutex> lk(g_slot_mutex);
    for (int i = 0; i < snk::kModelSlots; i++)
        if (!g_slot_used[i]) { g_slot_used[i] = true; return i; }
    return -1;
}
void release_model_slot(int i) {
    if (i < 0) return;
    std::lock_guard<std::mutex> lk(g_slot_mutex);
    g_slot_used[i] = false;
}

// the step kernel's bounded waits (snk_device.hpp: sched_pop) raise this word when one runs out.  From then on the
// handle is poisoned: an env-step was abandoned half-way, so records, contact caches and queue no longer describe a
// simulator state.  Every call that launches on, reads or writes that state refuses; snk_destroy, snk_last_error, the
// dimension getters, the counters (snk_contact_overflow / _histogram) and the timing calls still work.
int check_alarm(const snk_handle* h) {
    if (h->h_alarm && *(volatile int32_t*)h->h_alarm)
        return fail("env-step scheduler: a bounded wait ran out (state of this handle is no longer valid; snk_destroy it)");
    return 0;
}

// THE ENTRY CONTRACT.  Every entry point calls enter(h, what) once, behind its own null-argument refusals (and where
// a call today names another refusal first -- "null buffer", "no contact cache", "no free box" -- behind that too):
//   D  kDev    hipSetDevice(h->device)
//   I  kIdle   hipDeviceSynchronize(): a step enqueued on a non-blocking stream may still be running
//   A  kAlive  refuses a poisoned handle (check_alarm), after D and I
// The code's copy of the paragraph at snk_debug_raise_alarm in include/snk.h:
//   D I A  snk_get_state  snk_set_state  snk_get_manifold  snk_set_manifold  snk_get_box  snk_set_box  snk_get_obs
//          snk_mean_height  snk_link_positions  snk_joint3_reaction_fz  snk_set_ground_friction  snk_get_reset_pose
//          snk_set_reset_pose  snk_debug_set_tickets  snk_render_host  snk_link_states_host  snk_copy_envs_host
//          snk_debug_rows  snk_contacts_host  snk_closest_points_host  snk_ray_test_host
//   D . A  snk_reset  snk_step  snk_step_packed  snk_step_traced  snk_reset_host  snk_step_host  snk_step_traced_host
//          snk_substep_host  snk_set_reset_pose_dev  snk_render  snk_substep  snk_observe  snk_link_states  snk_copy_envs
//          snk_contacts  snk_closest_points  snk_ray_test  snk_contact_slots (returns 0)
//   . . A  snk_reset_pose_floats (returns 0)
//   D I .  snk_get_ground_friction  snk_contact_overflow  snk_contact_histogram  snk_contact_histogram_enable
//          snk_destroy (the two calls bare: errors ignored, snk_last_error untouched)
//   D . .  snk_timing_enable  snk_timing_read
//   . I .  snk_sched_stats (SNK_SCHED_DEBUG builds)
//   . . .  snk_num_envs  snk_obs_dim  snk_act_dim  snk_state_dim  snk_record_floats  snk_trace_row_floats
//          snk_manifold_floats  snk_model_describe  snk_debug_raise_alarm  snk_link_state_rows; and the calls without a
//          handle
enum : unsigned { kDev = 1, kIdle = 2, kAlive = 4, kState = kDev | kIdle | kAlive };
int enter(const snk_handle* h, unsigned what) {
    if (what & kDev) HIP_TRY(hipSetDevice(h->device));
    if (what & kIdle) HIP_TRY(hipDeviceSynchronize());
    return (what & kAlive) ? check_alarm(h) : 0;
}

// the launch of snk_step / snk_step_packed / snk_step_traced (trace != null), between a pair of snk_timing_enable's
// events while the pool has one left
int timed_step(snk_handle* h, float* act, float* obs, float* rew, uint8_t* done, int32_t* sub, int vec_mode, hipStream_t st,
               int packed_stride, float* trace = nullptr, int trace_rows = 0) {
    const bool timed = 2 * h->ev_used + 1 < (int)h->ev.size();
    if (timed) HIP_TRY(hipEventRecord(h->ev[2 * h->ev_used], st));
    const int rc = dispatch(h, [&](auto k) {
        return trace ? launch_step<true>(k, h, act, obs, rew, done, sub, vec_mode, st, packed_stride, trace, trace_rows)
                     : launch_step<false>(k, h, act, obs, rew, done, sub, vec_mode, st, packed_stride, nullptr, 0);
    });
    if (rc) return rc;
    if (timed) {
        HIP_TRY(hipEventRecord(h->ev[2 * h->ev_used + 1], st));
        h->ev_used++;
    }
    return snk::launch_ok(nullptr);
}

// one obs_kernel pass over h's records, enqueued on st (snk_observe)
int launch_obs(snk_handle* h, float* obs, float* height, float* linkpos, hipStream_t st) {
    h->rows_of_substep = false;
    const int rc = dispatch(h, [&](auto k) {
        hipLaunchKernelGGL((snk::obs_kernel<decltype(k)::N, decltype(k)::V2>), dim3(h->n_envs), dim3(64), h->lds_bytes,
                           st, h->d_model, h->d_recs, obs, height, linkpos, h->n_envs);
        return 0;
    });
    return (rc || snk::launch_ok(nullptr)) ? 1 : 0;
}

// A contact manifold on the host (the oracle's layout): [count, 4 x (point on the link in link coordinates 3, point on
// the ground 3, applied normal impulse)] = 29 floats.  On the device: a count, and 4 x (a3, b.x, b.y, lambda) at `pts`
// (the ground point's z is the plane's, 0).  Slots past the count hold stale points: reported as zeros.
void manifold_to_host(float count, const float* pts, float* o) {
    const int n = count < 0.f ? 0 : (count > 4.f ? 4 : (int)count);
    o[0] = (float)n;
    for (int j = 0; j < 4; j++) {
        const bool on = j < n;
        for (int r = 0; r < 3; r++) o[1 + 7 * j + r] = on ? pts[6 * j + r] : 0.f;
        o[4 + 7 * j] = on ? pts[3 + 6 * j] : 0.f;
        o[5 + 7 * j] = on ? pts[4 + 6 * j] : 0.f;
        o[6 + 7 * j] = 0.f;
        o[7 + 7 * j] = on ? pts[5 + 6 * j] : 0.f;
    }
}
// the reverse: fills pts, returns the count (a manifold holds 0 .. 4 points, whatever the caller says)
float manifold_from_host(const float* o, float* pts) {
    for (int j = 0; j < 4; j++) {
        for (int r = 0; r < 3; r++) pts[6 * j + r] = o[1 + 7 * j + r];
        pts[3 + 6 * j] = o[4 + 7 * j];
        pts[4 + 6 * j] = o[5 + 7 * j];
        pts[5 + 6 * j] = o[7 + 7 * j];
    }
    return o[0] >= 0.f ? (o[0] <= 4.f ? floorf(o[0]) : 4.f) : 0.f;
}

// A per-environment device table: `rows` rows of `stride` floats (the padding included).  The handle's tables:
struct RowTable { float* d; size_t stride, rows; };
// the state records: [base 13 | q n | qd n || motor torques n | joint-0 fz | previous x || joint-3 fz | padding]
//                     `-- state_dim = 13 + 2n --'`------------- aux: n + 2 ------------'
RowTable records(const snk_handle* h) { return {h->d_recs, (size_t)h->rec, (size_t)h->n_envs}; }
size_t rec_joint3_fz(const snk_handle* h) { return (size_t)(15 + 3 * h->n); }
RowTable friction(const snk_handle* h) { return {h->d_mu, 1, (size_t)h->n_envs}; }
RowTable reset_poses(const snk_handle* h) { return {h->d_reset, (size_t)reset_row_floats(h->n), (size_t)h->n_envs}; }
// one row per CYLINDER: [count, 3 pad, 4 x (a3, b.x, b.y, lambda)]
RowTable link_manifolds(const snk_handle* h) { return {h->d_mf, (size_t)snk::kMfFloats, (size_t)h->n_envs * 2 * h->n}; }
// the free box: [state 13 | count, 4 x (a3, b.x, b.y, lambda) | padding]
RowTable boxes(const snk_handle* h) { return {h->d_box, (size_t)snk::kBoxFloats, (size_t)h->n_envs}; }
constexpr size_t kBoxState = 13, kBoxMf = 25;

// Column range [first, first + width) of a table and its dense host array [rows][width] (null: skipped; rows_get WRITES it)
struct Cols { size_t first, width; const float* host; };
// rows [r0, r1) of one range straight between the table and its host array (`set`: to the device)
int direct(const RowTable& t, const Cols& c, size_t r0, size_t r1, bool set) {
    const size_t f = sizeof(float), dp = t.stride * f, hp = c.width * f;
    float *dev = t.d + r0 * t.stride + c.first, *hst = const_cast<float*>(c.host) + r0 * c.width;
    const hipMemcpyKind kind = set ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    if (c.width == t.stride) HIP_TRY(hipMemcpy(set ? dev : hst, set ? hst : dev, (r1 - r0) * hp, kind));
    else HIP_TRY(hipMemcpy2D(set ? dev : hst, set ? dp : hp, set ? hst : dev, set ? hp : dp, hp, r1 - r0, kind));
    return 0;
}
// rows_get / rows_set: THE transfer between a table and dense host arrays (the device idle: enter(kIdle)), `mask` [rows]
// (null: all) naming the rows rows_set writes.  Measured (profiles/r13_host_api_before_after.txt): a table of up to
// kDirectBytes goes range by range, strided, unstaged (16 envs, every table <= 57 KB: this wins); a larger one crosses
// whole, once, the ranges gathered / scattered on the host (4096 envs, >= 512 KB: wins by 25 %).  Whole rows go straight.
constexpr size_t kDirectBytes = 64 << 10;
int rows_move(const RowTable& t, std::initializer_list<Cols> cols, const uint8_t* mask, bool set) {
    const size_t bytes = t.rows * t.stride * sizeof(float);
    const bool staged = bytes > kDirectBytes && !(cols.size() == 1 && cols.begin()->width == t.stride && !mask);
    std::vector<float> all(staged ? t.rows * t.stride : 0);
    if (staged) HIP_TRY(hipMemcpy(all.data(), t.d, bytes, hipMemcpyDeviceToHost));
    for (const Cols& c : cols)
        for (size_t r0 = 0, r1; c.host && r0 < t.rows; r0 = r1 + 1) {      // every run [r0, r1) of rows the mask names
            for (r1 = r0; r1 < t.rows && (!mask || mask[r1]); r1++) {}
            if (!staged && r1 > r0 && direct(t, c, r0, r1, set)) return 1;
            for (size_t r = r0; staged && r < r1; r++) {
                float *a = &all[r * t.stride + c.first], *x = const_cast<float*>(c.host) + r * c.width;
                memcpy(set ? a : x, set ? x : a, c.width * sizeof(float));
            }
        }
    if (staged && set) HIP_TRY(hipMemcpy(t.d, all.data(), bytes, hipMemcpyHostToDevice));
    return 0;
}
int rows_get(const RowTable& t, std::initializer_list<Cols> cols) { return rows_move(t, cols, nullptr, false); }
int rows_set(const RowTable& t, std::initializer_list<Cols> cols, const uint8_t* mask = nullptr) { return rows_move(t, cols, mask, true); }

// h->D to the device: the handle's copy in global memory and, on a scheduled handle, its slot of snk::g_models
int upload_model(snk_handle* h) {
    HIP_TRY(hipMemcpy(h->d_model, &h->D, sizeof(snk::DevModel), hipMemcpyHostToDevice));
    if (h->model_slot >= 0)
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(snk::g_models), &h->D, sizeof(snk::DevModel),
                                  (size_t)h->model_slot * sizeof(snk::DevModel), hipMemcpyHostToDevice));
    return 0;
}

// the host and device models of bare params (the models are large: on the heap)
struct Models { snk::HostModel H; snk::DevModel D; };
std::unique_ptr<Models> models_of(const snk_params& p) {
    std::unique_ptr<Models> m(new Models);
    snk::build_host_model(p, m->H);
    snk::build_dev_model(p, m->H, m->D);
    return m;
}

}  // namespace

// the seam of the other objects (snk_seam.hpp): their translation units see this much of a handle, and report
// through g_err
namespace snk {
int api_fail(const char* msg) { return fail(msg); }
int render_view(snk_handle* h, bool sync, RenderView* v) {
    if (enter(h, sync ? kState : (kDev | kAlive))) return 1;
    h->rows_of_substep = false;
    v->device = h->device; v->n = h->n; v->n_envs = h->n_envs; v->v2 = h->v2;
    v->D = &h->D; v->d_model = h->d_model; v->d_recs = h->d_recs; v->d_box = h->d_box;
    return 0;
}
int world_view(snk_handle* h, bool sync, WorldView* v) {
    if (render_view(h, sync, v)) return 1;
    v->d_links = h->d_links;
    const size_t ne = (size_t)h->n_envs;
    const RowTable t[WorldView::kTables] = {records(h), link_manifolds(h), boxes(h), friction(h), reset_poses(h)};
    for (int i = 0; i < WorldView::kTables; i++) v->tables[i] = {t[i].d, t[i].stride * (t[i].rows / ne)};
    return 0;
}
float* render_scratch(snk_handle* h, size_t need) { return ensure(h, &h->d_render, need) ? nullptr : h->d_render; }
// (SNK_POISON: a new or replaced arena starts as NaNs, like every fresh allocation of init_handle)
void* stage_arena(snk_handle* h, size_t need) {
    return ensure(h, &h->d_stage, need, h->D.poison ? 0xFF : kNoFill) ? nullptr : h->d_stage;
}
}  // namespace snk

extern "C" {

const char* snk_last_error(void) { return g_err.c_str(); }

void snk_default_params(snk_params* p) {
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(snk_params);
    p->abi_version = SNK_ABI_VERSION;
    p->n_modules = 16;
    p->inertia_from_file = 0;
    p->default_mass = 1.0;
    p->collision_margin = 0.001;
    p->hull_sides = 32;         // PyBullet's import of a URDF <cylinder> [U]; snake.py:93 passes no URDF_USE_IMPLICIT_CYLINDER
    p->contact_model = 1;       // Bullet's persistent manifold [U] (0 + hull_sides 0: the round-1 model)
    p->self_collision = 1;      // the reference loads the snake with URDF_USE_SELF_COLLISION (snake.py:93)
    p->obstacle = 0;            // snake.py:94 has add_obstacle commented out; snake_gait_test.py:51 loads it
    p->obstacle_pos[0] = 2.0; p->obstacle_pos[1] = 0.0; p->obstacle_pos[2] = 0.1;
    p->obstacle_half[0] = 0.1; p->obstacle_half[1] = 0.4; p->obstacle_half[2] = 0.1;      // snake/block.urdf:16
    p->mu_obstacle = 0.5;       // [U]
    p->obstacle_mass = 200.0;   // snake/block.urdf:6
    p->dt = 1.0 / 240.0;
    p->gravity_z = -9.8;
    p->lin_damping = 0.04;
    p->ang_damping = 0.04;
    p->joint_damping = 0.1;
    p->max_coord_vel = 100.0;
    p->kp = 0.1;
    p->kd = 1.0;
    p->max_motor_impulse = std::numeric_limits<double>::infinity();
    p->joint_lo = -1.57;
    p->joint_hi = 1.57;
    p->limit_erp = 0.2;
    p->limit_max_impulse = 100.0;
    p->mu_link = 2.0;
    p->aniso[0] = 1.0; p->aniso[1] = 0.1; p->aniso[2] = 0.01;
    p->contact_erp = 0.08;
    p->linear_slop = 1e-5;
    p->breaking_threshold = 0.02;
    p->relative_breaking_threshold = 1;     // btCollisionDispatcher's default flags [U]
    p->cone_friction = 1;
    p->n_iterations = 50;
    p->residual_threshold = 1e-7;
    p->warm_start = 0;          // disabled in btMultiBodyConstraintSolver [U]
    p->warmstarting_factor = 0.85;
    p->friction_directions = 2;
    p->scaling_factor = 3.14159265358979323846 / 6.0;
    p->gait = 1;
    p->servo_tol = 0.05;
    p->max_counter = 40;
    p->height_threshold = 0.1;
    p->energy_dt = 1.0 / 100.0;
    p->alpha = 1.0; p->beta = 0.01; p->gamma = 0.1;
    p->term_angle = 0.5;
    p->term_index = 9;
    p->collision_force = 10.0;
    p->collision_penalty = -10.0;
    p->done_penalty = -5.0;
    p->contact_order = 0;
    p->reserved0 = 0;
    p->noncontact_order = 0;
    p->contact_erp_rule = 0;
}

int snk_destroy(snk_handle* h);
namespace {
// scheduler state (snk_device.hpp: Sched): the model slot, the rings and counters, the host-mapped alarm word
int init_sched(snk_handle* h) {
    const char* q = getenv("SNK_QUANTUM");       // substeps per slice; 0 = whole env-steps in launch order
    const int quantum = q ? atoi(q) : 1;
    h->model_slot = quantum > 0 ? take_model_slot() : -1;
    h->use_sched = h->model_slot >= 0;
    snk::Sched& sc = h->sched;
    sc.cap = 2u;                                  // power of two >= 2 n_envs: slot = ticket & (cap - 1) survives the
    while (sc.cap < 2u * (uint32_t)h->n_envs) sc.cap <<= 1;      // wrap-around of the 32-bit tickets
    sc.quantum = quantum;
    const char* hy = getenv("SNK_HYST");          // experiments: see snk_device.hpp Sched::hyst
    sc.hyst = hy ? atoi(hy) : 3;
    if (sc.hyst < 1) sc.hyst = 1;
    if (ensure(h, &sc.head, sizeof(uint32_t), 0) || ensure(h, &sc.tail, sizeof(uint32_t), 0) ||
        ensure(h, &sc.waiting, snk::kBuckets * sizeof(int32_t), 0) ||
        ensure(h, &sc.ent, (size_t)sc.cap * sizeof(unsigned long long), 0xFF) ||      // (all bits set: an empty slot)
        ensure(h, &sc.counter, (size_t)h->n_envs * sizeof(int32_t)) || ensure(h, &sc.finished, sizeof(int32_t), 0))
        return 1;
    HIP_TRY(hipHostMalloc(&h->h_alarm, 64 * sizeof(int32_t), hipHostMallocMapped));
    memset(h->h_alarm, 0, 64 * sizeof(int32_t));
    HIP_TRY(hipHostGetDevicePointer((void**)&sc.alarm, h->h_alarm, 0));
#ifdef SNK_SCHED_DEBUG
    if (ensure(h, &sc.wstat, (size_t)h->grid_waves * 8 * sizeof(long long))) return 1;
#endif
    return 0;
}

// everything snk_create allocates; on failure the caller destroys the half-built handle
int init_handle(snk_handle* h, const snk_params* p, int32_t n_envs, int32_t device) {
    h->P = *p;
    h->n_envs = n_envs;
    h->device = device;
    h->n = p->n_modules;
    snk::build_host_model(*p, h->H);
    snk::build_dev_model(*p, h->H, h->D);
    // SNK_POISON=1 (tests): the kernels' LDS images and every fresh device allocation start as NaNs instead of as
    // whatever was there, so that a read of something never written shows in the outputs
    const bool poison = getenv("SNK_POISON") != nullptr;
    h->D.poison = poison ? 1 : 0;
    h->D.hist = 0;
    h->rec = h->D.rec_floats;
    // 16 links: the register-resident solve (the obstacle's contacts take slots out of the ground's 64).
    // SNK_FORCE_STREAMED=1 (diagnostics, tests): the streamed-row kernels for a 16-link handle too
    h->v2 = h->n == 16 && getenv("SNK_FORCE_STREAMED") == nullptr && p->obstacle != 2;      // (a free box: six more
                                                                                            //  components, streamed rows)
    // SNK_MOTORS_APART=1 (cross-checks): the motor rows never ride in the normals' batch (snk_pgs_v2.hpp: substep_v2)
    h->D.motors_apart = getenv("SNK_MOTORS_APART") != nullptr ? 1 : 0;
    // SNK_SUPPORT_SERIAL=1 (cross-checks): the support vertex of a hull by the serial search (snk_contacts.hpp: hull_support)
    h->D.support_serial = getenv("SNK_SUPPORT_SERIAL") != nullptr ? 1 : 0;
    size_t rf = 0, z0 = 0, zn = 0, m0 = 0, m1 = 0;      // the layout of a block of streamed constraint rows (below)
    int rc = dispatch(h, [&](auto k) {
        using LR = snk::Lds<decltype(k)::N, false>;
        h->lds_bytes = sizeof(snk::Lds<decltype(k)::N, decltype(k)::V2>);
        rf = LR::kRowFloats; z0 = (size_t)(LR::kRows - 3) * LR::kRS; zn = 3 * (size_t)LR::kRS; m0 = LR::kMmOff; m1 = LR::kYOff;
        return set_lds_attr(k, h->lds_bytes);
    });
    if (rc) return rc;
    if (resident_waves(h->lds_bytes, device, &h->grid_waves)) return 1;
    if (h->grid_waves <= 0 || h->grid_waves > n_envs) h->grid_waves = n_envs;
    // Every buffer: slot, bytes, fill.  d_rows: one block of streamed constraint rows per RESIDENT WAVE (every
    // step / substep kernel is launched with that many workgroups and strides over the environments): 2048 x 112 KB =
    // 230 MB for 32 links, whatever n_envs is.  (16-link handles on the register-resident solve need them too: a substep
    // whose contacts outgrow its 64 slots goes through the streamed-row solve in place, snk_device.hpp: substep())
    const size_t ne = (size_t)n_envs, f = sizeof(float), nb = (size_t)h->grid_waves, R = (size_t)reset_row_floats(h->n);
    if (ensure(h, &h->d_model, sizeof(snk::DevModel)) ||
        ensure(h, &h->d_recs, ne * h->rec * f, 0) ||
        ensure(h, &h->d_mu, ne * f) ||
        ensure(h, &h->d_order, ne * sizeof(int32_t)) ||
        ensure(h, &h->d_rows, nb * rf * f, poison ? 0xFF : 0) ||
        (p->obstacle == 2 && ensure(h, &h->d_box, ne * snk::kBoxFloats * f)) ||
        ensure(h, &h->d_reset, ne * R * f) ||
        ensure(h, &h->d_links, (size_t)snk::link_rows(h->n) * snk::kLinkFloats * f) ||
        ensure(h, &h->d_ovf, (snk::kOvfCounters + snk::kHistBins) * sizeof(unsigned long long), 0) ||
        (p->contact_model == 1 && ensure(h, &h->d_mf, ne * 2 * h->n * snk::kMfFloats * f, 0)))      // hard reset: empty manifolds
        return 1;
    // what the kernels rely on being zero for good: the last three rows of every block of d_rows (the refill of a
    // skipped friction pair) and the pad columns of the M^-1 block behind the rows
    if (poison)
        for (size_t e = 0; e < nb; e++) {
            HIP_TRY(hipMemsetAsync(h->d_rows + e * rf + z0, 0, zn * f, nullptr));
            HIP_TRY(hipMemsetAsync(h->d_rows + e * rf + m0, 0, (m1 - m0) * f, nullptr));
        }
    // the tables that start from values: ground friction 1 (plane.urdf lateral_friction [U]); the free box where loadURDF
    // puts it (snake.py:84, snake_gait_test.py:51: at rest, identity orientation, empty manifold); the reset poses at the
    // reference's defaults (snake.py:22-24: zeros, quaternion 0 0 0 1)
    HIP_TRY(hipMemcpy(h->d_mu, std::vector<float>(ne, 1.0f).data(), ne * f, hipMemcpyHostToDevice));
    if (h->d_box) {
        std::vector<float> b(ne * snk::kBoxFloats, 0.f);
        for (size_t e = 0; e < ne; e++) {
            float* x = &b[e * snk::kBoxFloats];
            for (int i = 0; i < 3; i++) x[i] = (float)p->obstacle_pos[i];
            x[6] = 1.0f;
        }
        HIP_TRY(hipMemcpy(h->d_box, b.data(), b.size() * f, hipMemcpyHostToDevice));
    }
    std::vector<float> t(ne * R, 0.f);
    for (size_t e = 0; e < ne; e++) t[e * R + 6] = 1.0f;
    HIP_TRY(hipMemcpy(h->d_reset, t.data(), t.size() * f, hipMemcpyHostToDevice));
    std::vector<float> lt((size_t)snk::link_rows(h->n) * snk::kLinkFloats);
    snk::build_link_table(h->H, lt.data());
    HIP_TRY(hipMemcpy(h->d_links, lt.data(), lt.size() * f, hipMemcpyHostToDevice));
    h->plan = getenv("SNK_NO_PLAN") == nullptr;
    if (init_sched(h) || upload_model(h)) return 1;
    // hard reset (snake.py:88-95)
    rc = dispatch(h, [&](auto k) { return launch_reset(k, h, nullptr, nullptr, 1, nullptr); });
    if (rc || snk::launch_ok(nullptr)) return 1;
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

// snk_create's refusals of a parameter set, before anything touches the device
int validate_params(const snk_params* p) {
    if (p->struct_size != (uint32_t)sizeof(snk_params) || p->abi_version != SNK_ABI_VERSION) {
        static char msg[256];
        snprintf(msg, sizeof(msg), "snk_create: snk_params layout mismatch: the caller's struct is %u bytes, ABI version %u; this "
                 "library's is %zu bytes, version %d (fill the struct with snk_default_params of THIS library's header)",
                 p->struct_size, p->abi_version, sizeof(snk_params), SNK_ABI_VERSION);
        return fail(msg);
    }
    if (p->n_modules != 16 && p->n_modules != 32) return fail("snk_create: n_modules must be 16 or 32");
    if (p->hull_sides != 0 && (p->hull_sides < 3 || p->hull_sides > 32))
        return fail("snk_create: hull_sides must be 0 (implicit cylinder) or 3 .. 32");
    if (p->contact_model != 0 && p->contact_model != 1) return fail("snk_create: contact_model must be 0 or 1");
    if (p->obstacle < 0 || p->obstacle > 2) return fail("snk_create: obstacle must be 0, 1 (static box) or 2 (free box)");
    if (p->obstacle == 2 && p->n_modules != 16)
        return fail("snk_create: obstacle 2 (the free box) is built for n_modules 16 (its six velocity components sit behind "
                    "the snake's 22 in the 40-lane solve)");
    if (p->obstacle == 2 && !(p->obstacle_mass > 0.0)) return fail("snk_create: obstacle_mass must be positive");
    if (p->warm_start != 0 && p->warm_start != 1) return fail("snk_create: warm_start must be 0 or 1");
    if (p->friction_directions != 1 && p->friction_directions != 2) return fail("snk_create: friction_directions must be 1 or 2");
    if (p->contact_order < 0) return fail("snk_create: contact_order must be 0 (link order), 1 (reversed), 2 (Bullet's quickSort on equal keys) or k >= 3 (a fixed permutation)");
    if (p->contact_order != 0 && p->contact_model != 1)
        return fail("snk_create: contact_order needs contact_model 1 (it orders the persistent ground manifolds)");
    if (p->noncontact_order != 0 && p->noncontact_order != 1)
        return fail("snk_create: noncontact_order must be 0 (limits, then motors, by joint index) or 1 (Bullet's quickSort on equal keys)");
    if (p->contact_erp_rule != 0 && p->contact_erp_rule != 1)
        return fail("snk_create: contact_erp_rule must be 0 (contact_erp at any depth) or 1 (limit_erp above the split-impulse threshold)");
    if (p->warm_start && p->contact_model != 1)
        return fail("snk_create: warm_start needs contact_model 1 (the impulses live in the persistent contact cache)");
    if (!(p->breaking_threshold > 0.0)) return fail("snk_create: breaking_threshold must be positive");
    if (p->term_index < 0 || p->term_index >= 3 * p->n_modules + 8) return fail("snk_create: term_index out of range");
    return 0;
}
}  // namespace

int snk_create(const snk_params* p, int32_t n_envs, int32_t device, snk_handle** out) {
    if (!p || !out) return fail("snk_create: null argument");
    if (n_envs <= 0) return fail("snk_create: n_envs must be positive");
    if (n_envs >= (1 << 24)) return fail("snk_create: n_envs must be below 2^24 (the step queue packs the env index into 24 bits)");
    if (validate_params(p)) return 1;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail("snk_create: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    snk_handle* h = new snk_handle();
    const int rc = init_handle(h, p, n_envs, device);
    if (rc) {
        const std::string why = snk_last_error();      // snk_destroy's own calls must not overwrite the reason
        snk_destroy(h);
        return fail(why);
    }
    *out = h;
    return 0;
}

int snk_destroy(snk_handle* h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (const snk_handle::Owned& o : h->owned) (void)hipFree(*o.slot);
    if (h->h_alarm) (void)hipHostFree(h->h_alarm);
    release_model_slot(h->model_slot);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    delete h;
    return 0;
}

#ifdef SNK_SCHED_DEBUG
// per resident wave of the last step: ticks (100 MHz) waiting in the queue, ticks alive, slices, substeps
int snk_sched_stats(snk_handle* h, long long* out, int32_t* n_waves) {
    if (enter(h, kIdle)) return 1;
    HIP_TRY(hipMemcpy(out, h->sched.wstat, (size_t)h->grid_waves * 8 * sizeof(long long), hipMemcpyDeviceToHost));
    *n_waves = h->grid_waves;
    return 0;
}
#endif
int32_t snk_num_envs(const snk_handle* h) { return h->n_envs; }
int32_t snk_obs_dim(const snk_handle* h) { return h->D.obs_dim; }
int32_t snk_act_dim(const snk_handle* h) { return h->D.act_dim; }
int32_t snk_state_dim(const snk_handle* h) { return h->D.state_dim; }
int32_t snk_record_floats(const snk_handle* h) { return h->rec; }

int snk_reset(snk_handle* h, const uint8_t* mask_dev, float* obs_dev, void* stream) {
    if (!h) return fail("snk_reset: null handle");
    if (enter(h, kDev | kAlive)) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (dispatch(h, [&](auto k) { return launch_reset(k, h, mask_dev, obs_dev, 0, st); })) return 1;
    return snk::launch_ok(nullptr);
}

int snk_step(snk_handle* h, float* actions_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev,
             int32_t* substeps_dev, int32_t vec_mode, void* stream) {
    if (!h) return fail("snk_step: null handle");
    if (!actions_dev || !obs_dev || !rew_dev || !done_dev) return fail("snk_step: null buffer");
    if (enter(h, kDev | kAlive)) return 1;
    return timed_step(h, actions_dev, obs_dev, rew_dev, done_dev, substeps_dev, vec_mode, (hipStream_t)stream, 0);
}

int snk_step_packed(snk_handle* h, float* actions_dev, float* packed_dev, int32_t row_stride, int32_t* substeps_dev,
                    int32_t vec_mode, void* stream) {
    if (!h) return fail("snk_step_packed: null handle");
    if (!actions_dev || !packed_dev) return fail("snk_step_packed: null buffer");
    if (row_stride < h->D.obs_dim + 2) return fail("snk_step_packed: row_stride must be at least obs_dim + 2");
    if (enter(h, kDev | kAlive)) return 1;
    return timed_step(h, actions_dev, packed_dev, nullptr, nullptr, substeps_dev, vec_mode, (hipStream_t)stream, row_stride);
}

int32_t snk_trace_row_floats(const snk_handle* h) { return h ? trace_row_floats(h->n) : 0; }

int snk_step_traced(snk_handle* h, float* actions_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev,
                    int32_t* substeps_dev, float* trace_dev, int32_t trace_rows, int32_t vec_mode, void* stream) {
    if (!h) return fail("snk_step_traced: null handle");
    if (!actions_dev || !obs_dev || !rew_dev || !done_dev) return fail("snk_step_traced: null buffer");
    if (!substeps_dev) return fail("snk_step_traced: substeps_dev is required (it says how many rows of each env are valid)");
    if (!trace_dev) return fail("snk_step_traced: null trace buffer");
    if (trace_rows < h->P.max_counter + 1) {
        char msg[200];
        snprintf(msg, sizeof(msg), "snk_step_traced: trace_rows %d is less than max_counter + 1 = %d (an env-step runs up to "
                 "that many physics substeps)", (int)trace_rows, (int)h->P.max_counter + 1);
        return fail(msg);
    }
    if (reinterpret_cast<uintptr_t>(trace_dev) % 128 != 0)
        return fail("snk_step_traced: the trace buffer must be 128-byte aligned (a row is a whole number of 128-byte lines)");
    if (enter(h, kDev | kAlive)) return 1;
    return timed_step(h, actions_dev, obs_dev, rew_dev, done_dev, substeps_dev, vec_mode, (hipStream_t)stream, 0, trace_dev,
                      trace_rows);
}

int snk_timing_enable(snk_handle* h, int32_t capacity) {
    if (!h) return fail("null handle");
    if (enter(h, kDev)) return 1;
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    h->ev.clear();
    h->ev_used = 0;
    for (int i = 0; i < 2 * capacity; i++) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        h->ev.push_back(e);
    }
    return 0;
}
int snk_timing_read(snk_handle* h, double* mean_ms, int32_t* count) {
    if (!h) return fail("null handle");
    if (enter(h, kDev)) return 1;
    double sum = 0;
    for (int i = 0; i < h->ev_used; i++) {
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(h->ev[2 * i + 1]));
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[2 * i], h->ev[2 * i + 1]));
        sum += ms;
    }
    if (mean_ms) *mean_ms = h->ev_used ? sum / h->ev_used : 0.0;
    if (count) *count = h->ev_used;
    h->ev_used = 0;
    return 0;
}

int snk_reset_host(snk_handle* h, const uint8_t* mask, float* obs) {
    if (!h) return fail("snk_reset_host: null handle");
    if (enter(h, kDev | kAlive)) return 1;
    const size_t ne = (size_t)h->n_envs;
    snk::HostCall c(h);
    const auto s_mask = c.in(mask, ne);
    const auto s_obs = c.inout(obs, ne * h->D.obs_dim * sizeof(float));      // (unmasked rows come back as they went)
    if (c.stage() && snk_reset(h, s_mask, s_obs, nullptr)) return 1;
    return c.finish("snk_reset_host");
}

// snk_step_host (trace null) and snk_step_traced_host (`who`): the alarm, the upload, the step, the device idle, the alarm
// again, the downloads.  The callers have refused their null arguments.
static int step_host(const char* who, snk_handle* h, float* actions, float* obs, float* rew, uint8_t* done, int32_t* substeps,
                     float* trace, int32_t trace_rows, int32_t vec_mode) {
    if (enter(h, kDev | kAlive)) return 1;
    const size_t ne = (size_t)h->n_envs, f = sizeof(float);
    const size_t tbytes = trace ? ne * (size_t)trace_rows * trace_row_floats(h->n) * f : 0;
    snk::HostCall c(h);
    const auto s_act = c.inout(actions, ne * h->D.act_dim * f);      // (clipped in place)
    const auto s_obs = c.out(obs, ne * h->D.obs_dim * f);
    const auto s_rew = c.out(rew, ne * f);
    const auto s_done = c.out(done, ne);
    const auto s_sub = c.out(substeps, ne * sizeof(int32_t));
    const auto s_trace = c.out(trace, tbytes);
    if (c.stage()) {
        // what the kernel does not write -- the padding of a row, the rows from an env's count on -- comes back as NaNs
        // (all bits set), whatever the caller's buffer held
        if (trace) HIP_TRY(hipMemsetAsync(s_trace, 0xFF, tbytes, nullptr));
        if (trace ? snk_step_traced(h, s_act, s_obs, s_rew, s_done, s_sub, s_trace, trace_rows, vec_mode, nullptr)
                  : snk_step(h, s_act, s_obs, s_rew, s_done, s_sub, vec_mode, nullptr)) return 1;
    }
    if (c.wait(who) || check_alarm(h)) return 1;      // (a step that poisoned the handle downloads nothing)
    return c.download(who);
}

int snk_step_host(snk_handle* h, float* actions, float* obs, float* rew, uint8_t* done, int32_t* substeps,
                  int32_t vec_mode) {
    if (!h) return fail("snk_step_host: null handle");
    if (!actions || !obs || !rew || !done) return fail("snk_step_host: null buffer");
    return step_host("snk_step_host", h, actions, obs, rew, done, substeps, nullptr, 0, vec_mode);
}

int snk_step_traced_host(snk_handle* h, float* actions, float* obs, float* rew, uint8_t* done, int32_t* substeps,
                         float* trace, int32_t trace_rows, int32_t vec_mode) {
    if (!h) return fail("snk_step_traced_host: null handle");
    if (!actions || !obs || !rew || !done || !substeps || !trace) return fail("snk_step_traced_host: null buffer");
    if (trace_rows <= 0) return fail("snk_step_traced_host: trace_rows must be positive");
    return step_host("snk_step_traced_host", h, actions, obs, rew, done, substeps, trace, trace_rows, vec_mode);
}

int snk_substep_host(snk_handle* h, const float* targets, int32_t k, int32_t* info) {
    if (!h || !targets) return fail("snk_substep_host: null argument");
    if (k < 0) return fail("snk_substep_host: k < 0");
    if (enter(h, kDev | kAlive)) return 1;
    const size_t ne = (size_t)h->n_envs;
    snk::HostCall c(h);
    const auto s_tgt = c.in(targets, ne * h->n * sizeof(float));
    const auto s_info = c.out(info, ne * 2 * sizeof(int32_t));
    if (c.stage() && snk_substep(h, s_tgt, k, nullptr, s_info, nullptr)) return 1;
    return c.finish("snk_substep_host");
}

int snk_substep(snk_handle* h, const float* targets_dev, int32_t k, const uint8_t* active_dev, int32_t* info_dev, void* stream) {
    if (!h || !targets_dev) return fail("snk_substep: null argument");
    if (k < 0) return fail("snk_substep: k < 0");
    if (enter(h, kDev | kAlive)) return 1;
    if (dispatch(h, [&](auto v) { return launch_substep(v, h, targets_dev, k, info_dev, active_dev, (hipStream_t)stream); }))
        return 1;
    return snk::launch_ok(nullptr);
}

int snk_observe(snk_handle* h, float* obs_dev, float* height_dev, float* linkpos_dev, void* stream) {
    if (!h) return fail("snk_observe: null handle");
    if (!obs_dev && !height_dev && !linkpos_dev) return fail("snk_observe: obs_dev, height_dev and linkpos_dev are all null");
    if (enter(h, kDev | kAlive)) return 1;
    return launch_obs(h, obs_dev, height_dev, linkpos_dev, (hipStream_t)stream);
}

int snk_get_state(snk_handle* h, float* state, float* aux) {
    if (!h) return fail("snk_get_state: null handle");
    if (enter(h, kState)) return 1;
    const size_t sd = (size_t)h->D.state_dim;
    return rows_get(records(h), {{0, sd, state}, {sd, (size_t)h->n + 2, aux}});
}
int snk_set_state(snk_handle* h, const float* state, const float* aux) {
    if (!h) return fail("snk_set_state: null handle");
    if (enter(h, kState)) return 1;
    const size_t sd = (size_t)h->D.state_dim;
    return rows_set(records(h), {{0, sd, state}, {sd, (size_t)h->n + 2, aux}});
}

int32_t snk_reset_pose_floats(const snk_handle* h) {
    if (!h) { fail("snk_reset_pose_floats: null handle"); return 0; }
    if (enter(h, kAlive)) return 0;
    return 7 + h->n;
}

int snk_get_reset_pose(snk_handle* h, float* pose) {
    if (!h || !pose) return fail("snk_get_reset_pose: null argument");
    if (enter(h, kState)) return 1;
    return rows_get(reset_poses(h), {{0, (size_t)(7 + h->n), pose}});
}
int snk_set_reset_pose(snk_handle* h, const uint8_t* mask, const float* pose) {
    if (!h || !pose) return fail("snk_set_reset_pose: null argument");
    if (enter(h, kState)) return 1;
    const size_t ne = (size_t)h->n_envs, W = (size_t)(7 + h->n);
    // validated before anything is written: a refused call leaves the table as it was
    for (size_t e = 0; e < ne; e++) {
        if (mask && !mask[e]) continue;
        const float* r = pose + e * W;
        char msg[200];
        for (size_t i = 0; i < W; i++)
            if (!std::isfinite(r[i])) {
                if (i < 3) snprintf(msg, sizeof(msg), "snk_set_reset_pose: env %zu: position[%zu] is not finite", e, i);
                else if (i < 7) snprintf(msg, sizeof(msg), "snk_set_reset_pose: env %zu: quaternion[%zu] is not finite", e, i - 3);
                else snprintf(msg, sizeof(msg), "snk_set_reset_pose: env %zu: joint angle[%zu] is not finite", e, i - 7);
                return fail(msg);
            }
        const double nq = std::sqrt((double)r[3] * r[3] + (double)r[4] * r[4] + (double)r[5] * r[5] + (double)r[6] * r[6]);
        if (std::fabs(nq - 1.0) > 1e-3) {
            snprintf(msg, sizeof(msg), "snk_set_reset_pose: env %zu: quaternion has norm %.6g, not 1 (it is stored as given, "
                     "not normalised)", e, nq);
            return fail(msg);
        }
    }
    return rows_set(reset_poses(h), {{0, W, pose}}, mask);
}

int snk_set_reset_pose_dev(snk_handle* h, const uint8_t* mask_dev, const float* pose_dev, void* stream) {
    if (!h || !pose_dev) return fail("snk_set_reset_pose_dev: null argument");
    if (enter(h, kDev | kAlive)) return 1;
    const unsigned blocks = (unsigned)(((size_t)h->n_envs * (size_t)(7 + h->n) + 255) / 256);
    if (dispatch(h, [&](auto k) {
            hipLaunchKernelGGL((snk::reset_pose_copy_kernel<decltype(k)::N>), dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                               h->d_reset, mask_dev, pose_dev, h->n_envs);
            h->rows_of_substep = false;
            return 0;
        })) return 1;
    return snk::launch_ok(nullptr);
}

int32_t snk_manifold_floats(const snk_handle* h) { return (h && h->d_mf) ? 2 * h->n * 29 : 0; }

// per cylinder: host layout manifold_to_host's; device layout link_manifolds'
int snk_get_manifold(snk_handle* h, float* out) {
    if (!h || !out) return fail("snk_get_manifold: null argument");
    if (!h->d_mf) return fail("snk_get_manifold: this handle has contact_model 0 (no contact cache)");
    if (enter(h, kState)) return 1;
    const RowTable t = link_manifolds(h);
    std::vector<float> dev(t.rows * t.stride);
    if (rows_get(t, {{0, t.stride, dev.data()}})) return 1;
    for (size_t c = 0; c < t.rows; c++) manifold_to_host(dev[t.stride * c], &dev[t.stride * c + 4], out + 29 * c);
    return 0;
}
int snk_set_manifold(snk_handle* h, const float* in) {
    if (!h || !in) return fail("snk_set_manifold: null argument");
    if (!h->d_mf) return fail("snk_set_manifold: this handle has contact_model 0 (no contact cache)");
    if (enter(h, kState)) return 1;
    const RowTable t = link_manifolds(h);
    std::vector<float> dev(t.rows * t.stride, 0.f);
    for (size_t c = 0; c < t.rows; c++) dev[t.stride * c] = manifold_from_host(in + 29 * c, &dev[t.stride * c + 4]);
    return rows_set(t, {{0, t.stride, dev.data()}});
}

int snk_get_box(snk_handle* h, float* state, float* manifold) {
    if (!h) return fail("snk_get_box: null handle");
    if (!h->d_box) return fail("snk_get_box: this handle has no free box (obstacle != 2)");
    if (enter(h, kState)) return 1;
    const size_t ne = (size_t)h->n_envs;
    std::vector<float> m(manifold ? ne * kBoxMf : 0);      // (count, points) of every box
    if (rows_get(boxes(h), {{0, kBoxState, state}, {kBoxState, kBoxMf, manifold ? m.data() : nullptr}})) return 1;
    for (size_t e = 0; manifold && e < ne; e++) manifold_to_host(m[kBoxMf * e], &m[kBoxMf * e + 1], manifold + 29 * e);
    return 0;
}
int snk_set_box(snk_handle* h, const float* state, const float* manifold) {
    if (!h) return fail("snk_set_box: null handle");
    if (!h->d_box) return fail("snk_set_box: this handle has no free box (obstacle != 2)");
    if (enter(h, kState)) return 1;
    const size_t ne = (size_t)h->n_envs;
    std::vector<float> m(manifold ? ne * kBoxMf : 0);
    for (size_t e = 0; manifold && e < ne; e++) m[kBoxMf * e] = manifold_from_host(manifold + 29 * e, &m[kBoxMf * e + 1]);
    return rows_set(boxes(h), {{0, kBoxState, state}, {kBoxState, kBoxMf, manifold ? m.data() : nullptr}});
}

int snk_contact_overflow(snk_handle* h, uint64_t* out) {
    if (!h || !out) return fail("snk_contact_overflow: null argument");
    if (enter(h, kDev | kIdle)) return 1;
    unsigned long long v[3];
    HIP_TRY(hipMemcpy(v, h->d_ovf, sizeof(v), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; i++) out[i] = (uint64_t)v[i];
    return 0;
}

int32_t snk_contact_histogram_bins(void) { return snk::kHistBins; }
int snk_contact_histogram_enable(snk_handle* h, int32_t on) {
    if (!h) return fail("snk_contact_histogram_enable: null handle");
    if (enter(h, kDev | kIdle)) return 1;
    h->D.hist = on ? 1 : 0;
    return upload_model(h);
}
int snk_contact_histogram(snk_handle* h, uint64_t* out, int32_t reset) {
    if (!h || !out) return fail("snk_contact_histogram: null argument");
    if (enter(h, kDev | kIdle)) return 1;
    std::vector<unsigned long long> v(snk::kHistBins);
    HIP_TRY(hipMemcpy(v.data(), h->d_ovf + snk::kOvfCounters, v.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < snk::kHistBins; i++) out[i] = (uint64_t)v[i];
    if (reset) HIP_TRY(hipMemset(h->d_ovf + snk::kOvfCounters, 0, v.size() * sizeof(unsigned long long)));
    return 0;
}

int snk_get_obs(snk_handle* h, float* obs) {
    if (!h || !obs) return fail("snk_get_obs: null argument");
    if (enter(h, kState)) return 1;
    snk::HostCall c(h);
    const auto s_obs = c.out(obs, (size_t)h->n_envs * h->D.obs_dim * sizeof(float));
    if (c.stage() && snk_observe(h, s_obs, nullptr, nullptr, nullptr)) return 1;
    return c.finish("snk_get_obs");
}
int snk_mean_height(snk_handle* h, float* out) {
    if (!h || !out) return fail("snk_mean_height: null argument");
    if (enter(h, kState)) return 1;
    snk::HostCall c(h);
    const auto s_height = c.out(out, (size_t)h->n_envs * sizeof(float));
    if (c.stage() && snk_observe(h, nullptr, s_height, nullptr, nullptr)) return 1;
    return c.finish("snk_mean_height");
}
int snk_link_positions(snk_handle* h, float* out) {
    if (!h || !out) return fail("snk_link_positions: null argument");
    if (enter(h, kState)) return 1;
    snk::HostCall c(h);
    const auto s_pos = c.out(out, (size_t)h->n_envs * 3 * (h->n + 1) * sizeof(float));
    if (c.stage() && snk_observe(h, nullptr, nullptr, s_pos, nullptr)) return 1;
    return c.finish("snk_link_positions");
}

int snk_set_ground_friction(snk_handle* h, const float* mu) {
    if (!h || !mu) return fail("snk_set_ground_friction: null argument");
    if (enter(h, kState)) return 1;
    return rows_set(friction(h), {{0, 1, mu}});
}

int snk_joint3_reaction_fz(snk_handle* h, float* out) {
    if (!h || !out) return fail("snk_joint3_reaction_fz: null argument");
    if (enter(h, kState)) return 1;
    return rows_get(records(h), {{rec_joint3_fz(h), 1, out}});
}

int snk_get_ground_friction(snk_handle* h, float* mu) {
    if (!h || !mu) return fail("snk_get_ground_friction: null argument");
    if (enter(h, kDev | kIdle)) return 1;
    return rows_get(friction(h), {{0, 1, mu}});
}

int snk_debug_set_tickets(snk_handle* h, uint32_t base) {
    if (!h) return fail("snk_debug_set_tickets: null handle");
    if (enter(h, kState)) return 1;
    HIP_TRY(hipMemcpy(h->sched.head, &base, sizeof(base), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->sched.tail, &base, sizeof(base), hipMemcpyHostToDevice));
    return 0;
}

int snk_debug_raise_alarm(snk_handle* h) {
    if (!h) return fail("snk_debug_raise_alarm: null handle");
    if (!h->h_alarm) return fail("snk_debug_raise_alarm: this handle has no alarm word");
    // the word is host-mapped memory: the host stores what a wave whose bounded wait ran out would (sched_alarm);
    // a step still running sees it at its next bounded wait and drains
    __atomic_store_n(h->h_alarm, 1, __ATOMIC_SEQ_CST);
    return 0;
}

int snk_debug_noncontact_order(int32_t n_modules, int32_t* out) {
    if (!out) return fail("snk_debug_noncontact_order: null output");
    auto write = [out](auto tab) {
        constexpr int n = (int)(sizeof(tab.motor_at) / sizeof(tab.motor_at[0]));
        for (int k = 0; k < n; k++) {
            out[k] = n + tab.motor_at[k];            // the motors first ...
            out[n + k] = tab.motor_at[k];            // ... then the limits, in the same joint order
        }
        return 0;
    };
    if (n_modules == 16) return write(snk::NoncontactOrder<16>::tab);
    if (n_modules == 32) return write(snk::NoncontactOrder<32>::tab);
    return fail("snk_debug_noncontact_order: n_modules must be 16 or 32");
}

int snk_debug_rows_layout(int32_t n_modules, int32_t* out) {
    if (!out) return fail("snk_debug_rows_layout: null output");
    auto write = [out](auto n) {
        using LR = snk::Lds<decltype(n)::value, false>;
        const int32_t v[14] = {LR::ND, LR::NC, LR::NCT, LR::kRows, LR::kFric, LR::kRS, LR::kMO, LR::kSpec, LR::kGeo,
                               (int32_t)LR::kGeoOff, (int32_t)LR::kMmOff, (int32_t)LR::kYOff, (int32_t)LR::kRowFloats,
                               LR::kBoxBody};
        for (int i = 0; i < 14; i++) out[i] = v[i];
        return 0;
    };
    if (n_modules == 16) return write(std::integral_constant<int, 16>{});
    if (n_modules == 32) return write(std::integral_constant<int, 32>{});
    return fail("snk_debug_rows_layout: n_modules must be 16 or 32");
}

int snk_debug_rows(snk_handle* h, int32_t env, float* out) {
    if (!h || !out) return fail("snk_debug_rows: null argument");
    if (enter(h, kState)) return 1;
    if (env < 0 || env >= h->n_envs) return fail("snk_debug_rows: no such environment");
    if (h->v2)
        return fail("snk_debug_rows: this handle runs the register-resident solve, whose rows never leave registers (the "
                    "streamed-row kernels: 32 links, obstacle 2, SNK_FORCE_STREAMED)");
    if (h->n_envs > h->grid_waves)
        return fail("snk_debug_rows: more environments than resident waves: a workgroup's block of rows is shared by "
                    "several environments");
    if (!h->rows_of_substep)
        return fail("snk_debug_rows: the last launch on this handle was not a substep of every environment (snk_substep_host, "
                    "or snk_substep without a mask): only then has workgroup b run environment b and nothing else");
    size_t rf = 0;
    if (dispatch(h, [&](auto k) { rf = snk::Lds<decltype(k)::N, false>::kRowFloats; return 0; })) return 1;
    HIP_TRY(hipMemcpy(out, h->d_rows + (size_t)env * rf, rf * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int snk_debug_reach_bound(const snk_params* p, float out[3]) {
    if (!p || !out) return fail("snk_debug_reach_bound: null argument");
    if (p->n_modules != 16 && p->n_modules != 32) return fail("snk_debug_reach_bound: n_modules must be 16 or 32");
    const auto m = models_of(*p);
    out[0] = m->D.reach_l; out[1] = m->D.reach_hb; out[2] = snk::kReachSlack;
    return 0;
}

int snk_selftest(int32_t device) {
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail("snk_selftest: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    float* d = nullptr;
    HIP_TRY(hipMalloc(&d, 136 * sizeof(float)));
    hipLaunchKernelGGL(snk::selftest_kernel, dim3(1), dim3(64), 0, nullptr, d);
    if (snk::launch_ok(nullptr)) return 1;
    float o[136];
    HIP_TRY(hipMemcpy(o, d, sizeof(o), hipMemcpyDeviceToHost));
    (void)hipFree(d);
    if (o[4] != 32.f * 33.f / 2.f || o[5] != (64.f * 65.f - 32.f * 33.f) / 2.f) {
        char buf[120];
        snprintf(buf, sizeof(buf), "selftest mismatch: half_reduce lower=%g upper=%g", o[4], o[5]);
        return fail(buf);
    }
    for (int l = 0; l < 64; l++) {
        // half_swap(x, y): a = [x.lo, y.lo], b = [x.hi, y.hi]
        float wa = l < 32 ? (float)(l + 1) : 100.f * (float)(l - 32 + 1);
        float wb = l < 32 ? (float)(l + 32 + 1) : 100.f * (float)(l + 1);
        if (o[8 + l] != wa || o[72 + l] != wb) {
            char buf[160];
            snprintf(buf, sizeof(buf), "selftest mismatch: half_swap lane %d a=%g (want %g) b=%g (want %g)", l, o[8 + l], wa,
                     o[72 + l], wb);
            return fail(buf);
        }
    }
    const float s22 = 22.f * 23.f / 2.f, s64 = 64.f * 65.f / 2.f, s38 = 38.f * 39.f / 4.f;
    if (o[0] != s22 || o[1] != s64 || o[2] != 18.f || o[3] != s38) {
        char buf[160];
        snprintf(buf, sizeof(buf), "selftest mismatch: sum32=%g (want %g) sum64=%g (want %g) bcast=%g (want 18) sum38=%g (want %g)",
                 o[0], s22, o[1], s64, o[2], o[3], s38);
        return fail(buf);
    }
    return 0;
}

int snk_params_derived(const snk_params* p, double* out) {
    if (!p || !out) return fail("snk_params_derived: null argument");
    if (p->n_modules != 16 && p->n_modules != 32) return fail("snk_params_derived: n_modules must be 16 or 32");
    const auto m = models_of(*p);
    const snk::DevModel& D = m->D;
    out[0] = D.break_thr; out[1] = D.cyl_r; out[2] = D.cyl_hl; out[3] = D.cyl_zoff; out[4] = D.margin; out[5] = D.obs_thr;
    return 0;
}

int snk_model_describe(const snk_handle* h, double* out_bodies, double* out_origins) {
    if (!h) return fail("snk_model_describe: null handle");
    const int n = h->n;
    double Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, op[3] = {0, 0, 0};
    for (int b = 0; b <= n; b++) {
        if (out_bodies) {
            double* o = out_bodies + 10 * b;
            o[0] = h->H.mass[b];
            for (int i = 0; i < 3; i++) o[1 + i] = h->H.com[b][i];
            const double* I = h->H.Ib[b];
            o[4] = I[0]; o[5] = I[1]; o[6] = I[2]; o[7] = I[4]; o[8] = I[5]; o[9] = I[8];
        }
        if (b >= 1) {
            double t[3], Rn[9];
            snk::detail::mv(Rp, h->H.pfix[b], t);
            for (int i = 0; i < 3; i++) op[i] += t[i];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) {
                    double s = 0;
                    for (int k = 0; k < 3; k++) s += Rp[3 * i + k] * h->H.Rfix[b][3 * k + j];
                    Rn[3 * i + j] = s;
                }
            memcpy(Rp, Rn, sizeof(Rn));
        }
        if (out_origins)
            for (int i = 0; i < 3; i++) out_origins[3 * b + i] = op[i];
    }
    return 0;
}

}  // extern "C"
