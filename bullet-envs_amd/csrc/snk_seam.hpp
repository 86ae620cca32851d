// snk_seam.hpp -- what the other translation units of libsnk.so (snk_render.hip: the renderer; snk_world.hip: link
// states, contacts and the env fork; snk_dyn.hip: mass matrix, bias forces, link Jacobians) may see of a handle, and the
// host scaffolding every entry-point pair shares.  snk_handle itself stays private to snk_api.hip; this is the one
// host-side seam between the objects of libsnk.so, and HostCall, on the handle's one staging arena (stage_arena), is the
// host form of EVERY entry-point pair, snk_api.hip's too.  No device code here: the step kernels' code object does not
// change with the renderer or with the world kernels.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cassert>
#include <cstddef>
#include <cstdint>
#include <string>
#include <type_traits>

#include "snk_model.hpp"

struct snk_handle;

namespace snk {

struct RenderView {
    int device, n, n_envs;
    bool v2;                      // which LDS image the handle's kernels use (Lds<N, V2>)
    const DevModel* D;            // host copy of the model (obstacle, ncyl)
    const DevModel* d_model;      // the same on the device
    const float* d_recs;          // [n_envs][rec] state records
    const float* d_box;           // obstacle 2: [n_envs][kBoxFloats], else null
};

// One per-environment table of the simulator state as the fork moves it: `floats` floats per env, padding included
// (d null: the handle has no such table).
struct EnvTable { float* d; size_t floats; };
// What snk_world.hip sees: the renderer's view, the link table (build_link_table) on the device, and EVERY table that
// Snapshot (_lib.py) calls simulator state, by the handle's own row-table accessors -- a table added there is added here.
struct WorldView : RenderView {
    const float* d_links;         // [link_rows(n)][kLinkFloats]
    enum { kRecords, kManifolds, kBox, kFriction, kResetPose, kTables };
    EnvTable tables[kTables];
};

// Fills `v`; non-zero (snk_last_error set) for a poisoned handle.  `sync`: the device idle first, like the state accessors.
__attribute__((visibility("hidden"))) int render_view(snk_handle* h, bool sync, RenderView* v);
__attribute__((visibility("hidden"))) int world_view(snk_handle* h, bool sync, WorldView* v);
// The handle's scratch for the renderer -- the per-image primitive and camera tables -- of at least `need` bytes: the
// handle owns, grows and frees it.  Null (snk_last_error set) when it cannot be had.
__attribute__((visibility("hidden"))) float* render_scratch(snk_handle* h, size_t need);
// The handle's staging arena -- the device side of every host form (HostCall, below) -- of at least `need` bytes, made on
// the first host-form call and replaced, contents not kept, when a call needs more: the handle owns, grows and frees it.
// Only calls that wait for the device before they return use it (which is why the renderer's scratch, read by the
// asynchronous snk_render after it has returned, is not part of it).  Null (snk_last_error set) when it cannot be had.
__attribute__((visibility("hidden"))) void* stage_arena(snk_handle* h, size_t need);
// snk_last_error's message, from the other object; returns 1
__attribute__((visibility("hidden"))) int api_fail(const char* msg);
inline int api_fail(const std::string& msg) { return api_fail(msg.c_str()); }

// Behind a launch: 0, or hipGetLastError() reported as "<who>: kernel launch: <text>" (who null: without the prefix).
inline int launch_ok(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    return api_fail((who ? std::string(who) + ": " : std::string()) + "kernel launch: " + hipGetErrorString(e));
}

// blocks of a kernel that strides over n work items, one per block
inline int grid_for(int n) { return n < 65536 ? n : 65536; }

// fn(integral_constant<int, N>{}, bool_constant<V2>{}) for the kernel variant (chain length n, register-resident solve
// v2) -- THE list of the variants libsnk.so instantiates -- and its result; kUnsupported for any other, which the caller
// reports in its own words.
constexpr int kUnsupported = -1;
template <class F>
int for_variant(int n, bool v2, F&& fn) {
    if (n == 16 && v2) return fn(std::integral_constant<int, 16>{}, std::true_type{});
    if (n == 16) return fn(std::integral_constant<int, 16>{}, std::false_type{});
    if (n == 32 && !v2) return fn(std::integral_constant<int, 32>{}, std::false_type{});
    return kUnsupported;
}

// The tail of a device form: launch(integral_constant<int, N>{}, bool_constant<V2>{}) enqueues the variant's kernel.
// 0, or "<who>: unsupported n_modules (16 or 32)" / launch_ok(who)'s report.
template <class F>
int launch_variant(const char* who, int n, bool v2, F&& launch) {
    if (for_variant(n, v2, [&](auto N, auto V2) { launch(N, V2); return 0; }) == kUnsupported)
        return api_fail(std::string(who) + ": unsupported n_modules (16 or 32)");
    return launch_ok(who);
}

// A host id list (null: none) against the handle: 0, or the first id outside 0 .. n_envs - 1 reported.
inline int check_env_ids(const char* who, const char* list_name, const int32_t* ids, int n, int n_envs) {
    for (int k = 0; ids && k < n; k++)
        if (ids[k] < 0 || ids[k] >= n_envs)
            return api_fail(std::string(who) + ": " + list_name + "[" + std::to_string(k) + "] = " + std::to_string(ids[k]) +
                            " is outside 0 .. " + std::to_string(n_envs - 1));
    return 0;
}
// A call without an id list names envs 0 .. n - 1: 0, or n > n_envs reported.
inline int check_count_without_ids(const char* who, const char* count_name, int n, int n_envs) {
    if (n <= n_envs) return 0;
    return api_fail(std::string(who) + ": " + count_name + " " + std::to_string(n) + " without env_ids is more than the handle's " +
                    std::to_string(n_envs) + " envs");
}

// The carve arithmetic of the staging arena, host only: offsets[i] of entry i (bytes[i] bytes; 0: an entry that takes no
// room and shares its neighbour's offset) in whole kStageAlign-byte units -- the alignment a device allocation of its
// own had, more than the 16 bytes the record stores and the 128 the trace rows need -- and the total, all in size_t.
constexpr size_t kStageAlign = 256;
inline size_t stage_carve(const size_t* bytes, size_t n, size_t* offsets) {
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        offsets[i] = total;
        total += (bytes[i] + kStageAlign - 1) / kStageAlign * kStageAlign;
    }
    return total;
}

// THE host form of an entry-point pair: device copies of the caller's arrays for one call of the device form on the null
// stream, carved from the handle's staging arena (stage_arena).  Nothing is allocated or freed per call, on the device or
// on the host: up to kMaxEntries arrays, declared in place.  in / out / inout DECLARE the arrays (a null host pointer
// stays null) and return a Staged<T>, which turns into the device pointer once stage() has sized the arena -- once, for
// the sum: a grown arena keeps nothing -- and uploaded the inputs; converting one earlier is a programming error and
// asserts (keep them `auto`).  After a failed allocation or copy every Staged gives null and nothing more touches the
// device; stage() says whether the device form may run, and finish (= wait, then download) reports the failure as
// "<who>: <hipGetErrorString>".
class HostCall {
    static constexpr size_t kMaxEntries = 8;
    snk_handle* h_;
    size_t n_ = 0;
    const void* up_[kMaxEntries];      // the host array to upload, or null
    void* down_[kMaxEntries];          // the host array to fill, or null
    size_t bytes_[kMaxEntries], offsets_[kMaxEntries];
    char* base_ = nullptr;
    bool staged_ = false, bad_ = false;
    size_t declare(const void* up, void* down, size_t bytes) {
        assert(n_ < kMaxEntries && !staged_);
        up_[n_] = up; down_[n_] = down; bytes_[n_] = (up || down) ? bytes : 0;
        return n_++;
    }
    void* dev(size_t i) const {
        assert(staged_);
        return (base_ && !bad_ && bytes_[i]) ? base_ + offsets_[i] : nullptr;
    }
    int report(const char* who) const { return api_fail(std::string(who) + ": " + hipGetErrorString(hipGetLastError())); }

public:
    template <class T>
    class Staged {
        friend class HostCall;
        const HostCall* c_;
        size_t i_;
        Staged(const HostCall* c, size_t i) : c_(c), i_(i) {}
    public:
        operator T*() const { return static_cast<T*>(c_->dev(i_)); }
    };
    explicit HostCall(snk_handle* h) : h_(h) {}
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;
    // a device copy of host[0 .. bytes)
    template <class T>
    Staged<const T> in(const T* host, size_t bytes) { return {this, declare(host, nullptr, bytes)}; }
    // a device buffer of `bytes` that download copies to host
    template <class T>
    Staged<T> out(T* host, size_t bytes) { return {this, declare(nullptr, host, bytes)}; }
    // both: host[0 .. bytes) goes up and comes back
    template <class T>
    Staged<T> inout(T* host, size_t bytes) { return {this, declare(host, host, bytes)}; }
    // sizes the arena for everything declared, then uploads the inputs in the order of their declaration; true: the
    // device form may run
    bool stage() {
        const size_t total = stage_carve(bytes_, n_, offsets_);
        base_ = total ? static_cast<char*>(stage_arena(h_, total)) : nullptr;
        staged_ = true;
        bad_ = total && !base_;
        for (size_t i = 0; !bad_ && i < n_; i++)
            if (up_[i] && bytes_[i])
                bad_ = hipMemcpy(base_ + offsets_[i], up_[i], bytes_[i], hipMemcpyHostToDevice) != hipSuccess;
        return !bad_;
    }
    // waits for the device
    int wait(const char* who) { return (!bad_ && hipDeviceSynchronize() == hipSuccess) ? 0 : report(who); }
    // fills every out's host array, in the order of their declaration
    int download(const char* who) {
        for (size_t i = 0; staged_ && i < n_; i++)
            if (void* d = down_[i] ? dev(i) : nullptr)
                if (hipMemcpy(down_[i], d, bytes_[i], hipMemcpyDeviceToHost) != hipSuccess) return report(who);
        return 0;
    }
    int finish(const char* who) { return wait(who) ? 1 : download(who); }
};

}  // namespace snk
