// snk_seam.hpp -- what the other translation units of libsnk.so (snk_render.hip: the renderer; snk_world.hip: link
// states, contacts and the env fork; snk_dyn.hip: mass matrix, bias forces, link Jacobians) may see of a handle, and the host scaffolding every entry-point pair shares.
// snk_handle itself stays private to snk_api.hip; this is the one host-side seam between the objects of libsnk.so.  No
// device code here: the step kernels' code object does not change with the renderer or with the world kernels.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

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

// THE host form of an entry-point pair: device copies of the caller's arrays for one call of the device form on the
// null stream, freed on every way out.  After a failed allocation or copy, in / out give null and touch the device no
// more; ok() says whether the device form may run, and finish reports the failure as "<who>: <hipGetErrorString>".
class HostCall {
    struct Out { void* host; void* dev; size_t bytes; };
    std::vector<void*> owned_;
    std::vector<Out> outs_;
    bool bad_ = false;
    void* alloc(size_t bytes) {
        void* d = nullptr;
        if (bad_ || hipMalloc(&d, bytes) != hipSuccess) { bad_ = true; return nullptr; }
        owned_.push_back(d);
        return d;
    }

public:
    HostCall() = default;
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;
    ~HostCall() { for (void* d : owned_) (void)hipFree(d); }
    bool ok() const { return !bad_; }
    // a device copy of host[0 .. bytes); null when host is null
    template <class T>
    T* in(const T* host, size_t bytes) {
        void* d = host ? alloc(bytes) : nullptr;
        if (d && hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) { bad_ = true; return nullptr; }
        return static_cast<T*>(d);
    }
    // a device buffer of `bytes` that finish copies to host; null when host is null
    template <class T>
    T* out(T* host, size_t bytes) {
        void* d = host ? alloc(bytes) : nullptr;
        if (d) outs_.push_back({host, d, bytes});
        return static_cast<T*>(d);
    }
    // waits for the device, then fills every out's host array, in the order of the out calls
    int finish(const char* who) {
        bool good = !bad_ && hipDeviceSynchronize() == hipSuccess;
        for (size_t i = 0; good && i < outs_.size(); i++)
            good = hipMemcpy(outs_[i].host, outs_[i].dev, outs_[i].bytes, hipMemcpyDeviceToHost) == hipSuccess;
        return good ? 0 : api_fail(std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
    }
};

}  // namespace snk
