// snk_render_view.hpp -- what the renderer's translation unit (snk_render.hip) may see of a handle.  snk_handle itself
// stays private to snk_api.hip; this is the one host-side seam between the two objects of libsnk.so.  No device code
// here: the step kernels' code object does not change with the renderer.
#pragma once
#include <cstddef>
#include <cstdint>

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

// Fills `v`; non-zero (snk_last_error set) for a poisoned handle.  `sync`: the device idle first, like the state accessors.
__attribute__((visibility("hidden"))) int render_view(snk_handle* h, bool sync, RenderView* v);
// The handle's scratch for the renderer -- the per-image primitive and camera tables -- of at least `need` bytes: the
// handle owns, grows and frees it.  Null (snk_last_error set) when it cannot be had.
__attribute__((visibility("hidden"))) float* render_scratch(snk_handle* h, size_t need);
// snk_last_error's message, from the other object; returns 1
__attribute__((visibility("hidden"))) int api_fail(const char* msg);

}  // namespace snk
