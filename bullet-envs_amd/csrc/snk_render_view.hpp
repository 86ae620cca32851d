// snk_render_view.hpp -- what the other translation units of libsnk.so (snk_render.hip: the renderer; snk_world.hip: link
// states and the env fork) may see of a handle.  snk_handle itself stays private to snk_api.hip; this is the one
// host-side seam between the objects of libsnk.so.  No device code here: the step kernels' code object does not change
// with the renderer or with the world kernels.
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

}  // namespace snk
