// snk_world.hip -- link states, reported contacts, the closest-point query and the env fork behind snk_link_states /
// snk_contacts / snk_closest_points / snk_copy_envs and their host forms, and the host-only link read-outs (include/snk.h).
// A translation unit and a code object of its own, like snk_render.hip: build.py compiles it to an object and links it
// into libsnk.so next to snk_api.hip, whose kernels it does not touch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../include/snk.h"
#include "snk_seam.hpp"
#include "snk_world.hpp"

namespace {

using snk::api_fail;
using snk::launch_ok;

// contact slots of a viewed handle (snk_contact_slots); 0: no contact cache
int contact_slots(const snk::WorldView& v) {
    if (!v.tables[snk::WorldView::kManifolds].d) return 0;
    return 4 * 2 * v.n + (v.tables[snk::WorldView::kBox].d ? 4 : 0);
}

}  // namespace

extern "C" {

int32_t snk_link_state_rows(const snk_handle* h) {
    if (!h) { api_fail("snk_link_state_rows: null handle"); return 0; }
    return snk_obs_dim(h) - 6;      // obs_dim = 3n + 8 (snake.py:163-164); the tree has 3n + 2 links
}

int snk_link_states(snk_handle* h, const int32_t* env_ids_dev, int32_t n_rows, float* out_dev, void* stream) {
    if (!h) return api_fail("snk_link_states: null handle (h)");
    if (n_rows < 1) return api_fail("snk_link_states: n_rows must be at least 1");
    if (!out_dev) return api_fail("snk_link_states: null out_dev");
    if (reinterpret_cast<uintptr_t>(out_dev) % 16 != 0)
        return api_fail("snk_link_states: out_dev must be 16-byte aligned (the rows leave as 16-byte stores)");
    snk::WorldView v;
    if (snk::world_view(h, false, &v)) return 1;
    return snk::launch_variant("snk_link_states", v.n, v.v2, [&](auto n, auto v2) {
        hipLaunchKernelGGL((snk::link_state_kernel<decltype(n)::value, decltype(v2)::value>), dim3(snk::grid_for(n_rows)), dim3(64),
                           0, (hipStream_t)stream, v.d_model, v.d_recs, v.d_links, env_ids_dev, out_dev, n_rows, v.n_envs);
    });
}

int snk_link_states_host(snk_handle* h, const int32_t* env_ids, int32_t n_rows, float* out) {
    if (!h) return api_fail("snk_link_states_host: null handle (h)");
    if (n_rows < 1) return api_fail("snk_link_states_host: n_rows must be at least 1");
    if (!out) return api_fail("snk_link_states_host: null out");
    snk::WorldView v;
    if (snk::world_view(h, true, &v)) return 1;
    if (env_ids ? snk::check_env_ids("snk_link_states_host", "env_ids", env_ids, n_rows, v.n_envs)
                : snk::check_count_without_ids("snk_link_states_host", "n_rows", n_rows, v.n_envs)) return 1;
    snk::HostCall c(h);
    const auto d_ids = c.in(env_ids, (size_t)n_rows * sizeof(int32_t));
    const auto d_out = c.out(out, (size_t)n_rows * snk::link_rows(v.n) * snk::kLinkStateFloats * sizeof(float));
    if (c.stage() && snk_link_states(h, d_ids, n_rows, d_out, nullptr)) return 1;
    return c.finish("snk_link_states_host");
}

int snk_link_inertial_offsets(const snk_params* p, double* out) {
    if (!p || !out) return api_fail("snk_link_inertial_offsets: null argument");
    if (p->n_modules != 16 && p->n_modules != 32) return api_fail("snk_link_inertial_offsets: n_modules must be 16 or 32");
    std::unique_ptr<snk::HostModel> H(new snk::HostModel);      // (the model is large: on the heap)
    snk::build_host_model(*p, *H);
    for (int r = 0; r < snk::link_rows(H->n); r++)
        for (int i = 0; i < 3; i++) out[3 * r + i] = H->link_c[r][i];
    return 0;
}

int32_t snk_contact_slots(const snk_handle* h) {
    if (!h) { api_fail("snk_contact_slots: null handle"); return 0; }
    snk::WorldView v;
    if (snk::world_view(const_cast<snk_handle*>(h), false, &v)) return 0;
    const int slots = contact_slots(v);
    if (!slots) api_fail("snk_contact_slots: this handle has contact_model 0 (no contact cache)");
    return slots;
}

int snk_contacts(snk_handle* h, const int32_t* env_ids_dev, int32_t n_rows, float* points_dev, float* force_dev,
                 int32_t* count_dev, void* stream) {
    if (!h) return api_fail("snk_contacts: null handle (h)");
    if (n_rows < 1) return api_fail("snk_contacts: n_rows must be at least 1");
    if (!points_dev && !force_dev && !count_dev) return api_fail("snk_contacts: points_dev, force_dev and count_dev are all null");
    if (reinterpret_cast<uintptr_t>(points_dev) % 16 != 0)
        return api_fail("snk_contacts: points_dev must be 16-byte aligned (the records leave as 16-byte stores)");
    snk::WorldView v;
    if (snk::world_view(h, false, &v)) return 1;
    if (!contact_slots(v)) return api_fail("snk_contacts: this handle has contact_model 0 (no contact cache)");
    return snk::launch_variant("snk_contacts", v.n, v.v2, [&](auto n, auto v2) {
        hipLaunchKernelGGL((snk::contacts_kernel<decltype(n)::value, decltype(v2)::value>), dim3(snk::grid_for(n_rows)), dim3(64), 0,
                           (hipStream_t)stream, v.d_model, v.d_recs, v.tables[snk::WorldView::kManifolds].d,
                           v.tables[snk::WorldView::kBox].d, env_ids_dev, points_dev, force_dev, count_dev, n_rows, v.n_envs);
    });
}

int snk_contacts_host(snk_handle* h, const int32_t* env_ids, int32_t n_rows, float* points, float* force, int32_t* count) {
    if (!h) return api_fail("snk_contacts_host: null handle (h)");
    if (n_rows < 1) return api_fail("snk_contacts_host: n_rows must be at least 1");
    if (!points && !force && !count) return api_fail("snk_contacts_host: points, force and count are all null");
    snk::WorldView v;
    if (snk::world_view(h, true, &v)) return 1;
    const int slots = contact_slots(v);
    if (!slots) return api_fail("snk_contacts_host: this handle has contact_model 0 (no contact cache)");
    if (env_ids ? snk::check_env_ids("snk_contacts_host", "env_ids", env_ids, n_rows, v.n_envs)
                : snk::check_count_without_ids("snk_contacts_host", "n_rows", n_rows, v.n_envs)) return 1;
    snk::HostCall c(h);
    const auto d_ids = c.in(env_ids, (size_t)n_rows * sizeof(int32_t));
    const auto d_pts = c.out(points, (size_t)n_rows * slots * snk::kContactFloats * sizeof(float));
    const auto d_force = c.out(force, (size_t)n_rows * (2 * v.n + 1) * sizeof(float));
    const auto d_count = c.out(count, (size_t)n_rows * sizeof(int32_t));
    if (c.stage() && snk_contacts(h, d_ids, n_rows, d_pts, d_force, d_count, nullptr)) return 1;
    return c.finish("snk_contacts_host");
}

int snk_contact_links(const snk_params* p, int32_t* out) {
    if (!p || !out) return api_fail("snk_contact_links: null argument");
    if (p->n_modules != 16 && p->n_modules != 32) return api_fail("snk_contact_links: n_modules must be 16 or 32");
    // cylinder c is the collider of INPUT_INTERFACE_k (even c = 2k - 2: Bullet link 3k - 2) or of OUTPUT_BODY_k (odd c =
    // 2k - 1: link 3k) -- build_host_model's cylinder loop, in the link numbering of its link table (row = link + 1)
    for (int c = 0; c < 2 * p->n_modules; c++) out[c] = (c & 1) ? 3 * ((c + 1) / 2) : 3 * (c / 2) + 1;
    return 0;
}

int32_t snk_link_pairs(const snk_handle* h) {
    if (!h) { api_fail("snk_link_pairs: null handle"); return 0; }
    snk::WorldView v;
    if (snk::world_view(const_cast<snk_handle*>(h), false, &v)) return 0;
    return snk::link_pairs_of(2 * v.n);
}

int32_t snk_closest_slots(const snk_handle* h, int32_t max_pairs) {
    if (!h) { api_fail("snk_closest_slots: null handle"); return 0; }
    snk::WorldView v;
    if (snk::world_view(const_cast<snk_handle*>(h), false, &v)) return 0;
    if (max_pairs < 0 || max_pairs > snk::link_pairs_of(2 * v.n)) {
        api_fail("snk_closest_slots: max_pairs " + std::to_string(max_pairs) + " is outside 0 .. " +
                 std::to_string(snk::link_pairs_of(2 * v.n)) + " (snk_link_pairs)");
        return 0;
    }
    return 2 * v.n + max_pairs;
}

namespace {

// what both forms of snk_closest_points refuse before they look at the handle; 0: nothing
int closest_args_refused(const char* who, int32_t n_rows, float distance, int32_t flags, const void* points, const void* clearance,
                         const void* count) {
    const std::string w(who);
    if (n_rows < 1) return api_fail(w + ": n_rows must be at least 1");
    if (!std::isfinite(distance) || distance < 0.f) return api_fail(w + ": distance must be finite and not negative");
    if (flags == 0 || (flags & ~(SNK_PAIRS_BOX | SNK_PAIRS_LINKS)))
        return api_fail(w + ": flags must be SNK_PAIRS_BOX, SNK_PAIRS_LINKS or both");
    if (!points && !clearance && !count) return api_fail(w + ": points, clearance and count are all null");
    return 0;
}
int closest_pairs_refused(const char* who, int32_t max_pairs, int n) {
    if (max_pairs >= 0 && max_pairs <= snk::link_pairs_of(2 * n)) return 0;
    return api_fail(std::string(who) + ": max_pairs " + std::to_string(max_pairs) + " is outside 0 .. " +
                    std::to_string(snk::link_pairs_of(2 * n)) + " (snk_link_pairs)");
}

}  // namespace

int snk_closest_points(snk_handle* h, const int32_t* env_ids_dev, int32_t n_rows, float distance, int32_t flags,
                       int32_t max_pairs, float* points_dev, float* clearance_dev, int32_t* count_dev, void* stream) {
    if (!h) return api_fail("snk_closest_points: null handle (h)");
    if (closest_args_refused("snk_closest_points", n_rows, distance, flags, points_dev, clearance_dev, count_dev)) return 1;
    if (reinterpret_cast<uintptr_t>(points_dev) % 16 != 0)
        return api_fail("snk_closest_points: points_dev must be 16-byte aligned (the records leave as 16-byte stores)");
    snk::WorldView v;
    if (snk::world_view(h, false, &v)) return 1;
    if (closest_pairs_refused("snk_closest_points", max_pairs, v.n)) return 1;
    return snk::launch_variant("snk_closest_points", v.n, v.v2, [&](auto n, auto v2) {
        hipLaunchKernelGGL((snk::closest_points_kernel<decltype(n)::value, decltype(v2)::value>), dim3(snk::grid_for(n_rows)),
                           dim3(64), 0, (hipStream_t)stream, v.d_model, v.d_recs, v.tables[snk::WorldView::kBox].d, env_ids_dev,
                           distance, flags, max_pairs, points_dev, clearance_dev, count_dev, n_rows, v.n_envs);
    });
}

int snk_closest_points_host(snk_handle* h, const int32_t* env_ids, int32_t n_rows, float distance, int32_t flags,
                            int32_t max_pairs, float* points, float* clearance, int32_t* count) {
    if (!h) return api_fail("snk_closest_points_host: null handle (h)");
    if (closest_args_refused("snk_closest_points_host", n_rows, distance, flags, points, clearance, count)) return 1;
    snk::WorldView v;
    if (snk::world_view(h, true, &v)) return 1;
    if (closest_pairs_refused("snk_closest_points_host", max_pairs, v.n)) return 1;
    if (env_ids ? snk::check_env_ids("snk_closest_points_host", "env_ids", env_ids, n_rows, v.n_envs)
                : snk::check_count_without_ids("snk_closest_points_host", "n_rows", n_rows, v.n_envs)) return 1;
    snk::HostCall c(h);
    const auto d_ids = c.in(env_ids, (size_t)n_rows * sizeof(int32_t));
    const auto d_pts = c.out(points, (size_t)n_rows * (2 * v.n + max_pairs) * snk::kContactFloats * sizeof(float));
    const auto d_clr = c.out(clearance, (size_t)n_rows * 2 * 2 * v.n * sizeof(float));
    const auto d_count = c.out(count, (size_t)n_rows * 2 * sizeof(int32_t));
    if (c.stage() && snk_closest_points(h, d_ids, n_rows, distance, flags, max_pairs, d_pts, d_clr, d_count, nullptr)) return 1;
    return c.finish("snk_closest_points_host");
}

int snk_copy_envs(snk_handle* h, const int32_t* src_ids_dev, const int32_t* dst_ids_dev, int32_t n_pairs, int32_t flags,
                  void* stream) {
    if (!h) return api_fail("snk_copy_envs: null handle (h)");
    if (!src_ids_dev || !dst_ids_dev) return api_fail("snk_copy_envs: null id list");
    if (n_pairs < 1) return api_fail("snk_copy_envs: n_pairs must be at least 1");
    if (flags & ~SNK_COPY_RESET_POSE) return api_fail("snk_copy_envs: unknown bits in flags (SNK_COPY_RESET_POSE is the only one)");
    snk::WorldView v;
    if (snk::world_view(h, false, &v)) return 1;
    static_assert((int)snk::WorldView::kTables == snk::kCopyTables, "one slot of the copy per table of the view");
    snk::CopyArgs a;
    for (int t = 0; t < snk::kCopyTables; t++) {
        const bool take = t != snk::WorldView::kResetPose || (flags & SNK_COPY_RESET_POSE);
        a.d[t] = take ? v.tables[t].d : nullptr;
        a.floats[t] = (int)v.tables[t].floats;
    }
    hipLaunchKernelGGL(snk::copy_envs_kernel, dim3(snk::grid_for(n_pairs)), dim3(256), 0, (hipStream_t)stream, a, src_ids_dev, dst_ids_dev,
                       n_pairs, v.n_envs);
    return launch_ok("snk_copy_envs");
}

int snk_copy_envs_host(snk_handle* h, const int32_t* src_ids, const int32_t* dst_ids, int32_t n_pairs, int32_t flags) {
    if (!h) return api_fail("snk_copy_envs_host: null handle (h)");
    if (!src_ids || !dst_ids) return api_fail("snk_copy_envs_host: null id list");
    if (n_pairs < 1) return api_fail("snk_copy_envs_host: n_pairs must be at least 1");
    if (flags & ~SNK_COPY_RESET_POSE)
        return api_fail("snk_copy_envs_host: unknown bits in flags (SNK_COPY_RESET_POSE is the only one)");
    snk::WorldView v;
    if (snk::world_view(h, true, &v)) return 1;
    // validated before anything is written: a refused call leaves every table as it was
    char msg[200];
    if (snk::check_env_ids("snk_copy_envs_host", "src_ids", src_ids, n_pairs, v.n_envs) ||
        snk::check_env_ids("snk_copy_envs_host", "dst_ids", dst_ids, n_pairs, v.n_envs)) return 1;
    std::vector<int> as_dst(v.n_envs, -1), as_src(v.n_envs, -1);      // the first index at which an env is named
    for (int k = 0; k < n_pairs; k++)
        if (as_src[src_ids[k]] < 0) as_src[src_ids[k]] = k;
    for (int k = 0; k < n_pairs; k++) {
        const int d = dst_ids[k];
        if (as_dst[d] >= 0) {
            snprintf(msg, sizeof(msg), "snk_copy_envs_host: dst_ids[%d] = %d repeats dst_ids[%d] (the destinations must be distinct)",
                     k, d, as_dst[d]);
            return api_fail(msg);
        }
        as_dst[d] = k;
        if (as_src[d] >= 0) {
            snprintf(msg, sizeof(msg), "snk_copy_envs_host: dst_ids[%d] = %d is also src_ids[%d] (no env may be both a source and a "
                     "destination)", k, d, as_src[d]);
            return api_fail(msg);
        }
    }
    snk::HostCall c(h);
    const auto d_src = c.in(src_ids, (size_t)n_pairs * sizeof(int32_t));
    const auto d_dst = c.in(dst_ids, (size_t)n_pairs * sizeof(int32_t));
    if (c.stage() && snk_copy_envs(h, d_src, d_dst, n_pairs, flags, nullptr)) return 1;
    return c.finish("snk_copy_envs_host");
}

}  // extern "C"
