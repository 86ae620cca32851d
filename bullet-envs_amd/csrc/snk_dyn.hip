// snk_dyn.hip -- the dynamics queries behind snk_dynamics / snk_jacobians and their host forms (include/snk.h, "The
// dynamics queries"): mass matrix, bias forces and link Jacobians per env.  A translation unit and a code object of its
// own, like snk_world.hip and snk_render.hip: build.py compiles it to an object and links it into libsnk.so next to
// snk_api.hip, whose kernels it does not touch.  It sees a handle through snk_seam.hpp's world_view and writes nothing of it
// -- but for snk_apply_impulse (include/snk.h, "The applied forces"), the forces' way INTO the state: a kernel of this unit
// that adds M^-1 Q x seconds to the velocity floats of the records, in front of whatever steps next.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/snk.h"
#include "snk_seam.hpp"
#include "snk_dyn.hpp"

namespace {

using snk::api_fail;

// what both forms of snk_dynamics refuse before they look at the handle; 0: nothing
int dynamics_args_refused(const char* who, int32_t n_rows, int32_t flags, const void* mass, const void* bias) {
    const std::string w(who);
    if (n_rows < 1) return api_fail(w + ": n_rows must be at least 1");
    if (flags == 0 || (flags & ~(SNK_BIAS_VELOCITY | SNK_BIAS_GRAVITY)))
        return api_fail(w + ": flags must be SNK_BIAS_VELOCITY, SNK_BIAS_GRAVITY or both");
    if (!mass && !bias) return api_fail(w + ": mass and bias are both null");
    return 0;
}

// ... and of snk_jacobians
int jacobians_args_refused(const char* who, int32_t n_rows, const void* link_rows, int32_t n_points, const void* jac) {
    const std::string w(who);
    if (n_rows < 1) return api_fail(w + ": n_rows must be at least 1");
    if (n_points < 1 || n_points > SNK_JAC_MAX_POINTS)
        return api_fail(w + ": n_points " + std::to_string(n_points) + " is outside 1 .. " + std::to_string(SNK_JAC_MAX_POINTS));
    if (!link_rows) return api_fail(w + ": null link_rows");
    if (!jac) return api_fail(w + ": null jac");
    return 0;
}

// ... and of snk_apply_impulse
int impulse_args_refused(const char* who, const void* gen_force, const void* link_rows, const void* wrench, int32_t n_points,
                         int32_t flags, float seconds, const void* delta) {
    const std::string w(who);
    if (flags & ~(SNK_IMPULSE_LINK_FRAME | SNK_IMPULSE_DRY))
        return api_fail(w + ": flags has bits other than SNK_IMPULSE_LINK_FRAME and SNK_IMPULSE_DRY");
    if (n_points < 0 || n_points > SNK_IMPULSE_MAX_POINTS)
        return api_fail(w + ": n_points " + std::to_string(n_points) + " is outside 0 .. " + std::to_string(SNK_IMPULSE_MAX_POINTS));
    if (n_points > 0 && !link_rows) return api_fail(w + ": null link_rows with n_points " + std::to_string(n_points));
    if (n_points > 0 && !wrench) return api_fail(w + ": null wrench with n_points " + std::to_string(n_points));
    if (!gen_force && n_points == 0) return api_fail(w + ": gen_force is null and n_points is 0: nothing to apply");
    if ((flags & SNK_IMPULSE_DRY) && !delta) return api_fail(w + ": null delta with SNK_IMPULSE_DRY");
    if (!std::isfinite(seconds) || seconds < 0.f) return api_fail(w + ": seconds must be finite and not negative");
    return 0;
}

}  // namespace

extern "C" {

int32_t snk_dyn_dofs(const snk_handle* h) {
    if (!h) { api_fail("snk_dyn_dofs: null handle"); return 0; }
    snk::WorldView v;
    if (snk::world_view(const_cast<snk_handle*>(h), false, &v)) return 0;
    return v.n + 6;
}

int snk_dynamics(snk_handle* h, const int32_t* env_ids_dev, int32_t n_rows, int32_t flags, float* mass_dev, float* bias_dev,
                 void* stream) {
    if (!h) return api_fail("snk_dynamics: null handle (h)");
    if (dynamics_args_refused("snk_dynamics", n_rows, flags, mass_dev, bias_dev)) return 1;
    if (reinterpret_cast<uintptr_t>(mass_dev) % 16 != 0)
        return api_fail("snk_dynamics: mass_dev must be 16-byte aligned (the blocks leave as 16-byte stores)");
    if (reinterpret_cast<uintptr_t>(bias_dev) % 4 != 0) return api_fail("snk_dynamics: bias_dev must be 4-byte aligned");
    snk::WorldView v;
    if (snk::world_view(h, false, &v)) return 1;
    return snk::launch_variant("snk_dynamics", v.n, v.v2, [&](auto n, auto v2) {
        hipLaunchKernelGGL((snk::dynamics_kernel<decltype(n)::value, decltype(v2)::value>), dim3(snk::grid_for(n_rows)), dim3(64), 0,
                           (hipStream_t)stream, v.d_model, v.d_recs, env_ids_dev, flags, mass_dev, bias_dev, n_rows, v.n_envs);
    });
}

int snk_dynamics_host(snk_handle* h, const int32_t* env_ids, int32_t n_rows, int32_t flags, float* mass, float* bias) {
    if (!h) return api_fail("snk_dynamics_host: null handle (h)");
    if (dynamics_args_refused("snk_dynamics_host", n_rows, flags, mass, bias)) return 1;
    snk::WorldView v;
    if (snk::world_view(h, true, &v)) return 1;
    if (env_ids ? snk::check_env_ids("snk_dynamics_host", "env_ids", env_ids, n_rows, v.n_envs)
                : snk::check_count_without_ids("snk_dynamics_host", "n_rows", n_rows, v.n_envs)) return 1;
    const size_t nd = (size_t)v.n + 6;
    snk::HostCall c(h);
    const auto d_ids = c.in(env_ids, (size_t)n_rows * sizeof(int32_t));
    const auto d_mass = c.out(mass, (size_t)n_rows * nd * nd * sizeof(float));
    const auto d_bias = c.out(bias, (size_t)n_rows * nd * sizeof(float));
    if (c.stage() && snk_dynamics(h, d_ids, n_rows, flags, d_mass, d_bias, nullptr)) return 1;
    return c.finish("snk_dynamics_host");
}

int snk_jacobians(snk_handle* h, const int32_t* env_ids_dev, int32_t n_rows, const int32_t* link_rows_dev, const float* local_dev,
                  int32_t n_points, float* jac_dev, void* stream) {
    if (!h) return api_fail("snk_jacobians: null handle (h)");
    if (jacobians_args_refused("snk_jacobians", n_rows, link_rows_dev, n_points, jac_dev)) return 1;
    if (reinterpret_cast<uintptr_t>(jac_dev) % 16 != 0)
        return api_fail("snk_jacobians: jac_dev must be 16-byte aligned (the blocks leave as 16-byte stores)");
    if (reinterpret_cast<uintptr_t>(link_rows_dev) % 4 != 0 || reinterpret_cast<uintptr_t>(local_dev) % 4 != 0)
        return api_fail("snk_jacobians: link_rows_dev and local_dev must be 4-byte aligned");
    snk::WorldView v;
    if (snk::world_view(h, false, &v)) return 1;
    return snk::launch_variant("snk_jacobians", v.n, v.v2, [&](auto n, auto v2) {
        hipLaunchKernelGGL((snk::jacobians_kernel<decltype(n)::value, decltype(v2)::value>), dim3(snk::grid_for(n_rows)), dim3(64), 0,
                           (hipStream_t)stream, v.d_model, v.d_recs, v.d_links, env_ids_dev, link_rows_dev, local_dev, n_points,
                           jac_dev, n_rows, v.n_envs);
    });
}

int snk_jacobians_host(snk_handle* h, const int32_t* env_ids, int32_t n_rows, const int32_t* link_rows, const float* local,
                       int32_t n_points, float* jac) {
    if (!h) return api_fail("snk_jacobians_host: null handle (h)");
    if (jacobians_args_refused("snk_jacobians_host", n_rows, link_rows, n_points, jac)) return 1;
    snk::WorldView v;
    if (snk::world_view(h, true, &v)) return 1;
    if (env_ids ? snk::check_env_ids("snk_jacobians_host", "env_ids", env_ids, n_rows, v.n_envs)
                : snk::check_count_without_ids("snk_jacobians_host", "n_rows", n_rows, v.n_envs)) return 1;
    const int last = snk::link_rows(v.n) - 1;
    for (int p = 0; p < n_points; p++)
        if (link_rows[p] < 0 || link_rows[p] > last)
            return api_fail("snk_jacobians_host: link_rows[" + std::to_string(p) + "] = " + std::to_string(link_rows[p]) +
                            " is outside 0 .. " + std::to_string(last));
    for (int i = 0; local && i < 3 * n_points; i++)
        if (!std::isfinite(local[i]))
            return api_fail("snk_jacobians_host: local[" + std::to_string(i / 3) + "][" + std::to_string(i % 3) + "] is not finite");
    const size_t nd = (size_t)v.n + 6;
    snk::HostCall c(h);
    const auto d_ids = c.in(env_ids, (size_t)n_rows * sizeof(int32_t));
    const auto d_rows = c.in(link_rows, (size_t)n_points * sizeof(int32_t));
    const auto d_local = c.in(local, (size_t)n_points * 3 * sizeof(float));
    const auto d_jac = c.out(jac, (size_t)n_rows * n_points * 6 * nd * sizeof(float));
    if (c.stage() && snk_jacobians(h, d_ids, n_rows, d_rows, d_local, n_points, d_jac, nullptr)) return 1;
    return c.finish("snk_jacobians_host");
}

int snk_apply_impulse(snk_handle* h, const uint8_t* active_dev, const float* gen_force_dev, const int32_t* link_rows_dev,
                      const float* wrench_dev, int32_t n_points, int32_t flags, float seconds, float* delta_dev, void* stream) {
    if (!h) return api_fail("snk_apply_impulse: null handle (h)");
    if (impulse_args_refused("snk_apply_impulse", gen_force_dev, link_rows_dev, wrench_dev, n_points, flags, seconds, delta_dev))
        return 1;
    if (reinterpret_cast<uintptr_t>(gen_force_dev) % 4 != 0 || reinterpret_cast<uintptr_t>(link_rows_dev) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(wrench_dev) % 4 != 0 || reinterpret_cast<uintptr_t>(delta_dev) % 4 != 0)
        return api_fail("snk_apply_impulse: gen_force_dev, link_rows_dev, wrench_dev and delta_dev must be 4-byte aligned");
    snk::WorldView v;
    if (snk::world_view(h, false, &v)) return 1;
    float* recs = v.tables[snk::WorldView::kRecords].d;
    return snk::launch_variant("snk_apply_impulse", v.n, v.v2, [&](auto n, auto v2) {
        hipLaunchKernelGGL((snk::impulse_kernel<decltype(n)::value, decltype(v2)::value>), dim3(snk::grid_for(v.n_envs)), dim3(64), 0,
                           (hipStream_t)stream, v.d_model, recs, v.d_links, active_dev, gen_force_dev, link_rows_dev, wrench_dev,
                           n_points, flags, seconds, delta_dev, v.n_envs);
    });
}

int snk_apply_impulse_host(snk_handle* h, const uint8_t* active, const float* gen_force, const int32_t* link_rows,
                           const float* wrench, int32_t n_points, int32_t flags, float seconds, float* delta) {
    if (!h) return api_fail("snk_apply_impulse_host: null handle (h)");
    if (impulse_args_refused("snk_apply_impulse_host", gen_force, link_rows, wrench, n_points, flags, seconds, delta)) return 1;
    snk::WorldView v;
    if (snk::world_view(h, true, &v)) return 1;
    const int last = snk::link_rows(v.n) - 1;
    for (int p = 0; p < n_points; p++)
        if (link_rows[p] < 0 || link_rows[p] > last)
            return api_fail("snk_apply_impulse_host: link_rows[" + std::to_string(p) + "] = " + std::to_string(link_rows[p]) +
                            " is outside 0 .. " + std::to_string(last));
    const size_t nd = (size_t)v.n + 6, E = (size_t)v.n_envs;
    // (an env whose byte is 0 is not read on the device either: its rows may hold anything)
    for (size_t e = 0; e < E; e++) {
        if (active && !active[e]) continue;
        for (size_t d = 0; gen_force && d < nd; d++)
            if (!std::isfinite(gen_force[e * nd + d]))
                return api_fail("snk_apply_impulse_host: gen_force[" + std::to_string(e) + "][" + std::to_string(d) + "] is not finite");
        for (size_t i = 0; i < (size_t)n_points * SNK_WRENCH_FLOATS; i++)
            if (!std::isfinite(wrench[e * n_points * SNK_WRENCH_FLOATS + i]))
                return api_fail("snk_apply_impulse_host: wrench[" + std::to_string(e) + "][" + std::to_string(i / SNK_WRENCH_FLOATS) +
                                "][" + std::to_string(i % SNK_WRENCH_FLOATS) + "] is not finite");
    }
    snk::HostCall c(h);
    const auto d_active = c.in(active, E);
    const auto d_force = c.in(gen_force, E * nd * sizeof(float));
    const auto d_rows = c.in(link_rows, (size_t)n_points * sizeof(int32_t));
    const auto d_wrench = c.in(wrench, E * n_points * SNK_WRENCH_FLOATS * sizeof(float));
    const auto d_delta = c.out(delta, E * nd * sizeof(float));
    if (c.stage() && snk_apply_impulse(h, d_active, d_force, d_rows, d_wrench, n_points, flags, seconds, d_delta, nullptr)) return 1;
    return c.finish("snk_apply_impulse_host");
}

}  // extern "C"
