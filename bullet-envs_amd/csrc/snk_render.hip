// snk_render.hip -- the batched ray caster behind snk_render / snk_render_host and snk_ray_test / snk_ray_test_host, and
// PyBullet's two camera-matrix helpers (include/snk.h: "The rendered scene", "The ray test").  A translation unit and a code object of its own: build.py compiles it to an
// object and links it into libsnk.so next to snk_api.hip, whose kernels it does not touch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/snk.h"
#include "snk_render.hpp"
#include "snk_seam.hpp"

namespace {

using snk::api_fail;

// what both forms refuse before they look at the handle's state; `who` = the entry point's name
int check_shape(const char* who, const snk_handle* h, int32_t n_images, int32_t width, int32_t height, int32_t flags) {
    const std::string w(who);
    if (!h) return api_fail(w + ": null handle (h)");
    if (n_images < 1) return api_fail(w + ": n_images must be at least 1");
    if (width < 1 || width > 4096) return api_fail(w + ": width must be in 1 .. 4096");
    if (height < 1 || height > 4096) return api_fail(w + ": height must be in 1 .. 4096");
    if ((long long)n_images * width * height > 2147483647LL)
        return api_fail(w + ": n_images x width x height is more than 2^31 - 1 pixels");
    if (flags & ~SNK_RENDER_SHADOW) return api_fail(w + ": unknown bits in flags (SNK_RENDER_SHADOW is the only one)");
    return 0;
}

static_assert(snk::kRayFloats == SNK_RAY_FLOATS && snk::kHitFloats == SNK_HIT_FLOATS, "the kernels' ray and record are the header's");

// the same for both forms of snk_ray_test
int check_rays(const char* who, const snk_handle* h, int32_t n_rows, int32_t n_rays, int32_t flags) {
    const std::string w(who);
    if (!h) return api_fail(w + ": null handle (h)");
    if (n_rows < 1) return api_fail(w + ": n_rows must be at least 1");
    if (n_rays < 1 || n_rays > 65536) return api_fail(w + ": n_rays must be in 1 .. 65536");
    if ((long long)n_rows * n_rays > (1LL << 28)) return api_fail(w + ": n_rows x n_rays is more than 2^28 rays");
    const int32_t kinds = SNK_RAYS_GROUND | SNK_RAYS_SNAKE | SNK_RAYS_BOX;
    if (flags & ~(kinds | SNK_RAYS_SHARED))
        return api_fail(w + ": unknown bits in flags (SNK_RAYS_GROUND, SNK_RAYS_SNAKE, SNK_RAYS_BOX, SNK_RAYS_SHARED)");
    if (!(flags & kinds)) return api_fail(w + ": flags name nothing to hit (SNK_RAYS_GROUND, SNK_RAYS_SNAKE, SNK_RAYS_BOX)");
    return 0;
}
int check_parent(const char* who, int32_t parent_row, int n) {
    if (parent_row >= -1 && parent_row < snk::link_rows(n)) return 0;
    return api_fail(std::string(who) + ": parent_row " + std::to_string(parent_row) + " is outside -1 .. " +
                    std::to_string(snk::link_rows(n) - 1));
}

}  // namespace

extern "C" {

int snk_render(snk_handle* h, const int32_t* env_ids_dev, int32_t n_images, const float* cameras_dev, int32_t shared_camera,
               int32_t width, int32_t height, int32_t flags, uint8_t* rgba_dev, float* depth_dev, int32_t* seg_dev,
               void* stream) {
    if (check_shape("snk_render", h, n_images, width, height, flags)) return 1;
    if (!rgba_dev) return api_fail("snk_render: null rgba_dev");
    if (!cameras_dev) return api_fail("snk_render: null cameras_dev");
    if (reinterpret_cast<uintptr_t>(rgba_dev) % 4 != 0)
        return api_fail("snk_render: rgba_dev must be 4-byte aligned (a pixel is one 32-bit store)");
    snk::RenderView v;
    if (snk::render_view(h, false, &v)) return 1;
    const size_t pf = (size_t)snk::prim_stride(v.n), need = (size_t)n_images * (pf + snk::kCamFloats) * sizeof(float);
    float* prims = snk::render_scratch(h, need);
    if (!prims) return 1;
    float* cams = prims + (size_t)n_images * pf;
    hipStream_t st = (hipStream_t)stream;
    const int shared = shared_camera ? 1 : 0;
    if (snk::launch_variant("snk_render", v.n, v.v2, [&](auto n, auto v2) {
            hipLaunchKernelGGL((snk::render_scene_kernel<decltype(n)::value, decltype(v2)::value>), dim3(snk::grid_for(n_images)),
                               dim3(64), 0, st, v.d_model, v.d_recs, v.d_box, env_ids_dev, cameras_dev, shared, prims, cams,
                               n_images, v.n_envs);
        })) return 1;
    const int tx = (width + snk::kRenderTile - 1) / snk::kRenderTile, ty = (height + snk::kRenderTile - 1) / snk::kRenderTile;
    const long long work = (long long)n_images * tx * ty;
    const unsigned blocks = (unsigned)(work < (1LL << 20) ? work : (1LL << 20));
    hipLaunchKernelGGL(snk::render_rays_kernel, dim3(blocks), dim3(256), 0, st, prims, cams, 2 * v.n, width, height, tx, ty, work,
                       flags, reinterpret_cast<uint32_t*>(rgba_dev), depth_dev, seg_dev);
    return snk::launch_ok("snk_render");
}

int snk_render_host(snk_handle* h, const int32_t* env_ids, int32_t n_images, const float* cameras, int32_t shared_camera,
                    int32_t width, int32_t height, int32_t flags, uint8_t* rgba, float* depth, int32_t* seg) {
    if (check_shape("snk_render_host", h, n_images, width, height, flags)) return 1;
    if (!rgba) return api_fail("snk_render_host: null rgba");
    if (!cameras) return api_fail("snk_render_host: null cameras");
    snk::RenderView v;
    if (snk::render_view(h, true, &v)) return 1;
    if (env_ids ? snk::check_env_ids("snk_render_host", "env_ids", env_ids, n_images, v.n_envs)
                : snk::check_count_without_ids("snk_render_host", "n_images", n_images, v.n_envs)) return 1;
    const size_t ncam = shared_camera ? 1 : (size_t)n_images;
    for (size_t k = 0; k < ncam * 32; k++)
        if (!std::isfinite(cameras[k])) {
            char msg[160];
            snprintf(msg, sizeof(msg), "snk_render_host: cameras[%zu][%zu] is not finite", k / 32, k % 32);
            return api_fail(msg);
        }
    const size_t px = (size_t)n_images * width * height;
    snk::HostCall c(h);
    const auto d_ids = c.in(env_ids, (size_t)n_images * 4);
    const auto d_cam = c.in(cameras, ncam * 32 * 4);
    const auto d_rgba = c.out(rgba, px * 4);
    const auto d_depth = c.out(depth, px * 4);
    const auto d_seg = c.out(seg, px * 4);
    if (c.stage() && snk_render(h, d_ids, n_images, d_cam, shared_camera, width, height, flags, d_rgba, d_depth, d_seg, nullptr))
        return 1;
    return c.finish("snk_render_host");
}

int snk_ray_test(snk_handle* h, const int32_t* env_ids_dev, int32_t n_rows, const float* rays_dev, int32_t n_rays,
                 int32_t parent_row, int32_t flags, float* hits_dev, void* stream) {
    if (check_rays("snk_ray_test", h, n_rows, n_rays, flags)) return 1;
    if (!rays_dev) return api_fail("snk_ray_test: null rays_dev");
    if (reinterpret_cast<uintptr_t>(rays_dev) % 4 != 0) return api_fail("snk_ray_test: rays_dev must be 4-byte aligned");
    if (!hits_dev) return api_fail("snk_ray_test: null hits_dev");
    if (reinterpret_cast<uintptr_t>(hits_dev) % 16 != 0)
        return api_fail("snk_ray_test: hits_dev must be 16-byte aligned (the records leave as 16-byte stores)");
    snk::WorldView v;
    if (snk::world_view(h, false, &v)) return 1;
    if (check_parent("snk_ray_test", parent_row, v.n)) return 1;
    // the render's scratch with the render's growth rule: a row counts as an image, its camera's room left unused
    const size_t pf = (size_t)snk::prim_stride(v.n), need = (size_t)n_rows * (pf + snk::kCamFloats) * sizeof(float);
    float* prims = snk::render_scratch(h, need);
    if (!prims) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (snk::launch_variant("snk_ray_test", v.n, v.v2, [&](auto n, auto v2) {
            hipLaunchKernelGGL((snk::ray_scene_kernel<decltype(n)::value, decltype(v2)::value>), dim3(snk::grid_for(n_rows)),
                               dim3(64), 0, st, v.d_model, v.d_recs, v.d_box, v.d_links, env_ids_dev, parent_row, prims, n_rows,
                               v.n_envs);
        })) return 1;
    const int chunks = (n_rays + snk::kRayChunk - 1) / snk::kRayChunk;
    const long long work = (long long)n_rows * chunks;
    const unsigned blocks = (unsigned)(work < (1LL << 20) ? work : (1LL << 20));
    hipLaunchKernelGGL(snk::ray_cast_kernel, dim3(blocks), dim3(snk::kRayChunk), 0, st, prims, rays_dev,
                       (flags & SNK_RAYS_SHARED) ? 1 : 0, 2 * v.n, n_rays, chunks, work, flags, hits_dev);
    return snk::launch_ok("snk_ray_test");
}

int snk_ray_test_host(snk_handle* h, const int32_t* env_ids, int32_t n_rows, const float* rays, int32_t n_rays,
                      int32_t parent_row, int32_t flags, float* hits) {
    if (check_rays("snk_ray_test_host", h, n_rows, n_rays, flags)) return 1;
    if (!rays) return api_fail("snk_ray_test_host: null rays");
    if (!hits) return api_fail("snk_ray_test_host: null hits");
    snk::WorldView v;
    if (snk::world_view(h, true, &v)) return 1;
    if (check_parent("snk_ray_test_host", parent_row, v.n)) return 1;
    if (env_ids ? snk::check_env_ids("snk_ray_test_host", "env_ids", env_ids, n_rows, v.n_envs)
                : snk::check_count_without_ids("snk_ray_test_host", "n_rows", n_rows, v.n_envs)) return 1;
    const bool shared = (flags & SNK_RAYS_SHARED) != 0;
    const size_t nray = (shared ? 1 : (size_t)n_rows) * (size_t)n_rays, total = (size_t)n_rows * (size_t)n_rays;
    for (size_t k = 0; k < nray * SNK_RAY_FLOATS; k++)
        if (!std::isfinite(rays[k])) {
            char msg[200];
            const size_t ray = k / SNK_RAY_FLOATS;
            if (shared) snprintf(msg, sizeof(msg), "snk_ray_test_host: rays[%zu][%zu] is not finite", ray, k % SNK_RAY_FLOATS);
            else snprintf(msg, sizeof(msg), "snk_ray_test_host: rays[%zu][%zu][%zu] is not finite", ray / (size_t)n_rays,
                          ray % (size_t)n_rays, k % SNK_RAY_FLOATS);
            return api_fail(msg);
        }
    snk::HostCall c(h);
    const auto d_ids = c.in(env_ids, (size_t)n_rows * sizeof(int32_t));
    const auto d_rays = c.in(rays, nray * SNK_RAY_FLOATS * sizeof(float));
    const auto d_hits = c.out(hits, total * SNK_HIT_FLOATS * sizeof(float));
    if (c.stage() && snk_ray_test(h, d_ids, n_rows, d_rays, n_rays, parent_row, flags, d_hits, nullptr)) return 1;
    return c.finish("snk_ray_test_host");
}

int snk_view_matrix_ypr(const float target[3], float distance, float yaw_deg, float pitch_deg, float roll_deg, int32_t up_axis,
                        float out[16]) {
    if (!target || !out) return api_fail("snk_view_matrix_ypr: null argument");
    if (up_axis != 1 && up_axis != 2) return api_fail("snk_view_matrix_ypr: up_axis must be 1 (y) or 2 (z)");
    (void)roll_deg;      // [U] b3ComputeViewMatrixFromYawPitchRoll sets its rollRad to 0: the argument is not used
    const double rad = 0.01745329251994329547;
    const double yaw = yaw_deg * rad, pitch = pitch_deg * rad;
    // [U] eyeRot.setEulerZYX(z, y, x) = Rz Ry Rx: up axis 2 -> (yaw, 0, pitch), the eye at -distance along y, up = z;
    // up axis 1 -> (0, yaw, -pitch), the eye at -distance along z, up = y.  Eye offset AND up vector are rotated, so a
    // pitch of -90 degrees has no degenerate up vector
    const double az = up_axis == 2 ? yaw : 0.0, ay = up_axis == 2 ? 0.0 : yaw, ax = up_axis == 2 ? pitch : -pitch;
    const double cz = cos(az), sz = sin(az), cy = cos(ay), sy = sin(ay), cx = cos(ax), sx = sin(ax);
    const double R[9] = {cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx,
                         sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx,
                         -sy, cy * sx, cy * cx};
    const int fwd = up_axis == 2 ? 1 : 2;
    double eye[3], up[3], f[3], s[3], u[3];
    for (int i = 0; i < 3; i++) {
        eye[i] = R[3 * i + fwd] * -(double)distance + target[i];
        up[i] = R[3 * i + up_axis];
    }
    // [U] b3ComputeViewMatrixFromPositions: f = normalised (target - eye), s = normalised f x up, u = s x f
    double nf = 0, nu = 0, ns = 0;
    for (int i = 0; i < 3; i++) { f[i] = target[i] - eye[i]; nf += f[i] * f[i]; nu += up[i] * up[i]; }
    nf = sqrt(nf); nu = sqrt(nu);
    for (int i = 0; i < 3; i++) { f[i] /= nf; up[i] /= nu; }
    s[0] = f[1] * up[2] - f[2] * up[1]; s[1] = f[2] * up[0] - f[0] * up[2]; s[2] = f[0] * up[1] - f[1] * up[0];
    for (int i = 0; i < 3; i++) ns += s[i] * s[i];
    ns = sqrt(ns);
    for (int i = 0; i < 3; i++) s[i] /= ns;
    u[0] = s[1] * f[2] - s[2] * f[1]; u[1] = s[2] * f[0] - s[0] * f[2]; u[2] = s[0] * f[1] - s[1] * f[0];
    double se = 0, ue = 0, fe = 0;
    for (int i = 0; i < 3; i++) { se += s[i] * eye[i]; ue += u[i] * eye[i]; fe += f[i] * eye[i]; }
    for (int i = 0; i < 3; i++) {
        out[4 * i + 0] = (float)s[i]; out[4 * i + 1] = (float)u[i]; out[4 * i + 2] = (float)-f[i]; out[4 * i + 3] = 0.f;
    }
    out[12] = (float)-se; out[13] = (float)-ue; out[14] = (float)fe; out[15] = 1.f;
    return 0;
}

int snk_projection_fov(float fov_deg, float aspect, float near_val, float far_val, float out[16]) {
    if (!out) return api_fail("snk_projection_fov: null argument");
    // [U] b3ComputeProjectionMatrixFOV.  far == near (the reference's own call, snake.py:317-320) divides by zero: the
    // entries come out infinite, as the formula gives them; nothing is refused here
    const double ys = 1.0 / tan((3.141592538 / 180.0) * (double)fov_deg / 2.0), xs = ys / (double)aspect;
    const double n = near_val, f = far_val;
    for (int i = 0; i < 16; i++) out[i] = 0.f;
    out[0] = (float)xs;
    out[5] = (float)ys;
    out[10] = (float)((n + f) / (n - f));
    out[11] = -1.f;
    out[14] = (float)((2.0 * f * n) / (n - f));
    return 0;
}

}  // extern "C"
