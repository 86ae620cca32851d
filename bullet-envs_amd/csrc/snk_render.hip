// snk_render.hip -- the batched ray caster behind snk_render / snk_render_host, and PyBullet's two camera-matrix helpers
// (include/snk.h: "The rendered scene").  A translation unit and a code object of its own: build.py compiles it to an
// object and links it into libsnk.so next to snk_api.hip, whose kernels it does not touch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/snk.h"
#include "snk_render.hpp"
#include "snk_render_view.hpp"

namespace {

int rfail(const std::string& msg) { return snk::api_fail(msg.c_str()); }

// what both forms refuse before they look at the handle's state; `who` = the entry point's name
int check_shape(const char* who, const snk_handle* h, int32_t n_images, int32_t width, int32_t height, int32_t flags) {
    const std::string w(who);
    if (!h) return rfail(w + ": null handle (h)");
    if (n_images < 1) return rfail(w + ": n_images must be at least 1");
    if (width < 1 || width > 4096) return rfail(w + ": width must be in 1 .. 4096");
    if (height < 1 || height > 4096) return rfail(w + ": height must be in 1 .. 4096");
    if ((long long)n_images * width * height > 2147483647LL)
        return rfail(w + ": n_images x width x height is more than 2^31 - 1 pixels");
    if (flags & ~SNK_RENDER_SHADOW) return rfail(w + ": unknown bits in flags (SNK_RENDER_SHADOW is the only one)");
    return 0;
}

template <int N, bool V2>
void launch_scene(const snk::RenderView& v, const int32_t* ids, const float* cams_in, int shared, float* prims, float* cams,
                  int n_images, hipStream_t st) {
    const int blocks = n_images < 65536 ? n_images : 65536;
    hipLaunchKernelGGL((snk::render_scene_kernel<N, V2>), dim3(blocks), dim3(64), 0, st, v.d_model, v.d_recs, v.d_box, ids,
                       cams_in, shared, prims, cams, n_images, v.n_envs);
}

}  // namespace

extern "C" {

int snk_render(snk_handle* h, const int32_t* env_ids_dev, int32_t n_images, const float* cameras_dev, int32_t shared_camera,
               int32_t width, int32_t height, int32_t flags, uint8_t* rgba_dev, float* depth_dev, int32_t* seg_dev,
               void* stream) {
    if (check_shape("snk_render", h, n_images, width, height, flags)) return 1;
    if (!rgba_dev) return rfail("snk_render: null rgba_dev");
    if (!cameras_dev) return rfail("snk_render: null cameras_dev");
    if (reinterpret_cast<uintptr_t>(rgba_dev) % 4 != 0)
        return rfail("snk_render: rgba_dev must be 4-byte aligned (a pixel is one 32-bit store)");
    snk::RenderView v;
    if (snk::render_view(h, false, &v)) return 1;
    const size_t pf = (size_t)snk::prim_stride(v.n), need = (size_t)n_images * (pf + snk::kCamFloats) * sizeof(float);
    float* prims = snk::render_scratch(h, need);
    if (!prims) return 1;
    float* cams = prims + (size_t)n_images * pf;
    hipStream_t st = (hipStream_t)stream;
    const int shared = shared_camera ? 1 : 0;
    if (v.n == 16 && v.v2) launch_scene<16, true>(v, env_ids_dev, cameras_dev, shared, prims, cams, n_images, st);
    else if (v.n == 16) launch_scene<16, false>(v, env_ids_dev, cameras_dev, shared, prims, cams, n_images, st);
    else if (v.n == 32) launch_scene<32, false>(v, env_ids_dev, cameras_dev, shared, prims, cams, n_images, st);
    else return rfail("snk_render: unsupported n_modules (16 or 32)");
    const int tx = (width + snk::kRenderTile - 1) / snk::kRenderTile, ty = (height + snk::kRenderTile - 1) / snk::kRenderTile;
    const long long work = (long long)n_images * tx * ty;
    const unsigned blocks = (unsigned)(work < (1LL << 20) ? work : (1LL << 20));
    hipLaunchKernelGGL(snk::render_rays_kernel, dim3(blocks), dim3(256), 0, st, prims, cams, 2 * v.n, width, height, tx, ty, work,
                       flags, reinterpret_cast<uint32_t*>(rgba_dev), depth_dev, seg_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rfail(std::string("snk_render: kernel launch: ") + hipGetErrorString(e));
    return 0;
}

int snk_render_host(snk_handle* h, const int32_t* env_ids, int32_t n_images, const float* cameras, int32_t shared_camera,
                    int32_t width, int32_t height, int32_t flags, uint8_t* rgba, float* depth, int32_t* seg) {
    if (check_shape("snk_render_host", h, n_images, width, height, flags)) return 1;
    if (!rgba) return rfail("snk_render_host: null rgba");
    if (!cameras) return rfail("snk_render_host: null cameras");
    snk::RenderView v;
    if (snk::render_view(h, true, &v)) return 1;
    char msg[160];
    if (env_ids)
        for (int k = 0; k < n_images; k++)
            if (env_ids[k] < 0 || env_ids[k] >= v.n_envs) {
                snprintf(msg, sizeof(msg), "snk_render_host: env_ids[%d] = %d is outside 0 .. %d", k, (int)env_ids[k], v.n_envs - 1);
                return rfail(msg);
            }
    if (!env_ids && n_images > v.n_envs) {
        snprintf(msg, sizeof(msg), "snk_render_host: n_images %d without env_ids is more than the handle's %d envs", (int)n_images, v.n_envs);
        return rfail(msg);
    }
    const size_t ncam = shared_camera ? 1 : (size_t)n_images;
    for (size_t k = 0; k < ncam * 32; k++)
        if (!std::isfinite(cameras[k])) {
            snprintf(msg, sizeof(msg), "snk_render_host: cameras[%zu][%zu] is not finite", k / 32, k % 32);
            return rfail(msg);
        }
    const size_t px = (size_t)n_images * width * height;
    int32_t* d_ids = nullptr;
    float* d_cam = nullptr;
    uint8_t* d_rgba = nullptr;
    float* d_depth = nullptr;
    int32_t* d_seg = nullptr;
    int rc = 1;
    do {
        if (env_ids && (hipMalloc(&d_ids, (size_t)n_images * 4) != hipSuccess ||
                        hipMemcpy(d_ids, env_ids, (size_t)n_images * 4, hipMemcpyHostToDevice) != hipSuccess)) break;
        if (hipMalloc(&d_cam, ncam * 32 * 4) != hipSuccess ||
            hipMemcpy(d_cam, cameras, ncam * 32 * 4, hipMemcpyHostToDevice) != hipSuccess) break;
        if (hipMalloc(&d_rgba, px * 4) != hipSuccess) break;
        if (depth && hipMalloc(&d_depth, px * 4) != hipSuccess) break;
        if (seg && hipMalloc(&d_seg, px * 4) != hipSuccess) break;
        rc = 2;
        if (snk_render(h, d_ids, n_images, d_cam, shared_camera, width, height, flags, d_rgba, d_depth, d_seg, nullptr)) break;
        rc = 1;
        if (hipDeviceSynchronize() != hipSuccess) break;
        if (hipMemcpy(rgba, d_rgba, px * 4, hipMemcpyDeviceToHost) != hipSuccess) break;
        if (depth && hipMemcpy(depth, d_depth, px * 4, hipMemcpyDeviceToHost) != hipSuccess) break;
        if (seg && hipMemcpy(seg, d_seg, px * 4, hipMemcpyDeviceToHost) != hipSuccess) break;
        rc = 0;
    } while (0);
    (void)hipFree(d_ids); (void)hipFree(d_cam); (void)hipFree(d_rgba); (void)hipFree(d_depth); (void)hipFree(d_seg);
    if (rc == 1) return rfail(std::string("snk_render_host: ") + hipGetErrorString(hipGetLastError()));
    return rc ? 1 : 0;
}

int snk_view_matrix_ypr(const float target[3], float distance, float yaw_deg, float pitch_deg, float roll_deg, int32_t up_axis,
                        float out[16]) {
    if (!target || !out) return rfail("snk_view_matrix_ypr: null argument");
    if (up_axis != 1 && up_axis != 2) return rfail("snk_view_matrix_ypr: up_axis must be 1 (y) or 2 (z)");
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
    if (!out) return rfail("snk_projection_fov: null argument");
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
