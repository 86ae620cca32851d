// snk_dyn.hpp -- the dynamics queries of the tensor seam (include/snk.h, "The dynamics queries": snk_dynamics,
// snk_jacobians): the joint-space inertia M(q), the bias forces h(q, u) and the link Jacobians J(q) of an env, read out of
// the state as it lies.  Read-only query kernels (snk_query.hpp; DESIGN.md, "Adding a query kernel"): one wave per output
// row, no atomics, no waits, no scratch memory, nothing allocated and nothing of the handle's state written.
// Only snk_dyn.hip includes this: the other code objects of libsnk.so have none of it.
//
// Everything is formed on the n + 1 composite bodies of DevModel (merging the fixed joints is exact for rigid bodies), in
// world axes, from what fk_vel leaves per body b: R[b], the joint origin o[b], r[b] = o[b] - o[b-1], the joint axis ax[b],
// the twist (w[b], v[b] = velocity of o[b]) and the velocity-product accelerations zeta[b].  The generalised velocity is
// u = [omega 3 | v of the root origin 3 | qd n]; component d < 6 moves body 0 about / along a world axis through o[0],
// component d >= 6 is joint d - 5: its "screw" is (ang, lin) at the point P.
#pragma once
#include <hip/hip_runtime.h>

#include "snk_query.hpp"

namespace snk {

constexpr int kBiasVelocity = 1, kBiasGravity = 2;      // SNK_BIAS_VELOCITY, SNK_BIAS_GRAVITY
constexpr int kJacPointsPerPass = 4;                    // points staged between two barriers of jacobians_kernel

// the body whose motion component d of u is: 0 for the base's six, d - 5 for a joint
__device__ __forceinline__ int dof_body(int d) { return d < 6 ? 0 : d - 5; }
// component i (0, 1, 2) of a
__device__ __forceinline__ float comp3(f3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }
__device__ __forceinline__ f3 unit3(int i) { return mk3(i == 0 ? 1.f : 0.f, i == 1 ? 1.f : 0.f, i == 2 ? 1.f : 0.f); }

// The screw of component d of u: ang = e_d (d < 3) / 0 (d < 6) / the joint's axis; lin = e_(d-3) for d = 3 .. 5, else 0;
// P = o[dof_body(d)].
template <class LT>
__device__ __forceinline__ void dof_screw(const LT& L, int d, f3& ang, f3& lin, f3& P) {
    const int b = dof_body(d);
    ang = d < 3 ? unit3(d) : (d < 6 ? mk3(0.f, 0.f, 0.f) : ld3(L.ax[b]));
    lin = (d >= 3 && d < 6) ? unit3(d - 3) : mk3(0.f, 0.f, 0.f);
    P = ld3(L.o[b]);
}

// A rigid body's inertia about a point, world axes: mass, first moment h = m (COM - point), second moment I (6, symmetric)
struct Inertia10 {
    float m;
    f3 h;
    float I[6];
};
// body b's own, about its joint origin o[b] (DevModel::Ib is about the body's origin)
template <class LT>
__device__ __forceinline__ Inertia10 body_inertia(const LT& L, const DevModel& M, int b) {
    Inertia10 o;
    o.m = M.mass[b];
    o.h = mulRv(L.R[b], ld3(M.com[b])) * o.m;
    rotSym(L.R[b], M.Ib[b], o.I);
    return o;
}

// One entry of M: the screw (ang, lin at Pl) of the LOWER index against the momentum (n about Ph, f) that the composite
// behind the HIGHER index has under its own unit rate: ang . (n + (Ph - Pl) x f) + lin . f.  Both triangles go through
// this one text with the same operands, contraction off: M == M^T bit for bit.
__device__ __forceinline__ float mass_entry(f3 ang, f3 lin, f3 Pl, f3 n, f3 f, f3 Ph) {
#pragma clang fp contract(off)
    const f3 d = mk3(Ph.x - Pl.x, Ph.y - Pl.y, Ph.z - Pl.z);
    const float tx = n.x + __builtin_fmaf(d.y, f.z, -(d.z * f.y));
    const float ty = n.y + __builtin_fmaf(d.z, f.x, -(d.x * f.z));
    const float tz = n.z + __builtin_fmaf(d.x, f.y, -(d.y * f.x));
    const float a = __builtin_fmaf(ang.z, tz, __builtin_fmaf(ang.y, ty, ang.x * tx));
    const float l = __builtin_fmaf(lin.z, f.z, __builtin_fmaf(lin.y, f.y, lin.x * f.x));
    return a + l;
}

// ----------------------------------------------------------------------------------
// dynamics_kernel: one wave per output row (one env id).  The env's record -> fk_vel -> lane = body forms its own
// inertia about its joint origin, then
//   M  composite-rigid-body.  (a) The suffix composite inertia of bodies b .. n about body b's OWN joint origin, ten
//      numbers shifted one body inward per step: a serial recurrence that the wave evaluates uniformly, the lane of
//      component d keeping the composite of dof_body(d) as it passes.  (Carried about the root instead, the tip joint's
//      1e-4 kg m^2 would be what is left of units of kg m^2.)  (b) lane = component d: its screw and the momentum F_d =
//      Ic S_d of its composite under it, 15 floats into LDS.  (c) lane = column c, a loop over the rows r: entry (r, c) by
//      mass_entry from the lower index's screw and the higher one's momentum -- one of them the lane's own registers, the
//      other a broadcast read -- staged row-major at stage[r nd + c] (consecutive lanes, consecutive banks), which IS the
//      output's layout: the block leaves as consecutive float4s, every 128-byte line whole.
//   h  recursive Newton-Euler at zero acceleration of u.  (a) velocity-product accelerations outward (the prefix sums of
//      zeta; serial, uniform, lane = body keeps its own); (b) lane = body: the wrench I alpha + w x I w + s x m (a - g),
//      m (a_com - g) about its joint origin -- rigid bodies only: none of body_bias's damping terms; (c) the suffix sum
//      inward, shifted joint to joint (serial, uniform, the lane of component d keeps dof_body(d)'s); (d) lane = component:
//      the base's six are the wrench about o[0], a joint's is its axis . moment.  One float per lane goes out.
// flags 3 is ONE pass with both terms in the bodies' wrenches, not the sum of the passes of flags 1 and 2.
// ----------------------------------------------------------------------------------
template <int N, bool V2>
__global__ __launch_bounds__(64) void dynamics_kernel(const DevModel* __restrict__ Mp, const float* __restrict__ recs,
                                                      const int32_t* __restrict__ env_ids, int flags,
                                                      float* __restrict__ mass, float* __restrict__ bias, int n_rows,
                                                      int n_envs) {
    using LT = Lds<N, V2>;
    constexpr int ND = N + 6;
    constexpr int QUADS = ND * ND / 4;
    static_assert(ND * ND % 4 == 0, "an env's block of M is whole quads");
    __shared__ float4 smem_raw[(sizeof(LT) + 15) / 16];
    __shared__ float4 stage4[QUADS];
    __shared__ float scr[ND][17];      // per component: [ang 3 | lin 3 | P 3 | n 3 | f 3 | - -]; 17: lane = component writes without bank conflicts
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    float* stage = reinterpret_cast<float*>(stage4);
    const DevModel& M = *Mp;
    const int lane = threadIdx.x;
    const int bd = dof_body(lane);      // (lanes >= ND: beyond the chain, they keep nothing)
    for (int row = blockIdx.x; row < n_rows; row += gridDim.x) {
        int env;
        const bool known = load_row_env(L, M, recs, env_ids, row, n_envs, lane, env);      // (not known: its outputs are zeros)
        Inertia10 own;
        own.m = 0.f; own.h = mk3(0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 6; i++) own.I[i] = 0.f;
        f3 s = mk3(0.f, 0.f, 0.f);      // the body's COM - o[b]
        if (known && lane <= N) {
            own = body_inertia(L, M, lane);
            s = mulRv(L.R[lane], ld3(M.com[lane]));
        }
        if (mass) {
            float4* dst = reinterpret_cast<float4*>(mass + (size_t)row * ND * ND);
            if (known) {
                if (lane <= N) {
                    float* o = L.IA[lane];
                    o[0] = own.m; st3(o + 1, own.h);
#pragma unroll
                    for (int i = 0; i < 6; i++) o[4 + i] = own.I[i];
                }
                lds_sync();
                // (a) composite of bodies b .. N about o[b]
                Inertia10 c, keep;
                c.m = 0.f; c.h = mk3(0.f, 0.f, 0.f);
#pragma unroll
                for (int i = 0; i < 6; i++) c.I[i] = 0.f;
                keep = c;
#pragma unroll 1
                for (int b = N; b >= 0; b--) {
                    if (b < N) {
                        // about o[b] instead of o[b+1] = o[b] + d: I += (2 h.d + m d.d) 1 - (h d^T + d h^T) - m d d^T, diagonal
                        // terms written without the part that cancels; h += m d
                        const f3 d = ld3(L.r[b + 1]);
                        const f3 h = c.h;
                        const float m = c.m;
                        c.I[0] += 2.f * (h.y * d.y + h.z * d.z) + m * (d.y * d.y + d.z * d.z);
                        c.I[3] += 2.f * (h.x * d.x + h.z * d.z) + m * (d.x * d.x + d.z * d.z);
                        c.I[5] += 2.f * (h.x * d.x + h.y * d.y) + m * (d.x * d.x + d.y * d.y);
                        c.I[1] -= (h.x * d.y + d.x * h.y) + m * d.x * d.y;
                        c.I[2] -= (h.x * d.z + d.x * h.z) + m * d.x * d.z;
                        c.I[4] -= (h.y * d.z + d.y * h.z) + m * d.y * d.z;
                        c.h = h + d * m;
                    }
                    const float* o = L.IA[b];
                    c.m += o[0];
                    c.h = c.h + ld3(o + 1);
#pragma unroll
                    for (int i = 0; i < 6; i++) c.I[i] += o[4 + i];
                    if (bd == b) keep = c;
                }
                // (b) the component's screw and its composite's momentum under it: n = I ang + h x lin, f = m lin + ang x h
                if (lane < ND) {
                    f3 ang, lin, P;
                    dof_screw(L, lane, ang, lin, P);
                    const f3 n = mulSv(keep.I, ang) + cross(keep.h, lin);
                    const f3 f = lin * keep.m + cross(ang, keep.h);
                    float* t = scr[lane];
                    st3(t, ang); st3(t + 3, lin); st3(t + 6, P); st3(t + 9, n); st3(t + 12, f);
                }
                lds_sync();
                // (c) lane = column
                if (lane < ND) {
                    const float* me = scr[lane];
                    const f3 ang = ld3(me), lin = ld3(me + 3), P = ld3(me + 6), n = ld3(me + 9), f = ld3(me + 12);
#pragma unroll 1
                    for (int r = 0; r < ND; r++) {
                        const float* t = scr[r];
                        const bool le = r <= lane;      // the row is the lower index: its screw, this lane's momentum
                        const f3 ta = ld3(t), tl = ld3(t + 3), tP = ld3(t + 6), tn = ld3(t + 9), tf = ld3(t + 12);
                        stage[r * ND + lane] = mass_entry(le ? ta : ang, le ? tl : lin, le ? tP : P, le ? n : tn, le ? f : tf,
                                                          le ? P : tP);
                    }
                }
                lds_sync();
                for (int Q = lane; Q < QUADS; Q += 64) dst[Q] = stage4[Q];
            } else {
                for (int Q = lane; Q < QUADS; Q += 64) dst[Q] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        if (bias) {
            float hv = 0.f;
            if (known) {
                const bool vel = (flags & kBiasVelocity) != 0;
                // (a) alpha_b, a(o[b]) at zero acceleration of u
                f3 al = mk3(0.f, 0.f, 0.f), a = al, kal = al, ka = al;
                if (vel) {
#pragma unroll 1
                    for (int b = 1; b <= N; b++) {
                        a = a + cross(al, ld3(L.r[b])) + ld3(&L.zeta[b][3]);
                        al = al + ld3(&L.zeta[b][0]);
                        if (lane == b) { kal = al; ka = a; }
                    }
                }
                // (b) the body's wrench about o[b]
                if (lane <= N) {
                    const f3 w = vel ? ld3(L.w[lane]) : mk3(0.f, 0.f, 0.f);
                    const f3 ag = mk3(ka.x, ka.y, ka.z - ((flags & kBiasGravity) ? M.gz : 0.f));      // a(o[b]) - g
                    const f3 ac = ag + cross(kal, s) + cross(w, cross(w, s));
                    const f3 nn = mulSv(own.I, kal) + cross(w, mulSv(own.I, w)) + cross(own.h, ag);
                    st3(&L.p[lane][0], nn);
                    st3(&L.p[lane][3], ac * own.m);
                }
                lds_sync();
                // (c) suffix sums inward, the moment about each body's own joint origin
                f3 cN = mk3(0.f, 0.f, 0.f), cF = cN, kN = cN, kF = cN;
#pragma unroll 1
                for (int b = N; b >= 0; b--) {
                    const f3 F = ld3(&L.p[b][3]) + cF;
                    const f3 Nn = ld3(&L.p[b][0]) + cN;
                    if (bd == b) { kN = Nn; kF = F; }
                    cN = Nn + cross(ld3(L.r[b]), F);
                    cF = F;
                }
                // (d)
                hv = lane < 3 ? comp3(kN, lane) : (lane < 6 ? comp3(kF, lane - 3) : dot(ld3(L.ax[lane < ND ? bd : 0]), kN));
            }
            if (lane < ND) bias[(size_t)row * ND + lane] = hv;
        }
        lds_sync();      // (the record, the bodies' wrenches and the stage are read by every lane above: the next env waits)
    }
}

// ----------------------------------------------------------------------------------
// jacobians_kernel: one wave per output row (one env id), lane = column j of J (component j of u).  The lane's screw
// (ang, lin, P) once per row; then per point -- the point's world position from link_row_frame, the same for every lane
// -- six floats: rows 0-2 ang x (x - P) + lin, rows 3-5 ang, zeros for a joint outside the link's body (or a link row
// outside the table).  A point's [6][nd] block is staged row-major, lane = column (consecutive banks), which is the
// output's layout; kJacPointsPerPass points leave together as consecutive float4s.
// ----------------------------------------------------------------------------------
template <int N, bool V2>
__global__ __launch_bounds__(64) void jacobians_kernel(const DevModel* __restrict__ Mp, const float* __restrict__ recs,
                                                       const float* __restrict__ links, const int32_t* __restrict__ env_ids,
                                                       const int32_t* __restrict__ link_rows_in,
                                                       const float* __restrict__ local, int n_points,
                                                       float* __restrict__ jac, int n_rows, int n_envs) {
    using LT = Lds<N, V2>;
    constexpr int ND = N + 6, LR = 3 * N + 2, PP = kJacPointsPerPass;
    constexpr int PQ = 6 * ND / 4;      // quads per point
    static_assert(6 * ND % 4 == 0, "a point's block of J is whole quads");
    __shared__ float4 smem_raw[(sizeof(LT) + 15) / 16];
    __shared__ float4 stage4[PP * PQ];
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    float* stage = reinterpret_cast<float*>(stage4);
    const DevModel& M = *Mp;
    const int lane = threadIdx.x;
    const int col = lane < ND ? lane : 0;
    const int bd = dof_body(col);
    for (int row = blockIdx.x; row < n_rows; row += gridDim.x) {
        int env;
        const bool known = load_row_env(L, M, recs, env_ids, row, n_envs, lane, env);      // (not known: its rows are zeros)
        float4* dst = reinterpret_cast<float4*>(jac + (size_t)row * n_points * 6 * ND);
        f3 ang = mk3(0.f, 0.f, 0.f), lin = ang, P = ang;
        if (known) dof_screw(L, col, ang, lin, P);
#pragma unroll 1
        for (int p0 = 0; p0 < n_points; p0 += PP) {
            const int cnt = n_points - p0 < PP ? n_points - p0 : PP;
#pragma unroll 1
            for (int k = 0; k < cnt; k++) {
                const int p = p0 + k;
                const int lr = link_rows_in[p];
                f3 jv = mk3(0.f, 0.f, 0.f), jw = jv;
                if (known && lr >= 0 && lr < LR) {
                    float Rw[9];
                    f3 ow, cw;
                    const int b = link_row_frame(L, links + (size_t)lr * kLinkFloats, Rw, ow, cw);
                    const f3 x = local ? cw + mulRv(Rw, ld3(local + (size_t)3 * p)) : cw;
                    if (bd <= b) {
                        jv = (col >= 3 && col < 6) ? lin : cross(ang, x - P);
                        jw = ang;
                    }
                }
                if (lane < ND) {
                    float* s = stage + k * 6 * ND + lane;
                    s[0] = jv.x; s[ND] = jv.y; s[2 * ND] = jv.z; s[3 * ND] = jw.x; s[4 * ND] = jw.y; s[5 * ND] = jw.z;
                }
            }
            lds_sync();
            for (int Q = lane; Q < cnt * PQ; Q += 64) dst[(size_t)p0 * PQ + Q] = stage4[Q];
            lds_sync();      // (the stage and the record are read by every lane above: the next pass / env waits for them)
        }
    }
}

// ----------------------------------------------------------------------------------
// impulse_kernel (include/snk.h, "The applied forces": snk_apply_impulse): the one kernel of this unit that WRITES the
// state -- the velocity floats of the record and nothing else.  One wave per env (the mask's byte per env, not an id
// list: two rows of one env would race), in front of whatever steps next; the step kernels do not know of it.
//   Q   lane = component d of u: gen_force[d], plus per point the lane's screw against the point's world wrench,
//       ang . (tau + (x - P) x f) + lin . f where the component moves the link's body (dof_body(d) <= body), else nothing:
//       the operands of jacobians_kernel's column d, so that Q = gen_force + sum_p J_p^T [f_p ; tau_p].  The points are
//       staged kJacPointsPerPass at a time, lane = point: the link's frame (link_row_frame), the wrench turned to world
//       axes (SNK_IMPULSE_LINK_FRAME) and the body, twelve floats, which every lane then reads as broadcasts.
//   M^-1 Q   the articulated-body recursion the substep itself runs (aba_main<FACTOR>, snk_dynamics.hpp) on an image with
//       no velocity in it: zeta = 0, the bodies' bias forces 0, no damping, no gravity -- the joint entries of Q as the
//       joint torques, minus its first six as the base's bias force.  In the device code's own coordinates (world axes,
//       each body about its joint origin, r[b] between neighbours, S_b = [axis ; 0]): inward IA_b, U_b = IA_b S_b, D_b =
//       S_b . U_b and the force recursion, a 6 x 6 inverse at the base, outward the accelerations.  Never a factorisation
//       of the dense M: the tip joints' 1e-4 kg m^2 sit next to whole kg m^2.
//   delta = seconds x that, one float per lane; without SNK_IMPULSE_DRY the record's velocity float becomes u + delta by
//       ONE float32 add (contraction off: not an fma of seconds), stored straight to the record.
// An env whose byte is 0 is neither loaded nor stored; its delta row is zeros.
// ----------------------------------------------------------------------------------
constexpr int kImpulseLinkFrame = 1, kImpulseDry = 2;      // SNK_IMPULSE_LINK_FRAME, SNK_IMPULSE_DRY
constexpr int kWrenchFloats = 9;                           // SNK_WRENCH_FLOATS: [force 3 | torque 3 | point 3]

template <int N, bool V2>
__global__ __launch_bounds__(64) void impulse_kernel(const DevModel* __restrict__ Mp, float* __restrict__ recs,
                                                     const float* __restrict__ links, const uint8_t* __restrict__ active,
                                                     const float* __restrict__ gen_force,
                                                     const int32_t* __restrict__ link_rows_in,
                                                     const float* __restrict__ wrench, int n_points, int flags, float seconds,
                                                     float* __restrict__ delta, int n_envs) {
    using LT = Lds<N, V2>;
    constexpr int ND = N + 6, LR = 3 * N + 2, PP = kJacPointsPerPass;
    __shared__ float4 smem_raw[(sizeof(LT) + 15) / 16];
    __shared__ float pts[PP][12];      // per staged point: [x 3 | f 3 | tau 3 | body (int bits; -1: no such link) | - -]
    LT& L = *reinterpret_cast<LT*>(smem_raw);
    const DevModel& M = *Mp;
    const int lane = threadIdx.x;
    const int col = lane < ND ? lane : 0;
    const int bd = dof_body(col);
    for (int row = blockIdx.x; row < n_envs; row += gridDim.x) {
        if (active && !active[row]) {      // (the same byte for every lane: the wave skips the env as one)
            if (delta && lane < ND) delta[(size_t)row * ND + lane] = 0.f;
            continue;
        }
        int env;
        load_row_env(L, M, recs, nullptr, row, n_envs, lane, env);
        f3 ang, lin, P;
        dof_screw(L, col, ang, lin, P);
        float Q = (gen_force && lane < ND) ? gen_force[(size_t)row * ND + lane] : 0.f;
#pragma unroll 1
        for (int p0 = 0; p0 < n_points; p0 += PP) {
            const int cnt = n_points - p0 < PP ? n_points - p0 : PP;
            if (lane < cnt) {
                const int p = p0 + lane;
                const int lr = link_rows_in[p];
                const float* w = wrench + ((size_t)row * n_points + p) * kWrenchFloats;
                f3 x = mk3(0.f, 0.f, 0.f), f = x, t = x;
                int b = -1;
                if (lr >= 0 && lr < LR) {
                    float Rw[9];
                    f3 ow, cw;
                    b = link_row_frame(L, links + (size_t)lr * kLinkFloats, Rw, ow, cw);
                    f = ld3(w); t = ld3(w + 3); x = ld3(w + 6);
                    if (flags & kImpulseLinkFrame) {
                        f = mulRv(Rw, f); t = mulRv(Rw, t); x = cw + mulRv(Rw, x);
                    }
                }
                float* s = pts[lane];
                st3(s, x); st3(s + 3, f); st3(s + 6, t); s[9] = __int_as_float(b);
            }
            lds_sync();
#pragma unroll 1
            for (int k = 0; k < cnt; k++) {
                const float* s = pts[k];
                const f3 x = ld3(s), f = ld3(s + 3), t = ld3(s + 6);
                if (bd <= __float_as_int(s[9])) Q += dot(ang, t + cross(x - P, f)) + dot(lin, f);
            }
            lds_sync();      // (the stage is read by every lane above: the next pass waits for them)
        }
        // the image aba_main<FACTOR> reads, without velocities: lane = body its inertia about its joint origin (body_bias's
        // layout [[Ibar, m [c]x], [-m [c]x, m 1]]), no bias force, no velocity product; lane = component its entry of Q
        if (lane <= N) {
            const int b = lane;
            const float* R = L.R[b];
            const float m = M.mass[b];
            const f3 cw = mulRv(R, ld3(M.com[b]));
            float Ibar[6];
            rotSym(R, M.Ib[b], Ibar);
            float* IA = L.IA[b];
#pragma unroll
            for (int i = 0; i < 6; i++) IA[i] = Ibar[i];
            const float hx = m * cw.x, hy = m * cw.y, hz = m * cw.z;
            IA[6] = 0.f; IA[7] = -hz; IA[8] = hy;
            IA[9] = hz;  IA[10] = 0.f; IA[11] = -hx;
            IA[12] = -hy; IA[13] = hx; IA[14] = 0.f;
            IA[15] = m; IA[16] = 0.f; IA[17] = 0.f; IA[18] = m; IA[19] = 0.f; IA[20] = m;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                L.zeta[b][i] = 0.f;
                if (b > 0) L.p[b][i] = 0.f;
            }
        }
        if (lane < 6) L.p[0][lane] = -Q;
        else if (lane < ND) L.tauj[lane - 6] = Q;
        lds_sync();
        aba_main<LT, true>(L, M, lane);      // (ends in a barrier: acc0 and qdd are there for every lane)
        if (lane < ND) {
#pragma clang fp contract(off)
            const float dl = seconds * (lane < 6 ? L.acc0[lane] : L.qdd[lane - 6]);
            if (delta) delta[(size_t)row * ND + lane] = dl;
            if (!(flags & kImpulseDry)) {
                const int at = lane < 6 ? 7 + lane : 13 + N + (lane - 6);      // omega, v | qd: the record's order
                recs[(size_t)env * LT::REC + at] = L.rec[at] + dl;
            }
        }
        lds_sync();      // (the record and the sweeps' results are read by every lane above: the next env waits)
    }
}

}  // namespace snk
