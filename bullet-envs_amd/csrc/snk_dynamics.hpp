// snk_dynamics.hpp -- the chain's dynamics on an LDS image, shared by both solves: forward kinematics and link velocities,
// checkSnakeHeight's mean height, the per-body bias forces, the articulated-body sweeps, and the rule for when a substep
// needs its sensor pass.
#pragma once
#include "snk_lds.hpp"
#include "snk_model.hpp"
#include "snk_wave.hpp"

namespace snk {

// ----------------------------------------------------------------------------------
// S1: forward kinematics + link velocities of the chain.  The chain over the bodies is a serial recurrence; within a
// body step one lane owns one component (lane c < 3 of every quad: row c of R in three registers, component c of every
// 3-vector), so that a vector operation is one instruction, R_parent Rfix nine, and a cross product two: its (y,z,x) and
// (z,x,y) operands are quad_perm DPP reads.  Nothing crosses quads, and nothing goes through LDS on the way.  The quad's
// fourth lane shadows the third's inputs and stores nothing; lanes 0..2 store what they hold.
//
// The arithmetic is that of the wave-uniform form (-DSNK_SCALAR_DYNAMICS: every lane evaluates every component, lane 0
// stores; kept for tests/test_gpu_lane_dynamics.py and for A/B timing, in no shipped kernel), tree by tree as the compiler
// contracts that form:  a b + c d + e f = fma(e, f, fma(a, b, c d)),  a b - c d = fma(a, b, -(c d)),  p + a s = fma(a, s, p),
// spelled out here with contraction off.
// ----------------------------------------------------------------------------------
#ifndef SNK_SCALAR_DYNAMICS
// x of lane (c + 1) % 3 / (c + 2) % 3 of the quad, for c < 3
__device__ __forceinline__ float quad_yzx(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xC9, 0xf, 0xf, true));   // quad_perm [1,2,0,3]
}
__device__ __forceinline__ float quad_zxy(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xD2, 0xf, 0xf, true));   // quad_perm [2,0,1,3]
}
// component c of a x b, from a's two rotations (a body step crosses the parent's angular velocity three times)
__device__ __forceinline__ float lane_cross(float a_yzx, float a_zxy, float b) {
#pragma clang fp contract(off)
    return __builtin_fmaf(a_yzx, quad_zxy(b), -(a_zxy * quad_yzx(b)));
}
// component c of the velocity part of a body step: w = wp + ax qd, v = vp + wp x r, zeta = [wp x ax qd ; wp x (wp x r)]
struct LaneVel {
    float w, v, za, zl;
};
__device__ __forceinline__ LaneVel lane_vel_step(float wp, float vp, float ax, float rb, float qdb) {
#pragma clang fp contract(off)
    const float wy = quad_yzx(wp), wz = quad_zxy(wp);
    const float cr = lane_cross(wy, wz, rb);
    LaneVel o;
    o.w = __builtin_fmaf(ax, qdb, wp);
    o.v = vp + cr;
    o.za = lane_cross(wy, wz, ax) * qdb;
    o.zl = lane_cross(wy, wz, cr);
    return o;
}
#endif

template <class LT>
__device__ void fk_vel(LT& L, const DevModel& M, int lane) {
    constexpr int N = LT::kN;
    const float* bs = L.base();
    float Rp[9];
    quat_rot(bs[3], bs[4], bs[5], bs[6], Rp);
    f3 op = ld3(bs), wp = ld3(bs + 7), vp = ld3(bs + 10);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) L.R[0][i] = Rp[i];
        st3(L.o[0], op); st3(L.w[0], wp); st3(L.v[0], vp);
        st3(L.r[0], mk3(0, 0, 0)); st3(L.ax[0], mk3(0, 0, 0));
#pragma unroll
        for (int i = 0; i < 6; i++) L.zeta[0][i] = 0.f;
    }
    // sin/cos of all joint angles at once (lane = joint); the serial chain below picks them up
    // with v_readlane instead of evaluating sincosf sixteen times one after the other
    float snv = 0.f, csv = 1.f;
    if (lane < N) sincosf(L.q()[lane], &snv, &csv);
#ifndef SNK_SCALAR_DYNAMICS
    const int ln = launder_lane(lane);
    const int c = ln & 3, cc = c < 3 ? c : 2;
    float C0 = c == 0 ? Rp[0] : (c == 1 ? Rp[3] : Rp[6]);      // row c of the parent's R
    float C1 = c == 0 ? Rp[1] : (c == 1 ? Rp[4] : Rp[7]);
    float C2 = c == 0 ? Rp[2] : (c == 1 ? Rp[5] : Rp[8]);
    float opv = bs[cc], wpv = bs[7 + cc], vpv = bs[10 + cc];   // component c of the parent's origin and velocities
#pragma unroll 4
    for (int b = 1; b <= N; b++) {
#pragma clang fp contract(off)
        const float* Rf = M.Rfix[b];
        const float* pf = M.pfix[b];
        const float qdb = L.qd()[b - 1];
        const float sn = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(snv), b - 1));
        const float cs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(csv), b - 1));
        const float T0 = __builtin_fmaf(C2, Rf[6], __builtin_fmaf(C0, Rf[0], C1 * Rf[3]));   // row c of R_parent Rfix
        const float T1 = __builtin_fmaf(C2, Rf[7], __builtin_fmaf(C0, Rf[1], C1 * Rf[4]));   // (its column 1: the joint axis)
        const float T2 = __builtin_fmaf(C2, Rf[8], __builtin_fmaf(C0, Rf[2], C1 * Rf[5]));
        const float N0 = __builtin_fmaf(T0, cs, -(sn * T2));
        const float N2 = __builtin_fmaf(sn, T0, cs * T2);
        const float rb = __builtin_fmaf(C2, pf[2], __builtin_fmaf(C0, pf[0], C1 * pf[1]));
        const float o = opv + rb;
        const LaneVel k = lane_vel_step(wpv, vpv, T1, rb, qdb);
        if (ln < 3) {
            L.R[b][3 * c] = N0; L.R[b][3 * c + 1] = T1; L.R[b][3 * c + 2] = N2;
            L.o[b][c] = o; L.r[b][c] = rb; L.ax[b][c] = T1; L.w[b][c] = k.w; L.v[b][c] = k.v;
            L.zeta[b][c] = k.za; L.zeta[b][3 + c] = k.zl;
        }
        C0 = N0; C1 = T1; C2 = N2;
        opv = o; wpv = k.w; vpv = k.v;
    }
#else
#pragma unroll 4
    for (int b = 1; b <= N; b++) {
        const float* Rf = M.Rfix[b];
        float T[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                T[3 * i + j] = Rp[3 * i] * Rf[j] + Rp[3 * i + 1] * Rf[3 + j] + Rp[3 * i + 2] * Rf[6 + j];
        float qdb = L.qd()[b - 1];
        const float sn = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(snv), b - 1));
        const float cs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(csv), b - 1));
        float Rn[9];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            Rn[3 * i + 0] = cs * T[3 * i] - sn * T[3 * i + 2];
            Rn[3 * i + 1] = T[3 * i + 1];
            Rn[3 * i + 2] = sn * T[3 * i] + cs * T[3 * i + 2];
        }
        f3 rb = mulRv(Rp, ld3(M.pfix[b]));
        f3 o = op + rb;
        f3 ax = mk3(T[1], T[4], T[7]);
        f3 w = wp + ax * qdb;
        f3 v = vp + cross(wp, rb);
        f3 za = cross(wp, ax) * qdb;
        f3 zl = cross(wp, cross(wp, rb));
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 9; i++) L.R[b][i] = Rn[i];
            st3(L.o[b], o); st3(L.r[b], rb); st3(L.ax[b], ax); st3(L.w[b], w); st3(L.v[b], v);
            st3(&L.zeta[b][0], za); st3(&L.zeta[b][3], zl);
        }
#pragma unroll
        for (int i = 0; i < 9; i++) Rp[i] = Rn[i];
        op = o; wp = w; vp = v;
    }
#endif
    lds_sync();
}

// The velocities changed and the pose did not (the sensor passes, after v += a dt): w, v, zeta of every body again, from
// the axes and lever arms fk_vel left.  The same recurrence and the same lane map as fk_vel's velocity part.
template <class LT>
__device__ __forceinline__ void vel_refresh(LT& L, int lane) {
    constexpr int N = LT::kN;
#ifdef SNK_SCALAR_DYNAMICS
    f3 wp = ld3(L.base() + 7), vp = ld3(L.base() + 10);
    if (lane == 0) { st3(L.w[0], wp); st3(L.v[0], vp); }
    for (int b = 1; b <= N; b++) {
        f3 ax = ld3(L.ax[b]), rb = ld3(L.r[b]);
        float qdb = L.qd()[b - 1];
        f3 w = wp + ax * qdb, v = vp + cross(wp, rb);
        f3 za = cross(wp, ax) * qdb, zl = cross(wp, cross(wp, rb));
        if (lane == 0) { st3(L.w[b], w); st3(L.v[b], v); st3(&L.zeta[b][0], za); st3(&L.zeta[b][3], zl); }
        wp = w; vp = v;
    }
#else
    const int ln = launder_lane(lane);
    const int c = ln & 3, cc = c < 3 ? c : 2;
    float wpv = L.base()[7 + cc], vpv = L.base()[10 + cc];
    if (ln < 3) { L.w[0][c] = wpv; L.v[0][c] = vpv; }
    for (int b = 1; b <= N; b++) {
        const LaneVel k = lane_vel_step(wpv, vpv, L.ax[b][cc], L.r[b][cc], L.qd()[b - 1]);
        if (ln < 3) { L.w[b][c] = k.w; L.v[b][c] = k.v; L.zeta[b][c] = k.za; L.zeta[b][3 + c] = k.zl; }
        wpv = k.w; vpv = k.v;
    }
#endif
}

// checkSnakeHeight's mean z over {`base` link COM, OUTPUT_BODY origins} (snake.py:237-245)
template <class LT>
__device__ float mean_height(LT& L, const DevModel& M, int lane) {
    constexpr int N = LT::kN;
    float z = 0.f;
    if (lane == 0) z = L.o[0][2] + L.R[0][6] * M.hbase[0] + L.R[0][7] * M.hbase[1] + L.R[0][8] * M.hbase[2];
    else if (lane <= N) z = L.o[lane][2];
    return wave_sum<64>(z) * (1.0f / (N + 1));
}

// ----------------------------------------------------------------------------------
// S2: per-body bias forces (lane = body): p_b = [w x I w ; m w x (w x c)] - external
// ----------------------------------------------------------------------------------
template <class LT, bool FIRST>
__device__ void body_bias(LT& L, const DevModel& M, int lane) {
    constexpr int N = LT::kN;
    if (lane <= N) {
        const int b = lane;
        const float* R = L.R[b];
        f3 w = ld3(L.w[b]), v = ld3(L.v[b]);
        float m = M.mass[b];
        f3 cw = mulRv(R, ld3(M.com[b]));
        float Ibar[6];
        rotSym(R, M.Ib[b], Ibar);
        f3 pN = cross(w, mulSv(Ibar, w));
        f3 pF = cross(w, cross(w, cw)) * m;
        // [U] btMultiBody link damping, per original URDF link of the composite
        float Irw[6];
        rotSym(R, M.Irot[b], Irw);
        float nw = sqrtf(dot(w, w));
        pN = pN + mulSv(Irw, w) * (M.ang_damp + M.ang_damp * nw);
        const int ns = M.nsub[b];
        for (int s = 0; s < ns; s++) {
            f3 cs = mulRv(R, ld3(M.sub_c[b][s]));
            f3 vs = v + cross(w, cs);
            float nv = sqrtf(dot(vs, vs));
            f3 F = vs * (M.sub_m[b][s] * (M.lin_damp + M.lin_damp * nv));   // opposes motion
            pF = pF + F;
            pN = pN + cross(cs, F);
        }
        if (FIRST) {
            f3 G = mk3(0.f, 0.f, m * M.gz);
            pF = pF - G;
            pN = pN - cross(cw, G);
            st3(L.cw[b], cw);
            // articulated inertia initial value  [[Ibar, m[c]x], [-m[c]x, m 1]]
            float* IA = L.IA[b];
#pragma unroll
            for (int i = 0; i < 6; i++) IA[i] = Ibar[i];
            float hx = m * cw.x, hy = m * cw.y, hz = m * cw.z;
            IA[6] = 0.f; IA[7] = -hz; IA[8] = hy;
            IA[9] = hz;  IA[10] = 0.f; IA[11] = -hx;
            IA[12] = -hy; IA[13] = hx; IA[14] = 0.f;
            IA[15] = m; IA[16] = 0.f; IA[17] = 0.f; IA[18] = m; IA[19] = 0.f; IA[20] = m;
        } else {
            pN = pN - ld3(L.ext(b));
            pF = pF - ld3(L.ext(b) + 3);
        }
        st3(&L.p[b][0], pN);
        st3(&L.p[b][3], pF);
    }
}

// ----------------------------------------------------------------------------------
// S3: ABA sweeps, evaluated uniformly by the wave (serial recurrence over the chain).
// FACTOR: also builds the articulated inertias IA, U = IA S, D = S^T U and the base inverse.
// ----------------------------------------------------------------------------------
template <class LT, bool FACTOR>
__device__ void aba_main(LT& L, const DevModel& M, int lane SNK_PROF_F_PARAM) {
    constexpr int N = LT::kN;
    float cA[6], cB[9], cC[6];   // child contribution to the parent's articulated inertia
#pragma unroll
    for (int i = 0; i < 6; i++) { cA[i] = 0.f; cC[i] = 0.f; }
#pragma unroll
    for (int i = 0; i < 9; i++) cB[i] = 0.f;
    f3 cN = mk3(0, 0, 0), cF = mk3(0, 0, 0);
    for (int b = N; b >= 1; b--) {
        float A[6], B[9], C[6];
        float* IA = L.IA[b];
#pragma unroll
        for (int i = 0; i < 6; i++) { A[i] = IA[i]; C[i] = IA[15 + i]; }
#pragma unroll
        for (int i = 0; i < 9; i++) B[i] = IA[6 + i];
        if (FACTOR) {
#pragma unroll
            for (int i = 0; i < 6; i++) { A[i] += cA[i]; C[i] += cC[i]; }
#pragma unroll
            for (int i = 0; i < 9; i++) B[i] += cB[i];
        }
        f3 pN = ld3(&L.p[b][0]) + cN, pF = ld3(&L.p[b][3]) + cF;
        f3 ax = ld3(L.ax[b]);
        f3 Ua, Ub;
        float Dinv;
        if (FACTOR) {
            Ua = mulSv(A, ax);
            Ub = mk3(B[0] * ax.x + B[3] * ax.y + B[6] * ax.z, B[1] * ax.x + B[4] * ax.y + B[7] * ax.z,
                     B[2] * ax.x + B[5] * ax.y + B[8] * ax.z);
            Dinv = 1.0f / dot(ax, Ua);
        } else {
            Ua = ld3(L.Ua[b]); Ub = ld3(L.Ub[b]); Dinv = L.Dinv[b];
        }
        f3 za = ld3(&L.zeta[b][0]), zl = ld3(&L.zeta[b][3]);
        float u = L.tauj[b - 1] - dot(ax, pN);
        // IA zeta
        f3 tN = mulSv(A, za) + mk3(B[0] * zl.x + B[1] * zl.y + B[2] * zl.z, B[3] * zl.x + B[4] * zl.y + B[5] * zl.z,
                                   B[6] * zl.x + B[7] * zl.y + B[8] * zl.z);
        f3 tF = mk3(B[0] * za.x + B[3] * za.y + B[6] * za.z, B[1] * za.x + B[4] * za.y + B[7] * za.z,
                    B[2] * za.x + B[5] * za.y + B[8] * za.z) + mulSv(C, zl);
        float uz = dot(Ua, za) + dot(Ub, zl);
        float s = (u - uz) * Dinv;
        f3 paN = pN + tN + Ua * s, paF = pF + tF + Ub * s;
        f3 r = ld3(L.r[b]);
        cN = paN + cross(r, paF);
        cF = paF;
        if (lane == 0) {
            L.u[b] = u;
            if (FACTOR) {
#pragma unroll
                for (int i = 0; i < 6; i++) { IA[i] = A[i]; IA[15 + i] = C[i]; }
#pragma unroll
                for (int i = 0; i < 9; i++) IA[6 + i] = B[i];
                st3(L.Ua[b], Ua); st3(L.Ub[b], Ub); L.Dinv[b] = Dinv;
            }
        }
        if (FACTOR) {
            // Ia = IA - U U^T / D
            float ua[3] = {Ua.x, Ua.y, Ua.z}, ub[3] = {Ub.x, Ub.y, Ub.z};
            float Ap[6], Bp[9], Cp[6];
            Ap[0] = A[0] - ua[0] * ua[0] * Dinv; Ap[1] = A[1] - ua[0] * ua[1] * Dinv; Ap[2] = A[2] - ua[0] * ua[2] * Dinv;
            Ap[3] = A[3] - ua[1] * ua[1] * Dinv; Ap[4] = A[4] - ua[1] * ua[2] * Dinv; Ap[5] = A[5] - ua[2] * ua[2] * Dinv;
            Cp[0] = C[0] - ub[0] * ub[0] * Dinv; Cp[1] = C[1] - ub[0] * ub[1] * Dinv; Cp[2] = C[2] - ub[0] * ub[2] * Dinv;
            Cp[3] = C[3] - ub[1] * ub[1] * Dinv; Cp[4] = C[4] - ub[1] * ub[2] * Dinv; Cp[5] = C[5] - ub[2] * ub[2] * Dinv;
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) Bp[3 * i + j] = B[3 * i + j] - ua[i] * ub[j] * Dinv;
            // shift to the parent's origin: X = [[1,0],[-rx,1]];  IA_parent += X^T Ia X
            //   Bn = Bp + rx Cp ;  An = Ap - Bp rx + rx Bn^T ;  Cn = Cp
            f3 c0 = cross(r, mk3(Cp[0], Cp[1], Cp[2]));   // rx * column j of Cp (symmetric)
            f3 c1 = cross(r, mk3(Cp[1], Cp[3], Cp[4]));
            f3 c2 = cross(r, mk3(Cp[2], Cp[4], Cp[5]));
            float Bn[9] = {Bp[0] + c0.x, Bp[1] + c1.x, Bp[2] + c2.x, Bp[3] + c0.y, Bp[4] + c1.y, Bp[5] + c2.y,
                           Bp[6] + c0.z, Bp[7] + c1.z, Bp[8] + c2.z};
            // (-Bp rx) row i = r x row_i(Bp);  (rx Bn^T) column j = r x row_j(Bn)
            f3 e0 = cross(r, mk3(Bp[0], Bp[1], Bp[2])), e1 = cross(r, mk3(Bp[3], Bp[4], Bp[5])),
               e2 = cross(r, mk3(Bp[6], Bp[7], Bp[8]));
            f3 g0 = cross(r, mk3(Bn[0], Bn[1], Bn[2])), g1 = cross(r, mk3(Bn[3], Bn[4], Bn[5])),
               g2 = cross(r, mk3(Bn[6], Bn[7], Bn[8]));
            cA[0] = Ap[0] + e0.x + g0.x;
            cA[1] = Ap[1] + e0.y + g1.x;
            cA[2] = Ap[2] + e0.z + g2.x;
            cA[3] = Ap[3] + e1.y + g1.y;
            cA[4] = Ap[4] + e1.z + g2.y;
            cA[5] = Ap[5] + e2.z + g2.z;
#pragma unroll
            for (int i = 0; i < 9; i++) cB[i] = Bn[i];
#pragma unroll
            for (int i = 0; i < 6; i++) cC[i] = Cp[i];
        }
    }
    SNK_FSTAMP(2)
    // base: [alpha0; a0] = -IA0^-1 p0
    f3 pN = ld3(&L.p[0][0]) + cN, pF = ld3(&L.p[0][3]) + cF;
    float p0[6] = {pN.x, pN.y, pN.z, pF.x, pF.y, pF.z};
    if (FACTOR) {
        float* IA = L.IA[0];
        float A[6], B[9], C[6];
#pragma unroll
        for (int i = 0; i < 6; i++) { A[i] = IA[i] + cA[i]; C[i] = IA[15 + i] + cC[i]; }
#pragma unroll
        for (int i = 0; i < 9; i++) B[i] = IA[6 + i] + cB[i];
        float G[6][6];
        G[0][0] = A[0]; G[0][1] = A[1]; G[0][2] = A[2]; G[1][1] = A[3]; G[1][2] = A[4]; G[2][2] = A[5];
        G[1][0] = A[1]; G[2][0] = A[2]; G[2][1] = A[4];
        G[3][3] = C[0]; G[3][4] = C[1]; G[3][5] = C[2]; G[4][4] = C[3]; G[4][5] = C[4]; G[5][5] = C[5];
        G[4][3] = C[1]; G[5][3] = C[2]; G[5][4] = C[4];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) { G[i][3 + j] = B[3 * i + j]; G[3 + j][i] = B[3 * i + j]; }
        // Gauss-Jordan inverse of the SPD 6x6 (no pivoting)
        float V[6][6];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j < 6; j++) V[i][j] = (i == j) ? 1.f : 0.f;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            float piv = 1.0f / G[k][k];
#pragma unroll
            for (int j = 0; j < 6; j++) { G[k][j] *= piv; V[k][j] *= piv; }
#pragma unroll
            for (int i = 0; i < 6; i++) {
                if (i != k) {
                    float f = G[i][k];
#pragma unroll
                    for (int j = 0; j < 6; j++) { G[i][j] -= f * G[k][j]; V[i][j] -= f * V[k][j]; }
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j < 6; j++) L.Inv0[6 * i + j] = V[i][j];
        }
        float a0[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 6; j++) s -= V[i][j] * p0[j];
            a0[i] = s;
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 6; i++) L.acc0[i] = a0[i];
        }
    } else {
        float a0[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 6; j++) s -= L.Inv0[6 * i + j] * p0[j];
            a0[i] = s;
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 6; i++) L.acc0[i] = a0[i];
        }
    }
    lds_sync();
    SNK_FSTAMP(3)
    if (!FACTOR) return;   // the sensor pass only needs the base acceleration (acc0)
    // forward sweep: joint accelerations
    f3 al = ld3(&L.acc0[0]), a = ld3(&L.acc0[3]);
    for (int b = 1; b <= N; b++) {
        f3 r = ld3(L.r[b]);
        f3 ap = a + cross(al, r) + ld3(&L.zeta[b][3]);
        f3 alp = al + ld3(&L.zeta[b][0]);
        float qdd = (L.u[b] - (dot(ld3(L.Ua[b]), alp) + dot(ld3(L.Ub[b]), ap))) * L.Dinv[b];
        al = alp + ld3(L.ax[b]) * qdd;
        a = ap;
        if (lane == 0) L.qdd[b - 1] = qdd;
    }
    lds_sync();
    SNK_FSTAMP(4)
}

// True when the substep whose solve just produced `dv` (this lane's component of the velocity
// change) can be the LAST of its env-step, i.e. when obs[55] (the joint-0 force sensor, the second
// ABA pass) can be observed: the servo error after it is within the tolerance, or the counter
// reaches its cap, or the mean height can cross its threshold.  The first two are evaluated
// exactly as the loop does (with a 1e-3 safety factor on the tolerance).  For the third, the height
// is the MEAN z of N + 1 points: the base link's COM (o[0] + R0 hbase) and the joint origins o[1..N],
// with o[b] = o[b-1] + R[b-1] pfix[b].  One substep moves o[0] by dt v, turns the base by at most
// dt |omega| and joint j by dt |x_j|; a joint turns only the origins behind it, about an axis through
// o[j], and o[k] is at most (k - j) l from there (l = max_b |pfix[b]|: rigid distances).  So
//   |d mean z| <= dt ( |v|_1 + |omega|_1 (|hbase| + l N(N+1)/2) / (N+1)
//                      + sum_j |x_j| l (N-j)(N-j+1) / (2 (N+1)) )  + kReachSlack,
// each lane's weight in closed form from its index and the model's two scalars (no table: a vector
// load here would sit on every substep's chain).  DESIGN.md 4.
template <class LT>
__device__ __forceinline__ bool sensor_pass_needed(LT& L, const DevModel& M, int lane, float dv, const SensorHint& hint) {
    constexpr int N = LT::kN;
    constexpr int ND = N + 6;
    if (hint.always) return true;
    const float dt = M.dt;
    float e = 0.f, wgt = 0.f;
    if (lane < ND) {
        const float vold = lane < 6 ? L.base()[7 + lane] : L.qd()[lane - 6];
        const float x = fminf(fmaxf(vold + dv, -M.max_vel), M.max_vel);
        if (lane >= 6) e = L.targets[lane - 6] - (L.q()[lane - 6] + dt * x);
        const int m = N + 5 - lane;      // lanes >= 6: joint j = lane - 5 has m = N - j joint origins behind it
        const float arm = lane < 3 ? (M.reach_hb + M.reach_l * (0.5f * N * (N + 1))) * (1.0f / (N + 1))
                                   : (lane < 6 ? 1.0f : M.reach_l * ((float)(m * (m + 1)) * (0.5f / (N + 1))));
        wgt = fabsf(x) * arm;
    }
    const float se = wave_sum<64>(e * e);
    const float reach = dt * wave_sum<64>(wgt) + kReachSlack;
    const float tol = M.servo_tol * 1.001f;
    const bool sensor = !(se > tol * tol) || hint.counter_next > M.max_counter || !(hint.h_prev + reach < M.height_thr);
    return __builtin_amdgcn_readfirstlane(sensor ? 1 : 0) != 0;
}

// The pose of a free base `bs` ([pos3, quat4, omega3, vel3]: the snake's base, the free box) after dt at its new
// velocity: btMultiBody::stepPositionsMultiDof's exponential-map update with its ANGULAR_MOTION_THRESHOLD rule [U].
// Every lane computes it; lane 0 stores it behind a barrier (the other lanes' reads of bs), and the caller's barrier follows.
__device__ __forceinline__ void step_base_pose(float* bs, float dt, int lane) {
    f3 om = ld3(bs + 7), vl = ld3(bs + 10);
    float fA = sqrtf(dot(om, om));
    const float kThr = 0.78539816339744831f;   // 0.5 * pi/2  [U] ANGULAR_MOTION_THRESHOLD
    if (fA * dt > kThr) fA = kThr / dt;
    float sc;
    if (fA < 0.001f) sc = 0.5f * dt - (dt * dt * dt) * 0.020833333333f * fA * fA;
    else sc = sinf(0.5f * fA * dt) / fA;
    float dx = om.x * sc, dy = om.y * sc, dz = om.z * sc, dw = cosf(fA * dt * 0.5f);
    float qx = bs[3], qy = bs[4], qz = bs[5], qw = bs[6];
    float nw = dw * qw - dx * qx - dy * qy - dz * qz;
    float nx = dw * qx + dx * qw + dy * qz - dz * qy;
    float ny = dw * qy - dx * qz + dy * qw + dz * qx;
    float nz = dw * qz + dx * qy - dy * qx + dz * qw;
    float inv = 1.0f / sqrtf(nx * nx + ny * ny + nz * nz + nw * nw);
    lds_sync();
    if (lane == 0) {
        bs[0] += dt * vl.x; bs[1] += dt * vl.y; bs[2] += dt * vl.z;
        bs[3] = nx * inv; bs[4] = ny * inv; bs[5] = nz * inv; bs[6] = nw * inv;
    }
}

}  // namespace snk
