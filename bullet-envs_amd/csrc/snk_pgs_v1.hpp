// snk_pgs_v1.hpp -- the streamed-row solve: any chain length, every contact (ground manifolds, link-link, obstacle, the
// free box), rows streamed from a per-wave block of global memory.  The 32-link kernels run it for every substep, the
// 16-link register-resident kernels for the rare substeps whose contacts outgrow their slots (snk_device.hpp: substep()).
// In order: the two ground-contact finders, the row builder, the row steps, the solve, the substep.
#pragma once
#include "snk_contacts.hpp"
#include "snk_dynamics.hpp"
#include "snk_freebox.hpp"
#include "snk_lds.hpp"
#include "snk_model.hpp"
#include "snk_selfcol.hpp"
#include "snk_wave.hpp"

namespace snk {

// The same persistent-manifold contacts for the streamed-row solve (chains up to 32 links: one cylinder per lane):
// the manifolds in global memory, geometry records written at the COMPACT index (clist is the identity), at most NC
// ground contacts (the same rule for which points keep their rows, the same counters).  geo[19] of a record: the
// impulse its normal row starts from (warm starting).
template <class LT>
__device__ int find_contacts_manifold_v1(LT& L, const DevModel& M, int lane, float* __restrict__ rows, float* __restrict__ mf,
                                         unsigned long long* __restrict__ ovf) {
    constexpr int N = LT::kN;
    static_assert(2 * N <= 64, "one cylinder per lane");
    const ContactK K = contact_k(M);                 // (scalar loads; the vertex table into the lanes: every lane is active)
    const HullLanes H = hull_lanes(M, lane);
    int cnt = 0;
    MPt p[4];
    f3 wa[4];
    float Rw[9];
    const int c = lane < 2 * N ? lane : 0;
    const int b = (c + 1) >> 1;
    if (lane < 2 * N) {
        const float* Rb = L.R[b];
        cyl_world_rot(Rb, M.cyl_R[c], Rw);
        const f3 dl = mk3(-Rw[6], -Rw[7], -Rw[8]);
        const f3 centre = ld3(L.o[b]) + mulRv(Rb, ld3(M.cyl_c[c]));
        const int n0 = manifold_load_global(mf + (size_t)c * kMfFloats, p);
        cnt = manifold_core(M, K, H, n0, p, Rw, centre, dl, wa);
    }
    int total;
    (void)lane_prefix3(cnt, lane, total);
    const int room = LT::NC;
    const int mask = manifold_keep_mask(cnt, p, lane, total, room);
    const int kept = __popc(mask);
    int tk;
    const int base = manifold_base(M, K, 2 * N, kept, lane, tk);
    if (total > room && lane == 0) {
        atomicAdd(ovf, 1ull);
        atomicAdd(ovf + 1, (unsigned long long)(total - tk));
    }
    if (lane < 2 * N) {
        // the sensor pass finds a body's contacts through its cylinders: [first compact index, count] of cylinder `lane`
        // (the slot -> contact table of the stateless model is not used in this one; its array holds these pairs) and,
        // in the upper bits of the count word, which cached points they are (for the impulses' way back into the cache)
        L.cidx[2 * lane] = base;
        L.cidx[2 * lane + 1] = kept | (mask << 8);
        f3 dA, dB;
        friction_dirs(K, Rw, dA, dB);
        int idx = base;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool on = (mask >> j) & 1;
            if (!on) p[j].lam = 0.f;
            if (on) {
                float* geo = rows + LT::kGeoOff + (size_t)idx * LT::kGeo;
                st3(geo, wa[j]);
                geo[3] = p[j].d;
                st3(geo + 4, dA);
                st3(geo + 7, dB);
                st3(geo + 10, mk3(0.f, 0.f, 1.f));
                st3(geo + 13, mk3(0.f, 0.f, 0.f));
                geo[16] = (float)b; geo[17] = -1.0f; geo[18] = 1.0f;
                geo[19] = K.warm_start ? p[j].lam * K.warm_factor : 0.f;
                L.clist[idx] = idx;
                idx++;
            }
        }
        manifold_store_global(mf + (size_t)c * kMfFloats, cnt, p);
    }
    return tk;
}

// ----------------------------------------------------------------------------------
// ground contacts (lane = slot): cylinder c = slot/2 on body (c+1)/2, end cap = slot&1.
// Implicit cylinder + margin against the plane z = 0; kept when closer than the
// breaking threshold [U].  Friction directions (0,-1,0),(1,0,0) scaled anisotropically in
// the cylinder link's axes: d' = Rc diag(aniso) Rc^T d  (snake.py:104-106).
// ----------------------------------------------------------------------------------
template <class LT>
__device__ int find_contacts_v1(LT& L, const DevModel& M, int lane, float* __restrict__ rows, float* __restrict__ mf,
                                unsigned long long* __restrict__ ovf) {
    constexpr int N = LT::kN;
    const ContactK K = contact_k(M);
    if (K.contact_model == 1) return find_contacts_manifold_v1(L, M, lane, rows, mf, ovf);
    const HullLanes H = hull_lanes(M, lane);
    int total = 0;
    for (int base = 0; base < 4 * N; base += 64) {
        const int slot = base + lane;
        bool active = false;
        if (slot < 4 * N) {
            const int c = slot >> 1;
            const int b = (c + 1) >> 1;
            const float* Rb = L.R[b];
            const float* Rc = M.cyl_R[c];
            float Rw[9];      // = cyl_world_rot(Rb, Rc, Rw), written out: the call changes this kernel's instruction text
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++)
                    Rw[3 * i + j] = Rb[3 * i] * Rc[j] + Rb[3 * i + 1] * Rc[3 + j] + Rb[3 * i + 2] * Rc[6 + j];
            f3 dl = mk3(-Rw[6], -Rw[7], -Rw[8]);
            float lx, ly;
            rim_point(M, K, H, dl, lx, ly);
            float lz = (slot & 1) ? K.cyl_hl : -K.cyl_hl;
            f3 loc = mk3(lx + K.margin * dl.x, ly + K.margin * dl.y, lz + K.margin * dl.z);
            f3 P = ld3(L.o[b]) + mulRv(Rb, ld3(M.cyl_c[c])) + mulRv(Rw, loc);
            float dist = P.z;
            active = dist < K.break_thr;
            float* geo = rows + LT::kGeoOff + (size_t)slot * LT::kGeo;
            st3(geo, P);
            geo[3] = dist;
            f3 a = mk3(K.aniso[0], K.aniso[1], K.aniso[2]);
            f3 l1 = mulRtv(Rw, mk3(0.f, -1.f, 0.f));
            f3 l2 = mulRtv(Rw, mk3(1.f, 0.f, 0.f));
            st3(geo + 4, mulRv(Rw, mk3(l1.x * a.x, l1.y * a.y, l1.z * a.z)));
            st3(geo + 7, mulRv(Rw, mk3(l2.x * a.x, l2.y * a.y, l2.z * a.z)) * K.fricB);
            st3(geo + 10, mk3(0.f, 0.f, 1.f));
            st3(geo + 13, mk3(0.f, 0.f, 0.f));
            geo[16] = (float)b; geo[17] = -1.0f; geo[18] = 1.0f; geo[19] = 0.f;
        }
        unsigned long long bal = __ballot(active);
        if (slot < 4 * N) L.cidx[slot] = -1;
        if (active) {
            int idx = total + __popcll(bal & ((1ull << lane) - 1ull));
            L.clist[idx] = slot;
            L.cidx[slot] = idx;
        }
        total += __popcll(bal);
    }
    return total;
}

// ----------------------------------------------------------------------------------
// S5: constraint rows of the streamed-row solve, built lane = velocity component (round 1 built them lane = row:
// one pair of ABA delta sweeps per row, see the history of this file).
// A contact row's M^-1 J^T is linear in the 6-dimensional wrench its unit impulse puts on its body:
//     M^-1 J^T = Y_k (tau, f),   tau = (P - o_k) x dir,  f = dir,   Y_k = M^-1 Jbody_k^T   (38 x 6),
// and the Y_k follow from the columns of M^-1 by a recursion down the chain (a wrench on body k about o_k is the
// wrench (tau + r_k x f, f) on body k-1 about o_{k-1} plus the torque ax_k . tau on joint k):
//     Y_0 = M^-1[:, 0..5],   Y_k(tau, f) = Y_{k-1}(tau + r_k x f, f) + M^-1[:, 6+k-1] (ax_k . tau).
// So instead of one pair of ABA delta sweeps PER ROW (416 rows = 7 trips of 64 lanes through two serial 32-body
// recurrences, 19 % of a substep) there is ONE trip of 38 sweeps -- the columns of M^-1, which the motor rows need
// anyway -- nine FMAs per lane and body for the recursion, and per row: six FMAs for M^-1 J^T, J from the lane's own
// joint axis, two wave reductions (denominator, relative velocity), and ONE coalesced store of the finished record.
// (btMultiBodyConstraintSolver::setupMultiBodyContactConstraint / btMultiBody::calcAccelerationDeltasMultiDof [U]: the
//  rows are the same linear map of the same unit impulses; only the order of the floating-point sums differs.)
// ----------------------------------------------------------------------------------
template <class LT>
__device__ void build_rows_v1(LT& L, const DevModel& M, int lane, int nc, int& n_noncontact, float* __restrict__ rows) {
    constexpr int N = LT::kN;
    constexpr int ND = N + 6;
    constexpr int kMO = LT::kMO;
    float* const Mmx = rows + LT::kMmOff;           // M^-1, ND rows of kMO floats (columns >= ND stay zero)
    float mden = 0.f;                               // lane 6+j: M^-1[6+j][6+j], motor j's denominator
    // ---- (a) the columns of M^-1: lane = velocity component d, unit generalized force on it -- the ABA delta sweeps of
    // btMultiBody::calcAccelerationDeltasMultiDof [U].  Backward sweep here; the forward sweep runs body by body inside
    // the contact loop below (fwd), because the spatial acceleration (al, a) it gives body b IS what the contacts of
    // body b need:  Y_b[d] = response of component d to a unit wrench on body b = (M^-1 symmetric) response of body b's
    // twist to a unit force on component d.  Until the end of round 3 Y_b was rebuilt from the TRANSPOSED entries -- the
    // wrench moved rigidly to the base plus a torque on every joint up to b, the responses of all of those summed --
    // which is the same number with ~30 x the round-off (the terms are large and cancel; 32 links: one-substep velocity
    // errors p90 5.9e-2 against the float32 oracle's 2.0e-3, tools/acc_distribution.py 1024 32).
    const bool dofl = lane < ND;
    float* const Mrow = Mmx + (size_t)(dofl ? lane : 0) * kMO;
    const int kj = lane - 5;                        // the joint's body (lanes >= 6)
    f3 al = mk3(0, 0, 0), a = mk3(0, 0, 0);         // this lane's sweep: spatial acceleration of the body reached so far
    if (dofl) {
        const bool isbase = lane < 6;
        f3 pN = mk3(0, 0, 0), pF = mk3(0, 0, 0);
#pragma unroll 4
        for (int b = N; b >= 1; b--) {
            f3 ax = ld3(L.ax[b]);
            float u = -dot(ax, pN);
            if (!isbase && b == kj) u += 1.0f;
            Mrow[6 + b - 1] = u;                    // (parked in the row the forward sweep overwrites with qdd_b)
            float t = u * L.Dinv[b];
            f3 paN = pN + ld3(L.Ua[b]) * t, paF = pF + ld3(L.Ub[b]) * t;
            pN = paN + cross(ld3(L.r[b]), paF);
            pF = paF;
        }
        float p0[6] = {pN.x, pN.y, pN.z, pF.x, pF.y, pF.z}, a0[6];
#pragma unroll
        for (int i = 0; i < 6; i++) if (lane == i) p0[i] = -1.0f;      // unit force on the base: bias -e_i
#pragma unroll
        for (int i = 0; i < 6; i++) {
            float sacc = 0.f;
#pragma unroll
            for (int j = 0; j < 6; j++) sacc -= L.Inv0[6 * i + j] * p0[j];
            a0[i] = sacc;
            Mrow[i] = sacc;
        }
        al = mk3(a0[0], a0[1], a0[2]);
        a = mk3(a0[3], a0[4], a0[5]);
    }
    // the free box (obstacle 2): a second multibody, block-diagonal in M^-1 -- rows ND .. ND + 5: the world inverse
    // inertia for its angular components, 1 / m for its linear ones
    const bool fbox = N <= 16 && M.obstacle == 2;         // (built for the 16-link chain only: snk_create)
    const bool boxlane = fbox && lane >= ND && lane < ND + 6;
    if (boxlane) {
        const int i = lane - ND;
        float* Mrow = Mmx + (size_t)lane * kMO;
        const float* W = L.bIw;
        const f3 r0 = i == 0 ? mk3(W[0], W[1], W[2]) : (i == 1 ? mk3(W[1], W[3], W[4]) : mk3(W[2], W[4], W[5]));
        Mrow[ND + 0] = i < 3 ? r0.x : 0.f; Mrow[ND + 1] = i < 3 ? r0.y : 0.f; Mrow[ND + 2] = i < 3 ? r0.z : 0.f;
        Mrow[ND + 3] = i == 3 ? M.obs_minv : 0.f; Mrow[ND + 4] = i == 4 ? M.obs_minv : 0.f; Mrow[ND + 5] = i == 5 ? M.obs_minv : 0.f;
    }
    // ---- (b) lane = velocity component d: what J[d] is made of, and the current velocity
    const int d = lane;
    const int jb = d >= 6 ? d - 5 : 0;              // the body this component's joint belongs to (0: the base)
    f3 Aj = mk3(0, 0, 0), Oj = mk3(0, 0, 0), Bj = mk3(0, 0, 0);
    float vd = 0.f;
    if (d < 3) { Aj = mk3(d == 0 ? 1.f : 0.f, d == 1 ? 1.f : 0.f, d == 2 ? 1.f : 0.f); Oj = ld3(L.o[0]); vd = L.base()[7 + d]; }
    else if (d < 6) { Bj = mk3(d == 3 ? 1.f : 0.f, d == 4 ? 1.f : 0.f, d == 5 ? 1.f : 0.f); vd = L.base()[7 + d]; }
    else if (d < ND) { Aj = ld3(L.ax[jb]); Oj = ld3(L.o[jb]); vd = L.qd()[d - 6]; }
    else if (boxlane) {
        const int i = d - ND;
        if (i < 3) { Aj = mk3(i == 0 ? 1.f : 0.f, i == 1 ? 1.f : 0.f, i == 2 ? 1.f : 0.f); Oj = ld3(L.box); }
        else Bj = mk3(i == 3 ? 1.f : 0.f, i == 4 ? 1.f : 0.f, i == 5 ? 1.f : 0.f);
        vd = L.box[7 + i];
    }
    // does this lane's component move a point of body k?  (the snake's: the joints up to k; the box's six: the box)
    auto moves = [&](int k) { return boxlane ? k == LT::kBoxBody : (k <= N && jb <= k); };
    const bool colv = d < kMO;                      // lanes that own a column of the records
    // Y of the body the sweep has reached: (Yt, Yf) = (al, a); zero on the lanes without a velocity component
    f3 Yt = al, Yf = a;                             // Y_0
    // link-link / obstacle contacts: any body, so every Y_k is kept.  And so it is when the ground contacts do not come in
    // the order of their bodies (snk_params::contact_order): the forward sweep below cannot follow them then, they take their
    // Y from the block like the two-body contacts (a switch of the error bar, not the default: the extra 32 KB of stores and
    // loads per substep are its price)
    const bool sorted = M.contact_order == 0;
    const bool two_body = nc > L.nplane || !sorted;
    float* const Yb = rows + LT::kYOff;
    auto storeY = [&](int k) {
        if (two_body && colv) {
            float* y = Yb + (size_t)k * 6 * kMO + d;
            y[0] = Yt.x; y[kMO] = Yt.y; y[2 * kMO] = Yt.z; y[3 * kMO] = Yf.x; y[4 * kMO] = Yf.y; y[5 * kMO] = Yf.z;
        }
    };
    storeY(0);
    int kcur = 0;
    auto advance = [&]() {                          // the forward sweep's step to body kcur + 1: Y_kcur -> Y_kcur+1
        kcur++;
        if (dofl) {
            const int b = kcur;
            Yf = Yf + cross(Yt, ld3(L.r[b]));
            const float u = Mrow[6 + b - 1];
            const float qdd = (u - (dot(ld3(L.Ua[b]), Yt) + dot(ld3(L.Ub[b]), Yf))) * L.Dinv[b];
            Yt = Yt + ld3(L.ax[b]) * qdd;
            Mrow[6 + b - 1] = qdd;
            if (b == kj) mden = qdd;
        }
        storeY(kcur);
    };
    // one contact: three rows from its geometry record and the Y of its body (and of the other body of a pair)
    struct Geo { float4 g[5]; };
    auto load_geo = [&](int ci) {
        const int slot = __builtin_amdgcn_readfirstlane(ci < L.nplane ? L.clist[ci] : LT::NC + (ci - L.nplane));
        const float4* g = reinterpret_cast<const float4*>(rows + LT::kGeoOff + (size_t)slot * LT::kGeo);
        Geo G;
#pragma unroll
        for (int i = 0; i < 5; i++) G.g[i] = g[i];
        return G;
    };
    const float spec0 = d == LT::kSpec ? 1.0f : 0.f, spec1 = d == LT::kSpec + 1 ? 1.0f : 0.f;    // the records' scalar columns
    // The solve resolves the normals two at a time (row_step_normal2): the second row's dot is taken from the same
    // delta-v as the first's and corrected by  c dI_first,  c = (J_2 / den_2) . (M^-1 J_1^T)  -- exactly the sequential
    // sweep.  c of an odd contact with its predecessor rides in the spare float of its impulse entry.
    float prevMn = 0.f;                             // M^-1 J^T of the previous contact's normal row (this lane's column)
    auto assemble = [&](int ci, const Geo& G, const f3 YtA, const f3 YfA, const f3 YtB, const f3 YfB, int kA, int kB,
                        auto two_c) {
        constexpr bool TWO = decltype(two_c)::value;       // a pair of bodies (link-link) or one body against the world
        const f3 P = mk3(G.g[0].x, G.g[0].y, G.g[0].z);
        const float dist = G.g[0].w;
        const f3 dA = mk3(G.g[1].x, G.g[1].y, G.g[1].z), dB = mk3(G.g[1].w, G.g[2].x, G.g[2].y);
        const f3 dn = mk3(G.g[2].z, G.g[2].w, G.g[3].x), PB = mk3(G.g[3].y, G.g[3].z, G.g[3].w);
        const float fsc = G.g[4].z, lam0 = G.g[4].w;     // lam0: where the normal row starts (warm starting; else 0)
        // J[d] = A_d . ((P - O_d) x dir) + B_d . dir = dir . (A_d x (P - O_d) + B_d), and likewise
        // M^-1 J^T [d] = Yt . ((P - o_k) x dir) + Yf . dir = dir . (Yt x (P - o_k) + Yf): one vector per contact and
        // lane for each, a dot product per row
        // (a body's reference point: its joint origin; the free box's: its centre)
        auto org = [&](int k) { return (TWO && k == LT::kBoxBody) ? ld3(L.box) : ld3(L.o[k <= N ? k : 0]); };
        f3 Cj = cross(Aj, P - Oj) + Bj;
        if (!moves(kA)) Cj = mk3(0, 0, 0);
        f3 Dj = cross(YtA, P - org(kA)) + YfA;
        if (TWO && kB >= 0) {                                           // wave-uniform: minus the same for the other body
            f3 Cb = cross(Aj, PB - Oj) + Bj;
            if (!moves(kB)) Cb = mk3(0, 0, 0);
            Cj = Cj - Cb;
            Dj = Dj - (cross(YtB, PB - org(kB)) + YfB);
        }
        float Jr[3], Mr[3], red[7];
#pragma unroll
        for (int kind = 0; kind < 3; kind++) {
            const f3 dir = kind == 0 ? dn : (kind == 1 ? dA : dB);
            const float j = dot(dir, Cj);
            float m = dot(dir, Dj);
            if (TWO && kind != 0) m *= fsc;                             // (ground contacts: scale 1)
            Jr[kind] = j; Mr[kind] = m;
            red[kind] = j * m; red[3 + kind] = j * vd;
        }
        red[6] = Jr[0] * prevMn;                                        // the normals' coupling with the previous contact
        // seven sums over the wave, their DPP steps interleaved (each instruction is the others' wait state)
        asm volatile(
            "s_nop 1\n\t"      // the operands may have been written by the instructions just before (VALU write -> DPP read)
            SNK_RED64x7_STEP("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1")
            SNK_RED64x7_STEP("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1")
            SNK_RED64x7_STEP("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1")
            SNK_RED64x7_STEP("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1")
            SNK_RED64x7_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf")
            SNK_RED64x7_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
            : [a] "+v"(red[0]), [b] "+v"(red[1]), [c] "+v"(red[2]), [d] "+v"(red[3]), [e] "+v"(red[4]), [f] "+v"(red[5]),
              [g] "+v"(red[6]));
        float cpl = 0.f;
        float Jo[3], Mo[3];
#pragma unroll
        for (int kind = 0; kind < 3; kind++) {
            const float dn_ = lane_bcast(red[kind], 63), rv_ = lane_bcast(red[3 + kind], 63);
            float rc = __builtin_amdgcn_rcpf(dn_);
            rc = rc * (2.0f - dn_ * rc);                                // one Newton step: within an ulp of 1 / den
            const float dinv = dn_ > 1.1920929e-7f ? rc : 0.f;
            float target = -rv_;
            if (kind == 0) {
                const float pen = dist + M.slop;
                float erp = M.contact_erp;
                if constexpr (LT::kERP) erp = pen > M.erp_split ? M.erp_shallow : M.erp_deep;     // contact_erp_rule
                target += pen > 0.f ? -pen * M.inv_dt : -pen * erp * M.inv_dt;
            }
            // the record's columns (Lds<N, false>): J / den with -rhs and 0 in the pad columns; M^-1 J^T with 0 and den
            // (J and M^-1 J^T are zero in the pad columns as they come)
            Jo[kind] = dinv * (Jr[kind] - spec0 * target);
            Mo[kind] = Mr[kind] + spec1 * dn_;
            if (kind == 0) cpl = (ci & 1) ? dinv * lane_bcast(red[6], 63) : 0.f;
        }
        prevMn = Mo[0];
        if (colv) {
            // contacts 2p and 2p + 1 share a 640-byte record [J0 M0 J1 M1] per column: the solve resolves them in one
            // step (row_step_normal2) and fetches them with one 16-byte load per lane
            *reinterpret_cast<float2*>(rows + (size_t)(ci >> 1) * 2 * LT::kRS + 4 * d + 2 * (ci & 1)) = make_float2(Jo[0], Mo[0]);
            *reinterpret_cast<float4*>(rows + (size_t)(LT::kFric + 2 * ci) * LT::kRS + 4 * d) = make_float4(Jo[1], Jo[2], Mo[1], Mo[2]);
        }
        if (lane == 0) *reinterpret_cast<float4*>(L.acc[ci]) = make_float4(lam0, 0.f, 0.f, cpl);
    };
    // ---- (c) ground contacts, in the order of their bodies: Y stays in registers
    const int nplane = L.nplane;
    {
        const f3 z3 = mk3(0, 0, 0);
        auto one = [&](int ci, const Geo& G) {
            const int kA = __builtin_amdgcn_readfirstlane((int)G.g[4].x);
            while (kcur < kA) advance();
            assemble(ci, G, Yt, Yf, z3, z3, kA, -1, std::false_type{});
        };
        if (nplane > 0 && sorted) {
            Geo ga = load_geo(0);                                       // two records in flight, no copies between them
            for (int ci = 0; ci < nplane; ci += 2) {
                const Geo gb = load_geo(ci + 1 < nplane ? ci + 1 : ci);
                one(ci, ga);
                if (ci + 1 < nplane) {
                    ga = load_geo(ci + 2 < nplane ? ci + 2 : ci + 1);
                    one(ci + 1, gb);
                }
            }
        }
    }
    while (kcur < N) advance();                     // (the rest of M^-1's rows: the motors need every joint's)
    // ---- (d) link-link and obstacle contacts: any two bodies, their Y from the block the sweep left behind
    if (two_body) {
        if (fbox && colv) {
            // Y of the box: a unit wrench (tau, f) about its centre moves its own six components only --
            // angular component i: row i of the world inverse inertia . tau, linear component i: f_i / m
            float* y = Yb + (size_t)LT::kBoxBody * 6 * kMO + d;
            const int i = d - ND;
            const float* W = L.bIw;
            f3 yt = mk3(0, 0, 0), yf = mk3(0, 0, 0);
            if (boxlane && i < 3) yt = i == 0 ? mk3(W[0], W[1], W[2]) : (i == 1 ? mk3(W[1], W[3], W[4]) : mk3(W[2], W[4], W[5]));
            if (boxlane && i >= 3) yf = mk3(i == 3 ? M.obs_minv : 0.f, i == 4 ? M.obs_minv : 0.f, i == 5 ? M.obs_minv : 0.f);
            y[0] = yt.x; y[kMO] = yt.y; y[2 * kMO] = yt.z; y[3 * kMO] = yf.x; y[4 * kMO] = yf.y; y[5 * kMO] = yf.z;
        }
        own_stores_visible();
        lds_sync();
        for (int ci = sorted ? nplane : 0; ci < nc; ci++) {
            const Geo G = load_geo(ci);
            const int kA = __builtin_amdgcn_readfirstlane((int)G.g[4].x), kB = __builtin_amdgcn_readfirstlane((int)G.g[4].y);
            auto ldY = [&](int k, f3& yt, f3& yf) {
                const float* y = Yb + (size_t)k * 6 * kMO + (colv ? d : 0);
                yt = colv ? mk3(y[0], y[kMO], y[2 * kMO]) : mk3(0, 0, 0);
                yf = colv ? mk3(y[3 * kMO], y[4 * kMO], y[5 * kMO]) : mk3(0, 0, 0);
            };
            f3 ytA, yfA, ytB = mk3(0, 0, 0), yfB = mk3(0, 0, 0);
            ldY(kA, ytA, yfA);
            if (kB >= 0) ldY(kB, ytB, yfB);
            assemble(ci, G, ytA, yfA, ytB, yfB, kA, kB, std::true_type{});
        }
    }
    lds_sync();
    // ---- (e) non-contact rows: violated joint limits first, then the n motors
    // (btMultiBodyJointLimitConstraint, btMultiBodyJointMotor [U])
    const float mden_j = __shfl(mden, lane + 6);    // motor / joint `lane`: its denominator sits in lane 6 + lane
    int nlim = 0;
    {
        bool viol = false;
        float sgn = 0.f, pen = 0.f;
        if (lane < N) {
            float qj = L.q()[lane];
            float plo = qj - M.jlo, phi = M.jhi - qj;
            if (plo <= 0.f) { viol = true; sgn = 1.f; pen = plo; }
            else if (phi <= 0.f) { viol = true; sgn = -1.f; pen = phi; }
        }
        unsigned long long bal = __ballot(viol);
        nlim = __popcll(bal);
        if (viol) {
            // noncontact_order 1: the violated limits in the quickSort's joint order, not by joint index
            unsigned long long before = (1ull << lane) - 1ull;
            if constexpr (LT::kNCO != 0) before = NoncontactOrder<N>::tab.below[lane];
            int idx = __popcll(bal & before);
            float den = mden_j;
            float dinv = den > 1.1920929e-7f ? 1.0f / den : 0.f;
            float rel = sgn * L.qd()[lane];
            L.nc_joint[idx] = lane; L.nc_sign[idx] = sgn;
            L.nc_rhs[idx] = (-rel + (-pen) * M.limit_erp * M.inv_dt) * dinv;
            L.nc_dinv[idx] = dinv; L.nc_den[idx] = den;
            L.nc_lo[idx] = 0.f; L.nc_hi[idx] = M.limit_max; L.nc_app[idx] = 0.f;
        }
        if (lane < N) {
            int idx = nlim + lane;
            float den = mden_j;
            float dinv = den > 1.1920929e-7f ? 1.0f / den : 0.f;
            float cur = L.qd()[lane];
            float want = M.kp * (L.targets[lane] - L.q()[lane]) * M.inv_dt + cur + M.kd * (0.f - cur);
            L.nc_joint[idx] = lane; L.nc_sign[idx] = 1.f;
            L.nc_rhs[idx] = (want - cur) * dinv;
            L.nc_dinv[idx] = dinv; L.nc_den[idx] = den;
            L.nc_lo[idx] = -M.max_motor_imp; L.nc_hi[idx] = M.max_motor_imp; L.nc_app[idx] = 0.f;
        }
    }
    n_noncontact = nlim + N;
    lds_sync();
}

// ----------------------------------------------------------------------------------
// S6: projected Gauss-Seidel for chains too long for the register-resident solve (the 32-link
// config: 38 velocity components, up to 384 contact rows kept in LDS), lane = velocity component
// (btMultiBodyConstraintSolver::solveSingleIteration / resolveSingleConstraintRowGeneric /
//  resolveConeFrictionConstraintRows [U]).  Returns delta-v of this lane.
//
// Same lessons as the 16-link solve (snk_pgs_v2.hpp): the row steps are hand-written with the
// fewest VALU instructions (one multiply + a 6-step DPP reduction per dot, the clamp on
// wave-uniform values, J rows pre-divided by their denominator), a row's operands are read
// from LDS one row ahead of their use, and the motor rows -- unit Jacobians -- need no
// reduction at all.
// ----------------------------------------------------------------------------------
// Row steps of the streamed-row solve.  jv: the row's J half (J / den, -rhs in lane kSpec, where delta-v holds 1), mv: its
// M^-1 J^T half (den in lane kSpec + 1), both one value per lane; the dot  s = (J.dv)/den - rhs  comes out of one
// multiply and a 6-step DPP reduction, the clamp runs on wave-uniform values, and |M^-1 J^T dI| carries the row's
// residual |dI den| in lane kSpec + 1 (collected per lane in lsq, read once per iteration).
// a contact-normal row: a' = max(a - s, 0); dv += M^-1 J^T (a' - a).  Returns a'.  14 VALU.
template <int SUM_LANE>
__device__ __forceinline__ float row_step_normal(float jv, float mv, float acc, float& dv, float& lsq) {
    float t, x, P, s;
    asm volatile(
        "v_mul_f32 %[t], %[jv], %[dv]\n\t"
        "s_nop 1\n\t"
        SNK_RED64("%[t]")
        "s_nop 0\n\t"
        "v_readlane_b32 %[s], %[t], %[SL]\n\t"
        "s_nop 1\n\t"
        "v_subrev_f32 %[x], %[s], %[acc]\n\t"
        "v_max_f32 %[x], 0, %[x]\n\t"
        "v_sub_f32 %[t], %[x], %[acc]\n\t"
        "v_mul_f32 %[P], %[t], %[mv]\n\t"
        "v_add_f32 %[dv], %[dv], %[P]\n\t"
        "v_max_f32_e64 %[lsq], %[lsq], |%[P]|\n\t"
        : [t] "=&v"(t), [x] "=&v"(x), [P] "=&v"(P), [s] "=&s"(s), [dv] "+v"(dv), [lsq] "+v"(lsq)
        : [jv] "v"(jv), [mv] "v"(mv), [acc] "v"(acc), [SL] "n"(SUM_LANE));
    return x;
}

// Two consecutive contact normals: both dots from the same delta-v, their reductions interleaved (one s_nop per stage
// instead of two per stage and row), the second row's sum corrected by  c dI_first  (c: see build_rows_v1).  28 VALU,
// 36 issue slots for the two rows against 2 x 30.
template <int SUM_LANE>
__device__ __forceinline__ void row_step_normal2(float jA, float mA, float jB, float mB, float& accA, float& accB, float c,
                                                 float& dv, float& lsq) {
    float tA, tB, xA, xB, dA, sA, sB;
    asm volatile(
        "v_mul_f32 %[tA], %[jA], %[dv]\n\t"
        "v_mul_f32 %[tB], %[jB], %[dv]\n\t"
        "s_nop 0\n\t"
        SNK_RED64x2_STEP("%[tA]", "%[tB]", "quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1")
        SNK_RED64x2_STEP("%[tA]", "%[tB]", "quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1")
        SNK_RED64x2_STEP("%[tA]", "%[tB]", "row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        SNK_RED64x2_STEP("%[tA]", "%[tB]", "row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        SNK_RED64x2_STEP("%[tA]", "%[tB]", "row_bcast:15 row_mask:0xa bank_mask:0xf")
        "v_add_f32_dpp %[tA], %[tA], %[tA] row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "v_add_f32_dpp %[tB], %[tB], %[tB] row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 0\n\t"
        "v_readlane_b32 %[sA], %[tA], %[SL]\n\t"
        "v_readlane_b32 %[sB], %[tB], %[SL]\n\t"
        "s_nop 0\n\t"
        "v_subrev_f32 %[xA], %[sA], %[accA]\n\t"
        "v_subrev_f32 %[xB], %[sB], %[accB]\n\t"
        "v_max_f32 %[xA], 0, %[xA]\n\t"
        "v_sub_f32 %[dA], %[xA], %[accA]\n\t"
        "v_fma_f32 %[xB], -%[c], %[dA], %[xB]\n\t"
        "v_max_f32 %[xB], 0, %[xB]\n\t"
        "v_mul_f32 %[tA], %[dA], %[mA]\n\t"
        "v_sub_f32 %[dA], %[xB], %[accB]\n\t"
        "v_add_f32 %[dv], %[dv], %[tA]\n\t"
        "v_mul_f32 %[tB], %[dA], %[mB]\n\t"
        "v_add_f32 %[dv], %[dv], %[tB]\n\t"
        "v_max3_f32 %[lsq], %[lsq], |%[tA]|, |%[tB]|\n\t"
        : [tA] "=&v"(tA), [tB] "=&v"(tB), [xA] "=&v"(xA), [xB] "=&v"(xB), [dA] "=&v"(dA), [sA] "=&s"(sA), [sB] "=&s"(sB),
          [dv] "+v"(dv), [lsq] "+v"(lsq)
        : [jA] "v"(jA), [mA] "v"(mA), [jB] "v"(jB), [mB] "v"(mB), [accA] "v"(accA), [accB] "v"(accB), [c] "v"(c),
          [SL] "n"(SUM_LANE));
    accA = xA;
    accB = xB;
}

// Bullet's cone-friction pair of one contact: both dots from the same delta-v, the new pair (a - s) projected
// radially onto the disc of radius lim.  31 VALU.
template <int SUM_LANE>
__device__ __forceinline__ void row_step_cone(float jA, float mA, float jB, float mB, float& accA, float& accB, float lim,
                                              float EPS, float& dv, float& lsq) {
    float tA, tB, xA, xB, r2, P, sA, sB;
    asm volatile(
        "v_mul_f32 %[tA], %[jA], %[dv]\n\t"
        "v_mul_f32 %[tB], %[jB], %[dv]\n\t"
        "s_nop 0\n\t"
        SNK_RED64x2_STEP("%[tA]", "%[tB]", "quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1")
        SNK_RED64x2_STEP("%[tA]", "%[tB]", "quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1")
        SNK_RED64x2_STEP("%[tA]", "%[tB]", "row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        SNK_RED64x2_STEP("%[tA]", "%[tB]", "row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        SNK_RED64x2_STEP("%[tA]", "%[tB]", "row_bcast:15 row_mask:0xa bank_mask:0xf")
        "v_add_f32_dpp %[tA], %[tA], %[tA] row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "v_add_f32_dpp %[tB], %[tB], %[tB] row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 0\n\t"
        "v_readlane_b32 %[sA], %[tA], %[SL]\n\t"
        "v_readlane_b32 %[sB], %[tB], %[SL]\n\t"
        "s_nop 0\n\t"
        "v_subrev_f32 %[xA], %[sA], %[accA]\n\t"
        "v_subrev_f32 %[xB], %[sB], %[accB]\n\t"
        "v_fma_f32 %[r2], %[xA], %[xA], %[EPS]\n\t"
        "v_fma_f32 %[r2], %[xB], %[xB], %[r2]\n\t"
        "v_rsq_f32 %[r2], %[r2]\n\t"
        "s_nop 0\n\t"
        "v_mul_f32_e64 %[r2], %[lim], %[r2] clamp\n\t"
        "v_mul_f32 %[xA], %[xA], %[r2]\n\t"
        "v_mul_f32 %[xB], %[xB], %[r2]\n\t"
        "v_sub_f32 %[tA], %[xA], %[accA]\n\t"
        "v_sub_f32 %[tB], %[xB], %[accB]\n\t"
        "v_mul_f32 %[P], %[tA], %[mA]\n\t"
        "v_mul_f32 %[r2], %[tB], %[mB]\n\t"
        "v_add_f32 %[dv], %[dv], %[P]\n\t"
        "v_add_f32 %[dv], %[dv], %[r2]\n\t"
        "v_max3_f32 %[lsq], %[lsq], |%[P]|, |%[r2]|\n\t"        // the two rows' residuals separately (their sum could cancel)
        : [tA] "=&v"(tA), [tB] "=&v"(tB), [xA] "=&v"(xA), [xB] "=&v"(xB), [r2] "=&v"(r2), [P] "=&v"(P), [sA] "=&s"(sA),
          [sB] "=&s"(sB), [dv] "+v"(dv), [lsq] "+v"(lsq)
        : [jA] "v"(jA), [mA] "v"(mA), [jB] "v"(jB), [mB] "v"(mB), [accA] "v"(accA), [accB] "v"(accB), [lim] "v"(lim),
          [EPS] "v"(EPS), [SL] "n"(SUM_LANE));
    accA = xA;
    accB = xB;
}

// INPLACE: the copy that runs inside the register-resident kernels for their rare substeps (substep()): it keeps rounds
// 2-3's 32 / 32 / 16 registers' split.  With the standalone kernels' 40 / 16 / 16 (round 4: +2 % for 32 links, +7 % for the
// 16-link streamed-row kernels) the register-resident kernel around it came out 3.6 % slower -- 352 k against 365 k
// env-steps/s with 19 such substeps in 80 000 -- for the registers live across the call.
template <class LT, bool INPLACE = false>
__device__ float pgs_v1(LT& L, const DevModel& M, int lane, int nc, int nn, float mu, int& iters,
                        float* __restrict__ rows) {
    constexpr int N = LT::kN;
    constexpr int ND = N + 6;
    static_assert(ND <= 64, "this solve is laid out for one row per 64-lane register");
    constexpr int kSpec = LT::kSpec;
    const bool act = lane < ND + ((N <= 16 && M.obstacle == 2) ? 6 : 0);      // (the free box's six components sit behind the snake's)
    const int nlim = nn - N;                       // violated joint limits come first in the non-contact list
    // model fields used inside the loops, read once (the model lives in global memory)
    // (v_readfirstlane: the loads go through vector memory, the values must be scalar for the
    //  branches on them to be scalar branches instead of exec-mask regions)
    const int n_iter = __builtin_amdgcn_readfirstlane(M.n_iter);
    const bool cone = __builtin_amdgcn_readfirstlane(M.cone) != 0;
    const float mi = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(M.max_motor_imp)));
    const float thr2 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(M.resid_thr)));
    // motor rows: lane 6+j holds motor j's target velocity change and 1/den
    const bool mot = lane >= 6 && act;
    const int jm = mot ? lane - 6 : 0;
    const float DINVV = mot ? L.nc_dinv[nlim + jm] : 0.f;
    const float DENV = mot ? L.nc_den[nlim + jm] : 0.f;
    const float TARGV = (mot && DINVV > 0.f) ? L.nc_rhs[nlim + jm] * DENV : 0.f;
    float ACCV = 0.f;                               // accumulated motor impulses, motor j in lane 6+j
    const float EPS = 1e-30f;
    // Row operands come from global memory through register rings (kRingN normals / kRingF friction pairs in flight), a
    // contact's record requested a ring's depth before it is used (the next trip's loads are
    // issued one by one as this trip's slots are consumed).  Lane d < ND reads column d of a row, lanes kSpec and
    // kSpec + 1 the row's scalars (160 contiguous bytes per half row: coalesced); the other lanes sit the solve out.
    // The rows and impulses of the contacts between nc and the end of the last group are zeroed: resolving them
    // changes nothing (dI = 0 exactly).
    constexpr int kRN = INPLACE ? SNK_IP_RINGN : LT::kRingN;      // normals in flight
    // contacts are resolved in groups of 8 behind one scalar branch: the rows between nc and the next multiple of 8
    // are zeroed (inert), a ring trip ends at that multiple instead of running its full depth (round 1 padded
    // to a whole trip: 144 contacts -- 128 on the ground + 16 link-link -- cost 160)
    const int nc_pad = __builtin_amdgcn_readfirstlane((nc + 7) / 8 * 8);
    {
        // (normals in pairs: an odd count leaves the last contact's partner inside its record -- its two floats per column --,
        //  then whole records)
        const int nce = (nc + 1) & ~1;
        if ((nc & 1) && lane < LT::kMO)
            *reinterpret_cast<float2*>(rows + (size_t)(nc >> 1) * 2 * LT::kRS + 4 * lane + 2) = make_float2(0.f, 0.f);
        float* z = rows + (size_t)nce * LT::kRS;
        float* zf = rows + (size_t)(LT::kFric + 2 * nc) * LT::kRS;
        const int nz = (nc_pad - nc) * LT::kRS;
        for (int i = lane; i < (nc_pad - nce) * LT::kRS; i += 64) z[i] = 0.f;
        for (int i = lane; i < 2 * nz; i += 64) zf[i] = 0.f;
        for (int i = lane; i < 4 * (nc_pad - nc); i += 64) L.acc[nc][i] = 0.f;
    }
    own_stores_visible();     // the rows were written lane = row, they are read lane = column
    lds_sync();
    constexpr int kRS = LT::kRS;
    // Addressing: a record's address is a wave-uniform base (scalar arithmetic) plus the lane's column, 4 * lane bytes,
    // so a load is  global_load_dword v, v_column, s[base:base+1] offset:imm  with no vector arithmetic at all
    // (round-2 measurement: per-lane 64-bit pointers cost 4 VALU per friction step, a tenth of its issue slots).
    // For that every lane that takes part must stride alike, so the solve runs with lanes 0 .. kMO - 1 only (the
    // 38 velocity components and the two scalar columns); the sum of a row's products lands in lane kMO - 1.
    constexpr unsigned kRecB = kRS * 4, kHalfB = LT::kMO * 4;        // bytes per record, offset of its M^-1 J^T half
    constexpr unsigned kFricB = (unsigned)LT::kFric * kRecB;          // the first friction pair
    // (buffer loads: resource descriptor and record offset in SGPRs, the column in a VGPR, the half in the immediate)
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(rows, 0, (int)(LT::kRowFloats * sizeof(float)), 0x00020000);
    const int vcol = 4 * lane;
    auto ldJ = [&](unsigned rec_bytes) {             // a column of a plain (motor) row
        return __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, vcol, (int)rec_bytes, 0));
    };
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    auto ldN = [&](unsigned rec_bytes, float& j, float& m) {       // {J, M^-1 J^T} of a normal's record
        // (rec_bytes = contact x kRecB as before; inside its pair's record the contact's two floats sit at 16 d + 8 (ci & 1))
        const unsigned odd = (rec_bytes / kRecB) & 1u;
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, 4 * vcol, (int)(rec_bytes - odd * kRecB + odd * 8u), SNK_V1_LDAUX);
        j = __uint_as_float(v.x); m = __uint_as_float(v.y);
    };
    auto ldN2 = [&](unsigned rec_bytes, float& j0, float& m0, float& j1, float& m1) {      // rec_bytes: of the EVEN contact
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, 4 * vcol, (int)rec_bytes, SNK_V1_LDAUX);
        j0 = __uint_as_float(v.x); m0 = __uint_as_float(v.y); j1 = __uint_as_float(v.z); m1 = __uint_as_float(v.w);
    };
    auto ldF = [&](unsigned rec_bytes, float& ja, float& jb, float& ma, float& mb) {    // a friction pair's record
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, 4 * vcol, (int)rec_bytes, SNK_V1_LDAUX);
        ja = __uint_as_float(v.x); jb = __uint_as_float(v.y); ma = __uint_as_float(v.z); mb = __uint_as_float(v.w);
    };
    // (Round 5 tried the solve with all 64 lanes enabled -- neutral -- and further resident rows in the upper 24 lanes of
    //  the resident registers, fetched with ds_bpermute: bit-identical and 2 % SLOWER, a stashed row costs more issue
    //  slots than the stream it saves; and one reduction for a step's two dots (v_permlane32_swap, 17 % fewer VALU
    //  instructions): no change -- the solve runs at the latency of each wave's chain of dependent row steps, not at a
    //  byte or an issue rate; profiles/r05_c32_stash_experiment.txt)
    float dv = lane == kSpec ? 1.0f : 0.f;        // lane kSpec: the constant that multiplies the rows' -rhs column
    int it = 0;
    if (lane < LT::kMO) {
    // the motors' M^-1 columns stay in registers for the whole solve (they are read 50 x n times)
    float RMm[N];
#pragma unroll
    for (int j = 0; j < N; j++) RMm[j] = ldJ((unsigned)(LT::kMmOff * 4) + (unsigned)(6 + j) * kHalfB);   // columns >= ND: zero
    // ... and so do the normal rows of the first kResN contacts: the registers the rings leave free hold an eighth of
    // the stream (the kernel is bound by that stream)
    constexpr int kResN = INPLACE ? SNK_IP_RESN : LT::kResN;
    // What the build-time knobs (SNK_V1_* / SNK_IP_*) must satisfy for the loops below to stay inside the records: rows
    // come in pairs (ldN2), the early exits and the ring's refill address are evaluated at every eighth row only, the
    // first ring trip starts behind the resident rows.  A sweep value such as 36 or 44 would compile and read beyond
    // nc_pad.
    static_assert(kResN % 8 == 0 && kResN > 0, "resident normal rows: a multiple of 8 (groups of 8 behind one scalar branch)");
    static_assert(kRN % 8 == 0 && kRN > 0, "normal rows in flight: a multiple of 8 (refill address taken at k % 8 == 0)");
    static_assert(kResN + kRN <= LT::NCT, "resident + in-flight normal rows exceed the contact slots of this layout");
    static_assert((INPLACE ? SNK_IP_RINGF : LT::kRingF) % 8 == 0, "friction pairs in flight: a multiple of 8");
    float RNJ[kResN], RNM[kResN];
#pragma unroll
    for (int k = 0; k < kResN; k += 2) ldN2((unsigned)k * kRecB, RNJ[k], RNM[k], RNJ[k + 1], RNM[k + 1]);
    if (__builtin_amdgcn_readfirstlane(M.warm_start)) {
        // warm starting: the normal rows start at the impulses build_rows_v1 took from the contact cache, delta-v at the
        // sum of M^-1 J^T of those (the scalar columns' part of that sum is dropped again: lane kSpec stays 1, and
        // lane kSpec + 1 is only ever read through lsq)
        for (int ci = 0; ci < nc; ci++) {
            const float a = L.acc[ci][0];
            if (__builtin_amdgcn_readfirstlane(a != 0.f ? 1 : 0)) {
                float jj, mm;
                ldN((unsigned)ci * kRecB, jj, mm);
                dv += act ? a * mm : 0.f;
            }
        }
    }
    for (; it < n_iter; it++) {
        float lsq = 0.f;       // per lane max |M^-1 J^T dI| of the contact rows: lane kSpec + 1 holds max |dI * den|
        float lsq_nc = 0.f;    // max |dI * den| of the limit and motor rows
        auto limit_rows = [&](bool fwd) {
            for (int jj = 0; jj < nlim; jj++) {
                const int idx = fwd ? jj : nlim - 1 - jj;
                const int j = __builtin_amdgcn_readfirstlane(L.nc_joint[idx]);
                const float sg = L.nc_sign[idx];
                float un = sg * lane_bcast(dv, 6 + j);
                float a0 = L.nc_app[idx];
                float dI = L.nc_rhs[idx] - un * L.nc_dinv[idx];
                float sum = fminf(fmaxf(a0 + dI, L.nc_lo[idx]), L.nc_hi[idx]);
                dI = sum - a0;
                L.nc_app[idx] = sum;   // uniform value, every lane stores it: no barrier needed
                const float mv = ldJ((unsigned)(LT::kMmOff * 4) + (unsigned)(6 + j) * kHalfB);      // a violated limit is rare
                dv += sg * mv * dI;
                lsq_nc = fmaxf(lsq_nc, fabsf(dI * L.nc_den[idx]));
            }
        };
        auto motor_rows = [&](auto fwd_c) {
            constexpr bool fwd = decltype(fwd_c)::value;
            float Uv = 0.f;                                              // lane 6+j: the dI motor j got in this sweep
#pragma unroll
            for (int jj = 0; jj < N; jj++) {
                // (noncontact_order 1: the quickSort's joint order, a compile-time table -- RMm[] stays in registers)
                const int j = LT::kNCO ? NoncontactOrder<N>::motor(fwd, jj) : (fwd ? jj : N - 1 - jj);
                float u = (TARGV - dv) * DINVV;                          // every motor's candidate dI, lane-local (DINVV = 0 beyond the joints)
                if (mi < 1e30f) u = fminf(fmaxf(ACCV + u, -mi), mi) - ACCV;   // (a lane's ACCV only matters at its own step)
                const float sdI = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u), 6 + j));
                Uv = (lane == 6 + j) ? u : Uv;
                dv += sdI * RMm[j];                                      // zero beyond the velocity components
            }
            ACCV += Uv;
            lsq_nc = fmaxf(lsq_nc, cols_max<LT::kMO - 1>(fabsf(Uv * DENV)));
        };
        if constexpr (LT::kNCO == 0) {      // list = [limits..., motors...], odd iterations forwards
            if (it & 1) { limit_rows(true); motor_rows(std::true_type{}); }
            else { motor_rows(std::false_type{}); limit_rows(false); }
        } else {                            // noncontact_order 1: list = [motors..., limits...]
            if (it & 1) { motor_rows(std::true_type{}); limit_rows(true); }
            else { limit_rows(false); motor_rows(std::false_type{}); }
        }
        if (nc > 0) {
            // normals: slot k of the ring holds contact (trip base + k).  A slot is refilled with
            // the contact kRingN further on as soon as it has been consumed -- if there is one: round 1 refilled
            // unconditionally, and with the usual 128 contacts the last trip of each phase fetched 32 (16) contacts'
            // worth of rows nobody used, 14 % of the stream this kernel is bound by; the contact's
            // accumulated impulse comes from LDS one step ahead.
            float jr[kRN], mr[kRN];
#pragma unroll
            for (int k = 0; k < kRN; k += 2) ldN2((unsigned)(kResN + k) * kRecB, jr[k], mr[k], jr[k + 1], mr[k + 1]);
            // two contacts per step (row_step_normal2): {impulse of the even one, impulse and coupling of the odd one} come
            // from LDS one step ahead
            float a0n = L.acc[0][0];
            float2 a1n = make_float2(L.acc[1][0], L.acc[1][3]);
#pragma unroll
            for (int k = 0; k < kResN; k += 2) {                                // the resident rows
                if ((k & 7) == 0 && k > 0 && k >= nc_pad) break;                // wave-uniform
                float a0 = a0n, a1 = a1n.x;
                const float c1 = a1n.y;
                a0n = L.acc[k + 2][0];
                a1n = make_float2(L.acc[k + 3][0], L.acc[k + 3][3]);
                row_step_normal2<LT::kMO - 1>(RNJ[k], RNM[k], RNJ[k + 1], RNM[k + 1], a0, a1, c1, dv, lsq);
                L.acc[k][0] = a0;
                L.acc[k + 1][0] = a1;
            }
            unsigned rb = 0;           // record the current group of eight refills counts from (wave-uniform)
            for (int base = kResN; base < nc_pad; base += kRN) {
#pragma unroll
                for (int k = 0; k < kRN; k += 2) {
                    if ((k & 7) == 0 && k > 0 && base + k >= nc_pad) break;      // wave-uniform
                    float a0 = a0n, a1 = a1n.x;
                    const float c1 = a1n.y;
                    a0n = L.acc[base + k + 2][0];
                    a1n = make_float2(L.acc[base + k + 3][0], L.acc[base + k + 3][3]);
                    row_step_normal2<LT::kMO - 1>(jr[k], mr[k], jr[k + 1], mr[k + 1], a0, a1, c1, dv, lsq);
                    L.acc[base + k][0] = a0;
                    L.acc[base + k + 1][0] = a1;
                    // the refill: the contacts kRN further on if there are any, else this trip's once more
                    // (a cache hit instead of a fetch of rows nobody uses; no branch, the load is issued either way).
                    // Issued after the step: the register pairs are free then and take the new records as they are
                    if ((k & 7) == 0) rb = (unsigned)((base + kRN + k < nc_pad) ? base + kRN : base) * kRecB;
                    ldN2(rb + (unsigned)k * kRecB, jr[k], mr[k], jr[k + 1], mr[k + 1]);
                }
            }
            if (cone) {
                // friction pairs: half a ring of contacts in flight (four vectors per contact).
                // A pair whose contact carries no normal impulse and no friction impulse yet resolves to exactly
                // nothing (the disc it is projected onto has radius 0: a' = a = 0, dI = 0) -- typically one contact in
                // six.  Its step is skipped and its record is not fetched: `live`, one bit per contact, is fixed for the
                // whole phase (the normal impulses are this iteration's final ones, a pair's own impulses only change
                // at its own step), built with four ballots and kept in SGPRs, so a step's test is scalar.
                constexpr int kC = INPLACE ? SNK_IP_RINGF : LT::kRingF;
                // (the solve runs on lanes 0 .. kMO - 1: one ballot covers kMO contacts; kP ballots, kW 64-bit words)
                constexpr int kP = (LT::NCT + LT::kMO - 1) / LT::kMO, kW = (kP * LT::kMO + 63) / 64;
                unsigned long long mw[kW + 1];
#pragma unroll
                for (int w = 0; w <= kW; w++) mw[w] = 0ull;
#pragma unroll
                for (int p = 0; p < kP; p++) {
                    const int c = LT::kMO * p + lane;
                    bool lv = false;
                    if (c < nc_pad) {
                        const float4 a = *reinterpret_cast<const float4*>(L.acc[c]);
                        lv = (mu * a.x > 0.f) || (a.y != 0.f) || (a.z != 0.f);     // (-0 counts as zero: a pair projected onto radius 0)
                    }
                    const unsigned long long b = __ballot(lv);
                    const int w = (LT::kMO * p) / 64, sh = (LT::kMO * p) % 64;       // compile-time after unrolling
                    mw[w] |= b << sh;
                    if (sh + LT::kMO > 64) mw[w + 1] |= b >> (64 - sh);
                }
                // (the register is shifted down by kC contacts per trip)
                constexpr unsigned kZeroB = (unsigned)(LT::kRows - 3) * kRecB;   // 960 bytes of zeros: the refill of a skipped pair
                float jA[kC], jB[kC], mA[kC], mB[kC];
                {
                    const unsigned long long l0 = mw[0];
#pragma unroll
                    for (int k = 0; k < kC; k++)
                        ldF((l0 >> k) & 1ull ? kFricB + (unsigned)k * 2u * kRecB : kZeroB, jA[k], jB[k], mA[k], mB[k]);
                }
                float4 fn = *reinterpret_cast<const float4*>(L.acc[0]);
                for (int base = 0; base < nc_pad; base += kC) {
                    unsigned long long lv = mw[0];                  // bits 0 .. kC - 1: this trip, kC .. 2 kC - 1: the next
                    static_assert(2 * kC <= 64, "two trips' bits in one word");
#pragma unroll
                    for (int w = 0; w < kW; w++) mw[w] = (mw[w] >> kC) | (mw[w + 1] << (64 - kC));      // (mw[kW] stays 0)
#pragma unroll
                    for (int k = 0; k < kC; k++) {
                        if ((k & 7) == 0 && k > 0 && base + k >= nc_pad) break;  // wave-uniform
                        const float4 c = fn;
                        fn = *reinterpret_cast<const float4*>(L.acc[base + k + 1]);
                        asm volatile("" : "+s"(lv));         // the test stays a scalar bit test here (hoisted, sixteen lane masks spill SGPRs)
                        if ((lv >> k) & 1ull) {
                            float aA = c.y, aB = c.z;
                            row_step_cone<LT::kMO - 1>(jA[k], mA[k], jB[k], mB[k], aA, aB, mu * c.x, EPS, dv, lsq);
                            *reinterpret_cast<float2*>(&L.acc[base + k][1]) = make_float2(aA, aB);
                        }
                        // the refill, issued after the step (the four registers are free then): the pair kC further on
                        ldF((lv >> (kC + k)) & 1ull ? kFricB + (unsigned)(base + kC + k) * 2u * kRecB : kZeroB, jA[k], jB[k], mA[k], mB[k]);
                    }
                }
            } else {
                // pyramid friction (not Bullet's default here): box-clamped rows, one after the other
                for (int ci = 0; ci < nc; ci++) {
                    const unsigned o = kFricB + (unsigned)ci * 2u * kRecB;
                    float* ac = L.acc[ci];
                    const float lim = mu * ac[0];
                    if (!(lim > 0.f)) continue;
                    const float accA = ac[1], accB = ac[2];
                    float fjA, fjB, fmA, fmB;
                    ldF(o, fjA, fjB, fmA, fmB);
                    const float sA = fminf(fmaxf(accA - cols_sum<LT::kMO - 1>(fjA * dv), -lim), lim);
                    const float PA = fmA * (sA - accA);
                    dv += PA;
                    const float sB = fminf(fmaxf(accB - cols_sum<LT::kMO - 1>(fjB * dv), -lim), lim);
                    const float PB = fmB * (sB - accB);
                    dv += PB;
                    ac[1] = sA; ac[2] = sB;
                    lsq = fmaxf(lsq, fmaxf(fabsf(PA), fabsf(PB)));
                }
            }
        }
        const float res = fmaxf(lane_bcast(lsq, kSpec + 1), lsq_nc);
        if (res * res <= thr2 || it >= n_iter - 1) { it++; break; }
    }
    }
    it = __builtin_amdgcn_readfirstlane(it);
    if (lane >= 6 && lane < 6 + N) L.nc_app[nlim + lane - 6] = ACCV;
    lds_sync();
    iters = it;
    return act ? dv : 0.f;
}

// ----------------------------------------------------------------------------------
// one physics substep
// ----------------------------------------------------------------------------------
template <class LT, bool INPLACE = false>
__device__ __forceinline__ void substep_v1(LT& L, const DevModel& M, int lane, float mu, int& iters, int& ncontacts, float* __restrict__ rows,
                           const SensorHint& hint, float* __restrict__ mf, unsigned long long* __restrict__ ovf) {
    constexpr int N = LT::kN;
    constexpr int ND = N + 6;
    const float dt = M.dt;
#ifdef SNK_PROFILE
    unsigned long long prof_t[10];
#endif
    SNK_STAMP(0)
    const bool fbox = N <= 16 && M.obstacle == 2;         // the obstacle as a free body (16-link chain only): six more velocity components (lanes ND ..)
    if (fbox) box_frame_v1(L, M, lane);
    // (1) contacts of the current pose, (2) bias forces with gravity, joint damping torque
    int nc = find_contacts_v1(L, M, lane, rows, mf, ovf);
    SNK_STAMP(1)
    if (lane == 0) L.nplane = nc;
    const int nplane = nc;
    if (M.self_collision || M.obstacle)
        nc += find_self_contacts_v1(L, M, lane, mu, rows, ovf);   // link-link and obstacle contacts follow the ground's
    if (fbox) nc += find_box_ground_v1(L, M, lane, mu, nc - nplane, rows, ovf);     // ... and the box's own with the ground
    ncontacts = nc;
    own_stores_visible(); // contact geometry: written lane = slot, read lane = row
    lds_sync();
    SNK_STAMP(2)
    if (lane < N) {
        float qd = L.qd()[lane];
        L.qd_old[lane] = qd;
        L.tauj[lane] = -M.joint_damp * qd;   // PyBullet adds URDF joint damping as a torque [U]
    }
    body_bias<LT, true>(L, M, lane);
    lds_sync();
    aba_main<LT, true>(L, M, lane);
    SNK_STAMP(3)
    // joint-0 force sensor, first pass [U]: -zb . [m_r (a - g) + m_r v (k + k|v|)]
    f3 zb = mulRv(L.R[0], ld3(M.zbase));
    f3 v_old = ld3(L.base() + 10);
    float nv0 = sqrtf(dot(v_old, v_old));
    f3 a1 = ld3(&L.acc0[3]);
    float fz = -dot(zb, (a1 - mk3(0.f, 0.f, M.gz)) * M.m_root + v_old * (M.m_root * (M.lin_damp + M.lin_damp * nv0)));
    // reaction through the first motor joint (Bullet joint 3, snake_gait_test.py:33-40): what body 0 does not use up
    // of the forces on it, Newton on body 0 alone:  F = -(m_0 (a_0 + alpha_0 x c_0) + own force bias), z of body 1
    auto joint1_fz = [&]() {
        const f3 al0 = ld3(&L.acc0[0]), a0l = ld3(&L.acc0[3]);
        const f3 F = -((a0l + cross(al0, ld3(L.cw[0]))) * M.mass[0] + ld3(&L.p[0][3]));
        return F.x * L.R[1][2] + F.y * L.R[1][5] + F.z * L.R[1][8];
    };
    float fz3 = joint1_fz();
    // (3) v += a dt (clamped)
    if (lane < 6) {
        float x = L.base()[7 + lane] + L.acc0[lane] * dt;
        L.base()[7 + lane] = fminf(fmaxf(x, -M.max_vel), M.max_vel);
    } else if (lane < ND) {
        float x = L.qd()[lane - 6] + L.qdd[lane - 6] * dt;
        L.qd()[lane - 6] = fminf(fmaxf(x, -M.max_vel), M.max_vel);
    } else if (fbox && lane < ND + 6) {
        // the free box, a btMultiBody without links [U]: gravity, the base's damping m v (k + k|v|), I w (k + k|w|),
        // the gyroscopic term; lanes ND .. ND + 2 its angular, ND + 3 .. ND + 5 its linear components
        const f3 om = ld3(L.box + 7), vl = ld3(L.box + 10);
        const float nw = sqrtf(dot(om, om)), nv = sqrtf(dot(vl, vl));
        // world inertia times omega: R diag(1 / iinv) R^T omega
        const f3 wl = mulRtv(L.bR, om);
        const f3 Iw = mulRv(L.bR, mk3(M.obs_iinv[0] > 0.f ? wl.x / M.obs_iinv[0] : 0.f, M.obs_iinv[1] > 0.f ? wl.y / M.obs_iinv[1] : 0.f,
                                      M.obs_iinv[2] > 0.f ? wl.z / M.obs_iinv[2] : 0.f));
        const f3 tq = -cross(om, Iw) - Iw * (M.ang_damp + M.ang_damp * nw);
        const f3 al = mulSv(L.bIw, tq);
        const f3 a = mk3(0.f, 0.f, M.gz) - vl * (M.lin_damp + M.lin_damp * nv);
        const int i = lane - ND;
        const float acc = i == 0 ? al.x : (i == 1 ? al.y : (i == 2 ? al.z : (i == 3 ? a.x : (i == 4 ? a.y : a.z))));
        const float x = L.box[7 + i] + acc * dt;
        L.box[7 + i] = fminf(fmaxf(x, -M.max_vel), M.max_vel);
    }
    lds_sync();
    // (4) rows, (5) PGS
    int nn = 0;
    SNK_STAMP(4)
    build_rows_v1(L, M, lane, nc, nn, rows);
    SNK_STAMP(5)
    // the solve runs at a higher wave priority than everything around it (snk_pgs_v2.hpp: substep_v2)
    __builtin_amdgcn_s_setprio(3);
    float dv = pgs_v1<LT, INPLACE>(L, M, lane, nc, nn, mu, iters, rows);
    __builtin_amdgcn_s_setprio(0);
    SNK_STAMP(6)
    if (M.contact_model == 1 && lane < 2 * N) {
        // the normal impulses go back into the contact cache (btManifoldPoint::m_appliedImpulse [U]), write-through
        // like the cache itself
        int idx = L.cidx[2 * lane];
        const int mask = L.cidx[2 * lane + 1] >> 8;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if ((mask >> j) & 1) {
                const float a = L.acc[idx++][0];
                asm volatile("global_store_dword %0, %1, off sc1" : : "v"(mf + (size_t)lane * kMfFloats + 9 + 6 * j), "v"(a) : "memory");
            }
    }
    // only when this substep can be the last of its env-step (sensor_pass_needed)
    const bool sensor = sensor_pass_needed(L, M, lane, dv, hint);
    // delta-v crosses the sensor pass in LDS, not in a register (the pass is full of lane-dependent regions,
    // and a copy or a reload the allocator places inside one moves the active lanes only -- snk_pgs_v2.hpp has the
    // story; the register-resident substep's pass is a function of its own, here the value is parked): the solve is
    // over, so the non-contact rows' rhs column is free (the pass reads their joint, sign and impulse only)
    constexpr int kPark = 2 * N;        // = NL of this image (LdsCommon<N, 2 N>): 64 lanes for 32 links, 32 for 16
    static_assert(kPark >= N + 6 + (N <= 16 ? 6 : 0), "every lane with a velocity component has a slot");
    if (lane < kPark) L.nc_rhs[lane] = dv;
    if (sensor) {
        // (6) constraint pass for the joint-0 sensor [U]: ABA at the velocities after (3) with the
        // constraint forces as the only link forces, joint torques still applied
        if (lane <= N) {
            const int b = lane;
            f3 eN = mk3(0, 0, 0), eF = mk3(0, 0, 0);
            // contact slots of body b: cylinders 2b-1, 2b (body 0: cylinder 0) = slots 4b-2 .. 4b+1, in
            // contact order
            if (M.contact_model == 1) {
                // Bullet's manifolds: up to four points per cylinder, geometry stored by compact index;
                // cidx[2c], cidx[2c + 1] = first index and count of cylinder c (find_contacts_manifold_v1)
    #pragma unroll
                for (int cc = 0; cc < 2; cc++) {
                    const int c = 2 * b - 1 + cc;
                    if (c < 0 || c >= 2 * N) continue;
                    const int first = L.cidx[2 * c], cnt = L.cidx[2 * c + 1] & 0xff;
                    for (int j = 0; j < cnt; j++) {
                        const int ci = first + j;
                        const float* geo = rows + LT::kGeoOff + (size_t)ci * LT::kGeo;
                        f3 F = (mk3(0.f, 0.f, 1.f) * L.acc[ci][0] + ld3(geo + 4) * L.acc[ci][1] +
                                ld3(geo + 7) * L.acc[ci][2]) * M.inv_dt;
                        eF = eF + F;
                        eN = eN + cross(ld3(geo) - ld3(L.o[b]), F);
                    }
                }
            } else {
    #pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int slot = 4 * b - 2 + j;
                    const int ci = (slot >= 0 && slot < 4 * N) ? L.cidx[slot] : -1;
                    if (ci >= 0) {
                        const float* geo = rows + LT::kGeoOff + (size_t)slot * LT::kGeo;
                        f3 F = (mk3(0.f, 0.f, 1.f) * L.acc[ci][0] + ld3(geo + 4) * L.acc[ci][1] +
                                ld3(geo + 7) * L.acc[ci][2]) * M.inv_dt;
                        eF = eF + F;
                        eN = eN + cross(ld3(geo) - ld3(L.o[b]), F);
                    }
                }
            }
            // link-link contacts: equal and opposite forces on the two bodies (friction back from the solve's units)
            for (int ci = nplane; ci < nc; ci++) {
                const float* geo = rows + LT::kGeoOff + (size_t)(LT::NC + ci - nplane) * LT::kGeo;
                const int kA = (int)geo[16], kB2 = (int)geo[17];
                if (kA != b && kB2 != b) continue;
                const float fs = geo[18];
                const f3 F = (ld3(geo + 10) * L.acc[ci][0] + ld3(geo + 4) * (L.acc[ci][1] * fs) +
                              ld3(geo + 7) * (L.acc[ci][2] * fs)) * M.inv_dt;
                if (kA == b) { eF = eF + F; eN = eN + cross(ld3(geo) - ld3(L.o[b]), F); }
                if (kB2 == b) { eF = eF - F; eN = eN - cross(ld3(geo + 13) - ld3(L.o[b]), F); }
            }
            st3(L.ext(b), eN);
            st3(L.ext(b) + 3, eF);
        }
        if (lane < N) L.tauj[lane] = -M.joint_damp * L.qd_old[lane];
        lds_sync();
        if (lane == 0) {
            // in the list's order, as the oracle sums (the storage keeps the limits in front of the motors either way;
            // noncontact_order 1 sweeps -- and sums -- the motors first)
            const int nlim_ = nn - N;
            for (int i = 0; i < nn; i++) {
                const int r = LT::kNCO ? (i < N ? nlim_ + i : i - N) : i;
                L.tauj[L.nc_joint[r]] += L.nc_sign[r] * L.nc_app[r] * M.inv_dt;
            }
        }
        lds_sync();
        // velocities changed in (3): refresh w, v, zeta of every body (pose unchanged)
        vel_refresh(L, lane);
        lds_sync();
        body_bias<LT, false>(L, M, lane);
        lds_sync();
        aba_main<LT, false>(L, M, lane);
        {
            f3 v1 = ld3(L.base() + 10);
            float nv1 = sqrtf(dot(v1, v1));
            f3 a2 = ld3(&L.acc0[3]);
            fz += -dot(zb, a2 * M.m_root + v1 * (M.m_root * (M.lin_damp + M.lin_damp * nv1)));
            fz3 += joint1_fz();
        }
    }
    SNK_STAMP(7)
    if (fbox && lane == 0) {
        // the box's contacts with the ground are the last L.bmn-or-fewer of the list: their normal impulses go back
        // into its manifold (btManifoldPoint::m_appliedImpulse [U])
        int nb = 0;
        for (int ci = nplane; ci < nc; ci++) {
            const float* geo = rows + LT::kGeoOff + (size_t)(LT::NC + ci - nplane) * LT::kGeo;
            if ((int)geo[16] == LT::kBoxBody) { if (nb < 4) L.bman[6 * nb + 5] = L.acc[ci][0]; nb++; }
        }
    }
    // (7) apply the solver's delta-v (clamped), motor torques, integrate positions
    dv = lane < kPark ? L.nc_rhs[lane] : 0.f;
    if (lane < 6) {
        float x = L.base()[7 + lane] + dv;
        L.base()[7 + lane] = fminf(fmaxf(x, -M.max_vel), M.max_vel);
    } else if (lane < ND) {
        float x = L.qd()[lane - 6] + dv;
        x = fminf(fmaxf(x, -M.max_vel), M.max_vel);
        L.qd()[lane - 6] = x;
        L.q()[lane - 6] += dt * x;
    } else if (fbox && lane < ND + 6) {
        const float x = L.box[7 + lane - ND] + dv;
        L.box[7 + lane - ND] = fminf(fmaxf(x, -M.max_vel), M.max_vel);
    }
    if (lane < N) {
        // motor rows sit after the limit rows in the non-contact list's storage (whatever order the sweep takes them in)
        L.taum()[lane] = L.nc_app[nn - N + lane] * M.inv_dt;
    }
    lds_sync();
    step_base_pose(L.base(), dt, lane);
    if (lane == 0) {
        L.fz() = fz;
        L.fz3() = fz3;
    }
    lds_sync();
    if (fbox) {
        step_base_pose(L.box, dt, lane);      // the box's pose: the same update as the snake's base [U]
        lds_sync();
    }
    SNK_STAMP(8)
    // pose of the new state: feeds checkSnakeHeight and the next substep
    fk_vel(L, M, lane);
    SNK_STAMP(9)
#ifdef SNK_PROFILE
    lds_sync();
    if (lane < 9) L.taum()[lane] = (float)(prof_t[lane + 1] - prof_t[lane]);
    lds_sync();
#endif
}

}  // namespace snk
