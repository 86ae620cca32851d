// snk_lds.hpp -- the LDS image of one environment (one wave holds one environment): the part both solves share, the
// streamed-row and the register-resident layouts, the solver-rules variants, and the build-time (-D) knobs that size them.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "snk_model.hpp"

// -DSNK_PROFILE (bullet-envs_amd/build.py --profile): s_memtime stamps between the phases of a substep; the phase
// durations (ticks) replace the motor torques of the record (tools/profile_phases.py)
#ifdef SNK_PROFILE
#define SNK_STAMP(i) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); prof_t[i] = t_; }
#define SNK_PROF_T_PARAM , unsigned long long* prof_t
#define SNK_PROF_T_ARG , prof_t
#else
#define SNK_STAMP(i)
#define SNK_PROF_T_PARAM
#define SNK_PROF_T_ARG
#endif
// -DSNK_PROFILE -DSNK_PROFILE_FINE (build.py --profile-fine): a second set of stamps around the dynamics' own pieces --
// integrate, fk_vel, body_bias, the inward sweep, the base inverse, the outward sweep -- whose durations take the coarse
// phases' place in the record (tools/profile_phases.py fine), and behind them the pieces of find_contacts_v2 (obstacle and
// self-pair tests; manifold load, refresh, drop; the support search; nearest / sort / insert; prefix and stores).  A
// function that is also called without the table takes it as a pointer that may be null.
#if defined(SNK_PROFILE) && defined(SNK_PROFILE_FINE)
#define SNK_FSTAMP(i) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); if (prof_f) prof_f[i] = t_; }
#else
#define SNK_FSTAMP(i)
#endif
// The tables travel as a last parameter that exists in the instrumented builds only (SNK_PROF_T_PARAM / SNK_PROF_F_PARAM
// close a signature, SNK_PROF_T_ARG / SNK_PROF_F_ARG a call): text, not a type, so that a __noinline__ function's ABI
// in the product is the one it has without them.
#ifdef SNK_PROFILE_FINE
#define SNK_PROF_F_PARAM , unsigned long long* prof_f = nullptr
#define SNK_PROF_F_ARG , prof_f
#else
#define SNK_PROF_F_PARAM
#define SNK_PROF_F_ARG
#endif

namespace snk {

// ----------------------------------------------------------------------------------
// LDS image of one environment
// ----------------------------------------------------------------------------------
template <int N, int NL>
struct LdsCommon {
    static constexpr int kN = N;
    static constexpr int kNCO = 0;       // snk_params::noncontact_order this image's kernels are compiled for (LdsFor)
    static constexpr bool kERP = false;  // contact_erp_rule's depth test compiled in (LdsFor)
    static constexpr int NB = N + 1;     // composite bodies
    static constexpr int ND = N + 6;     // generalized velocity [omega_w, v_w, qd]
    static constexpr int NC = 4 * N;     // contact slots: 2n cylinders x 2 end caps
    static constexpr int NR = 3 * NC;    // contact rows: normal + 2 friction
    static constexpr int REC = (N <= 16) ? 64 : 128;
    // HBM record, same order: base[13] q[N] qd[N] taum[N] fz prev_x
    float rec[REC];
    // per body, world axes
    float R[NB][9], o[NB][3], r[NB][3], ax[NB][3], cw[NB][3];
    float w[NB][3], v[NB][3], zeta[NB][6], p[NB][6];
    float IA[NB][21];            // articulated inertia: A(6 sym) B(9) C(6 sym)
    float Ua[NB][3], Ub[NB][3], Dinv[NB], u[NB];
    float Inv0[36];
    float qd_old[N], tauj[N], qdd[N], targets[N];
    float acc0[6];
    // non-contact rows kept in LDS (NL of them): in v1 limits + motors (2 N), in v2 only the (rare) limit rows (N)
    int nc_joint[NL];
    float nc_sign[NL], nc_rhs[NL], nc_dinv[NL], nc_den[NL], nc_lo[NL], nc_hi[NL], nc_app[NL];

    // SNK_POISON=1 (snk_create; tests): every float of the image becomes a NaN before an environment is loaded, so that a
    // read of something this substep did not write shows up in the outputs instead of depending on what the previous
    // environment -- or another kernel -- left behind.  (The integer tables are left alone: a NaN's bits as an index
    // would turn such a bug into a wild address.)
    __device__ __forceinline__ void poison_common(int lane) {
        float* a = rec;
        const int nf = (int)(reinterpret_cast<float*>(nc_joint) - a);
        for (int i = lane; i < nf; i += 64) a[i] = __int_as_float(0x7fc00000);
        float* b = nc_sign;
        for (int i = lane; i < 7 * NL; i += 64) b[i] = __int_as_float(0x7fc00000);
    }
    __device__ __forceinline__ float* base() { return rec; }
    __device__ __forceinline__ float* q() { return rec + 13; }
    __device__ __forceinline__ float* qd() { return rec + 13 + N; }
    __device__ __forceinline__ float* taum() { return rec + 13 + 2 * N; }
    __device__ __forceinline__ float& fz() { return rec[13 + 3 * N]; }
    __device__ __forceinline__ float& prev_x() { return rec[14 + 3 * N]; }
    __device__ __forceinline__ float& fz3() { return rec[15 + 3 * N]; }   // reaction Fz of the first motor joint (streamed-row solve)
};

// Register budget of the streamed-row solve (experiments: -DSNK_V1_RESN=.. etc. through build.py's `defines`; the defaults
// are what ships).  Round 4's sweep on configs[3] (profiles/r04_c32_ring_sweep.txt): look-ahead beyond 16 normals / 16
// friction pairs buys nothing, every resident normal saves its 320 bytes per iteration -- 40 / 16 / 16 runs at 91.7 k
// env-steps/s against 89.9 k for round 2-3's 32 / 32 / 16; 48 resident or 24 pairs in flight spill into the loop.
#ifndef SNK_V1_RESN
#define SNK_V1_RESN 40
#endif
#ifndef SNK_V1_RINGN
#define SNK_V1_RINGN 16
#endif
#ifndef SNK_V1_RINGF
#define SNK_V1_RINGF 16
#endif
#ifndef SNK_LB
#define SNK_LB 2
#endif
// (the same three numbers for the copy that runs inside the register-resident kernels, pgs_v1<LT, INPLACE = true>)
#ifndef SNK_IP_RESN
#define SNK_IP_RESN 32
#endif
#ifndef SNK_IP_RINGN
#define SNK_IP_RINGN 32
#endif
#ifndef SNK_IP_RINGF
#define SNK_IP_RINGF 16
#endif
#ifndef SNK_V1_LDAUX
#define SNK_V1_LDAUX 0      // cache policy bits of the streamed rows' buffer loads (experiments: 1 sc0, 2 nt, 16 sc1)
#endif

template <int N, bool V2>
struct Lds;

// v1: every constraint row staged in LDS (any chain length; used for the 32-link config)
template <int N>
struct Lds<N, false> : LdsCommon<N, 2 * N> {
    static constexpr bool kV2 = false;
    // ground-contact slots: 128 for BOTH chain lengths.  The 32-link chain's two end-cap points per cylinder; for the
    // 16-link chain every point its 32 cylinders' manifolds can hold (4 each) -- this solve is where an environment
    // goes whose contacts do not fit the register-resident solve's 64 slots (snk_api.hip: overflow list), so that no
    // 16-link contact is ever left without rows
    // contact slots: every point the 2N cylinders' manifolds can hold (4 each) -- Bullet has no limit, and neither has
    // this solve for the ground contacts
    static constexpr int NC = 8 * N, NR = 3 * NC, ND = N + 6;
    float ext_[LdsCommon<N, 2 * N>::NB][6];      // link forces of the constraint pass
    __device__ __forceinline__ float* ext(int b) { return ext_[b]; }
    __device__ __forceinline__ void poison(int lane) {
        this->poison_common(lane);
        poison_own(lane);
    }
    // the members behind the common part only: what a register-resident kernel's rare streamed-row substep finds there is
    // that kernel's own leftovers (finite numbers: the poison of the environment's load is long overwritten)
    __device__ __forceinline__ void poison_own(int lane) {
        for (int i = lane; i < LdsCommon<N, 2 * N>::NB * 6; i += 64) (&ext_[0][0])[i] = __int_as_float(0x7fc00000);
        for (int i = lane; i < (NC + kRing + 3) * 4; i += 64) (&acc[0][0])[i] = __int_as_float(0x7fc00000);
    }
    int clist[NC];               // compact contact index -> slot
    int cidx[NC];                // slot -> compact contact index (-1: not in contact)
    // The contact rows themselves (J and M^-1 J^T, 2 x 384 x 38 floats = 117 KB) do not fit LDS next
    // to anything else; they live in a per-resident-wave block of global memory that the solve
    // streams once per iteration (see pgs_v1), one 320-byte record [J | M^-1 J^T] per row.
    static constexpr int kRing = 32;                       // padding entries behind the ground contacts' impulses (the link-link contacts' live there)
    static constexpr int kResN = SNK_V1_RESN;              // contacts whose normal rows stay in registers over the solve
    static constexpr int kRingN = SNK_V1_RINGN;            // normal rows in flight behind them
    static constexpr int kRingF = SNK_V1_RINGF;            // friction pairs in flight
    // link-link (self-collision) contacts follow the ground contacts in the compact list: at most kMaxSelf of them,
    // geometry slots NC .. NC + kMaxSelf - 1
    static constexpr int kMaxSelf = kRing;
    static constexpr int NCT = NC + kMaxSelf;              // contact slots in all
    // record order: the NCT normal rows, then the NCT friction pairs (A, B) -- each phase of the solve streams its own
    // rows back to back, every fetched cache line used whole (interleaved by contact, a phase used 320 of every 960
    // bytes and paid for the neighbours' half lines), then 3 rows that stay zero.  Inside a record the vectors are
    // interleaved by column -- a friction pair's 640 bytes are [JA0 JB0 MA0 MB0 JA1 ...], and the normals of contacts 2p,
    // 2p + 1, which the solve resolves in one step, share 640 bytes [J(2p)0 M(2p)0 J(2p+1)0 M(2p+1)0 J(2p)1 ...] (since the end of
    // round 4; 320 bytes per contact before: +1.5 %) -- so that lane d fetches everything it needs for a step with ONE
    // 16-byte load
    static constexpr int kRows = 3 * NCT + 3;
    static constexpr int kFric = NCT;                      // first friction record
    // a row of the block: [J (ND floats), pad, M^-1 J^T (ND floats), pad], 320 B = five aligned 64-B
    // sectors for 304 useful bytes (separate, unaligned 152-B rows fetched 1.4x their size)
    static constexpr int kRS = 80;                         // floats per row of the block
    static constexpr int kMO = 40;                         // float offset of the M^-1 J^T half
    // The two pad columns of each half carry the row's scalars, so that the solve needs nothing but the accumulated
    // impulses in LDS (round 2: 7.7 KB of per-contact scalars {rhs, den, 1/den, a} shrank to 2.5 KB of a's):
    //   J half:        columns < ND  J / den;   column kSpec  -rhs = -target / den;   column kSpec + 1  0
    //   M^-1 J^T half: columns < ND  M^-1 J^T;  column kSpec  0;                      column kSpec + 1  den
    // With delta-v's lane kSpec held at 1 the row's dot IS (J.dv)/den - rhs, and lane kSpec + 1 of the step's
    // M^-1 J^T dI is dI * den, the row's residual (the same layout trick as the register-resident solve's d = 22 / 24).
    static constexpr int kSpec = kMO - 2;
    static_assert(ND <= kSpec, "row layout");
    // behind the rows: the contact geometry of the NCT slots, 20 floats each: P[3] (point on body kA), distance,
    // friction direction A[3], B[3], normal[3], PB[3] (point on body kB), kA, kB (-1: the ground), friction scale,
    // pad (written lane = slot by find_contacts_v1 / find_self_contacts_v1, read by the row builder and the
    // sensor pass)
    static constexpr int kGeo = 20;
    static constexpr size_t kGeoOff = (size_t)kRows * kRS;
    // behind the geometry: M^-1 e_j of the n motor / limit rows, kMO floats each (columns >= ND zero).  The solve keeps
    // them in registers; they left LDS (4.9 KB for 32 links) so that eight waves fit a CU
    static constexpr size_t kMmOff = kGeoOff + (size_t)NCT * kGeo;     // M^-1: ND rows (6 base, then the joints) of kMO floats
    // (+ 6 rows and one more Y for the free box of obstacle 2, a second "tree" with six velocity components of its own
    //  behind the snake's: lanes ND .. ND + 5 of the solve, body index N + 1 in the contact records)
    static constexpr int kBoxBody = N + 1;
    static constexpr size_t kYOff = kMmOff + (size_t)(N + 6 + 6) * kMO;     // Y_k of every body (build_rows_v1), 6 x kMO floats each
    static constexpr size_t kRowFloats = kYOff + (size_t)(N + 2) * 6 * kMO;
    static_assert(N + 6 + 6 <= kSpec || N > 16, "the free box's lanes must fit in front of the scalar columns (16 links)");
    // accumulated impulses of contact ci: {normal, friction A, friction B, -}
    alignas(16) float acc[NC + kRing + 3][4];        // (+ the entries the solve reads ahead of the last pair)
    static_assert(NCT <= NC + kRing, "the impulses of the link-link contacts live in the ring's padding entries");
    int nplane;                  // ground contacts of this substep (the link-link contacts follow them)
    // obstacle 2: the free box while this wave holds the environment -- state [pos3, quat4, omega3, vel3], its world
    // rotation and world inverse inertia (sym6) for this substep, its manifold with the plane (4 x (a3, b.x, b.y,
    // lambda)) and the point count; travels with the state record (d_box)
    float box[13], bR[9], bIw[6], bman[24];
    int bmn;
    // ... and the plane's own friction coefficient of the environment (set_box_plane_mu; lane 0 writes and reads it): the
    // box-ground pair combines it with the box's and clamps the product, which the snake's clamped mu cannot give back
    float bmu;
};

// v2: rows live in VGPRs during the solve; LDS only stages one 64-row batch while they are built
template <int N>
struct Lds<N, true> : LdsCommon<N, N> {
    static constexpr bool kV2 = true;
    static constexpr int NC = 4 * N, ND = N + 6;
    static_assert(N + 6 + 3 <= 32, "v2 packs two rows per 64-lane register");
    float Mm[N][ND];             // M^-1 e_j for the motor / limit rows
    static constexpr int kObs = 8;                        // room for contacts with the obstacle box (behind the ground's)
    float ccP[NC][3], ccdist[NC];                         // indexed by COMPACT contact index
    unsigned char ccbody[NC], ccds[NC];                   // ... the contact's body; its entry of cdir
    // friction directions A, B: one entry per CYLINDER (all ground contacts of a cylinder share them), then one per
    // obstacle contact, whose normals are obn (a ground contact's is +z)
    float cdir[2 * N + kObs][2][3], obn[kObs][3];
    float stM[64][25];           // staging of one 64-row batch: M^-1 J^T [22], rhs, den, 1/den
    // link forces of the constraint pass: columns 8..13 of the staging rows, which that pass uses in columns 0..5 only
    __device__ __forceinline__ float* ext(int b) { return &stM[b][8]; }
    float MmS[N][4];             // the motors' rhs, den, 1/den, target velocity change (their M^-1 rows are Mm)
    float fz_park, fz3_park;     // first-pass parts of the joint-0 force and of the first motor joint's reaction, parked across the solve
    int nplane;                  // ground contacts of this substep (the obstacle's follow them in the compact list)
    // contacts of cylinder c: compact indices [cylbase[c], + cyln[c]); cylkeep[c]: which of its cached manifold points
    // they are (bit j = point j has rows; contact_model 1)
    unsigned char cylbase[2 * N], cyln[2 * N], cylkeep[2 * N];
    float app[2 * (N / 2 + NC / 2 + NC)];   // accumulated impulses by (register slot, half)
    // contact_model 1: the environment's persistent contact manifolds stay HERE while a wave holds the environment
    // (read and updated every substep, lane = cylinder); they travel to and from global memory with the state record
    // only -- at the start and the end of an env-step and at a hand-off between waves.  Component-major, so that lane
    // = cylinder strides by one word: per cached point j the floats [6 j .. 6 j + 5] = point on the link in link
    // coordinates (3), point on the ground x, y (its z is the plane's: 0), the normal impulse of the last substep
    float mfl[24][2 * N];
    unsigned char mfn[2 * N];    // cached points of cylinder c
    __device__ __forceinline__ void poison(int lane) {
        this->poison_common(lane);
        auto fill = [&](float* a, int n) { for (int i = lane; i < n; i += 64) a[i] = __int_as_float(0x7fc00000); };
        fill(&Mm[0][0], N * ND); fill(&ccP[0][0], NC * 3); fill(ccdist, NC); fill(&cdir[0][0][0], (2 * N + kObs) * 6);
        fill(&obn[0][0], kObs * 3); fill(&stM[0][0], 64 * 25); fill(&MmS[0][0], N * 4);
        fill(app, 2 * (N / 2 + NC / 2 + NC)); fill(&mfl[0][0], 24 * 2 * N);
    }
};

// The image the solving kernels of one solver-rules variant use (RULES, a kernel template parameter): the same layout, with
// the rules as compile-time constants.  RULES 0 = both rules at their defaults: Lds itself, so that the default kernels
// compile from exactly the code they did before the rules existed.  RULES 1 = noncontact_order 0 with contact_erp_rule's
// depth test (LT::kERP); RULES 2 = noncontact_order 1 (LT::kNCO: the solves unroll their motor sweeps over that order)
// with the depth test -- under contact_erp_rule 0 both of its ERPs are contact_erp, the same bits as without it.
template <class Base, int NCO>
struct LdsRules : Base {
    static constexpr int kNCO = NCO;
    static constexpr bool kERP = true;
};
template <int N, bool V2, int RULES>
using LdsFor = typename std::conditional<RULES == 0, Lds<N, V2>, LdsRules<Lds<N, V2>, RULES == 2 ? 1 : 0>>::type;
// the variant a parameter set runs on
inline int rules_variant(const DevModel& D) { return D.noncontact_order ? 2 : (D.contact_erp_rule ? 1 : 0); }

__device__ __forceinline__ void lds_sync() { __syncthreads(); }

// What the caller knows about a substep's place in the servo loop (snake.py:283-304).  The joint-0
// force sensor (obs[55]) is only observable after the LAST substep of an env-step, so the
// register-resident substep runs its second ABA pass only when this substep can be the last one.
struct SensorHint {
    bool always;        // single-substep API: every substep is observable
    int counter_next;   // value of `counter` after this substep
    float h_prev;       // checkSnakeHeight's mean height of the pose the substep starts from
};

}  // namespace snk
