"""One physics substep of the snake in plain float64 numpy (test helper, not product code).

A third derivation of `stepSimulation`, beside oracle/snake_oracle.cpp (link-coordinate articulated-body algorithm) and
the HIP kernels (merged composite bodies).  It is written from the rules as DESIGN.md §3 ("[U] rules") and the field
comments of include/snk.h state them, and from plain mechanics, on top of tests/np_model.py's world-frame link
Jacobians and mass matrix:

* free motion: M a = tau_joint_damping + gravity + link damping - bias, the bias sum_i Jv_i^T m_i Jdot_v,i qdot +
  Jw_i^T (I_i Jdot_w,i qdot + w_i x I_i w_i), with Jdot qdot a central difference of the Jacobians along the motion;
  v_free = clamp(v + a dt) to +-max_coord_vel on every generalized component;
* rows at the pose of the start of the substep: violated joint limits, then motors, by joint index; per contact a normal
  row and two friction rows along the btPlaneSpace1 tangents of its normal, each scaled by R diag(aniso) R^T of link A,
  then of link B (link-link contacts; two-body rows J_A(P_A) - J_B(P_B)); static-box contacts have one-body rows;
  M^-1 J^T by np.linalg.solve;
* projected Gauss-Seidel: per sweep the non-contact rows backward on even sweeps and forward on odd ones, then every
  normal, then every friction pair (cone_friction 1: both rows from one velocity, the accumulated pair projected
  radially onto the disc of radius mu lambda_n; 0: box bounds +-mu lambda_n, skipped while the bound is zero;
  friction_directions 1: the first tangent only, box bounds); exit when the largest (dI / dinv)^2 of a sweep is at or
  below residual_threshold, or after n_iterations;
* v = clamp(v_free + dv); q += dt qd, origin += dt v, the base quaternion by the exponential map with the angular
  motion limit of pi/4 per substep;
* the order in which the solver meets the ground manifolds (`contact_order` 1 / 2 / k >= 3) from the link-ordered list:
  `manifold_order`;
* warm starting (`warm_start 1`): the normal row of a contact starts at warmstarting_factor x the impulse its cached
  point carried into the substep (`lam0`, one per contact), and the solve's velocity change starts at the sum of
  M^-1 J^T of those starts; friction and non-contact rows start at zero.

* the free box (`obstacle 2`, `box` given): a second body with six velocity components of its own, omega (3) then v (3),
  behind the snake's 6 + n.  The mass matrix is block diagonal, diag(M_snake, R diag(I) R^T, m 1_3), I = btBoxShape's
  m / 3 (hy^2 + hz^2, hx^2 + hz^2, hx^2 + hy^2) of the nominal box, or (1, 100, 1) under inertia_from_file 1.  Free motion:
  alpha = I_w^-1 (-w x I_w w - I_w w (k_a + k_a |w|)), a = (0, 0, g_z) - v (k_l + k_l |v|), clamped per component like the
  snake's.  The row of a box point P along d is J_box = [(P - c) x d ; d] over the six components (c the box's centre): a
  box-ground contact (link < 0, linkB -1) has the row +J_box(P), friction min(mu_obstacle mu_plane, 10), tangents unscaled
  (the box has no anisotropy); a link-box contact (linkB -2) has J_link(P) - J_box(PB), friction min(mu_link mu_obstacle,
  10), tangents scaled by link A's anisotropy only.  Every other rule (position error, slop, contact_erp_rule, cone /
  pyramid / one direction, solve order, residual, warm start from `lam0`) is the snake's contacts'; the box's rows come
  where the list has them.  The box is integrated like the base: v = clamp(v_free + dv), pos += dt v, the quaternion by
  the same exponential map.

The contact list (points, depths, links, normals) is an input, and so is `lam0`: tests/np_manifold.py is the model of
the contact cache that yields both for the ground contacts, the box's own (update_box) included.

Out of scope (the callers do not ask for it):
* `noncontact_order 1`;
* the joint-0 force sensor's constraint pass (obs[55]): its [U] rules are themselves open.
"""
import numpy as np

import np_model

MAX_FRICTION = 10.0                 # btManifoldResult's clamp of a combined friction coefficient [U]
ANGULAR_MOTION_THRESHOLD = 0.25 * np.pi    # btMultiBody::stepPositionsMultiDof: at most pi/4 per substep [U]
SPLIT_IMPULSE_DEPTH = -0.04          # m_splitImpulsePenetrationThreshold [U] (contact_erp_rule 1)


def skew(r):
    return np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])


def quat_mul(a, b):
    """Hamilton product of two xyzw quaternions."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def rotate_quat(quat, rv):
    """The orientation turned by the world-frame rotation vector rv (exact exponential map)."""
    th = np.linalg.norm(rv)
    dq = np.concatenate([rv * (np.sin(0.5 * th) / th if th > 0 else 0.5), [np.cos(0.5 * th)]])
    return quat_mul(dq, quat)


class Chain:
    """The snake's tree with the constants np_model restates; `p` is any object with the fields of snk_params."""

    def __init__(self, p):
        self.p = p
        self.n = int(p.n_modules)
        self.links = np_model.build_tree(self.n, from_file=bool(p.inertia_from_file), default_mass=float(p.default_mass))
        self.nd = 6 + self.n

    def split(self, s):
        n = self.n
        return s[0:3], s[3:7], s[13:13 + n], np.concatenate([s[7:13], s[13 + n:]])

    def kinematics(self, pos, quat, q):
        Rw, ow = np_model.fk(self.links, pos, quat, q)
        return Rw, ow, np_model.link_jacobians(self.links, Rw, ow)

    def jdot_qdot(self, s, h=1e-3):
        """Per link (Jdot_w g, Jdot_v g): the Jacobians differentiated along the motion (the base turned by h w about
        world axes, the origin moved by h v, q by h qd) by the fourth-order central difference; h shrinks with the
        speed, so that the truncation error (~ (h |g|)^4) stays at round-off."""
        pos, quat, q, g = self.split(s)
        h = h / max(1.0, np.abs(g).max())
        w, v, qd = g[0:3], g[3:6], g[6:]

        def jac(t):
            return self.kinematics(pos + t * v, rotate_quat(quat, t * w), q + t * qd)[2]
        c = [(-2 * h, 1.0), (-h, -8.0), (h, 8.0), (2 * h, -1.0)]
        out = [[np.zeros(3), np.zeros(3)] for _ in self.links]
        for t, wt in c:
            for i, (Jw, Jv, _) in enumerate(jac(t)):
                out[i][0] += wt * (Jw @ g)
                out[i][1] += wt * (Jv @ g)
        return [(a / (12 * h), b / (12 * h)) for a, b in out]

    def free_acceleration(self, s, tau=None, gravity=True, damping=True):
        """d/dt [w_world, v_origin_world, qd] of the unconstrained chain; returns (a, M, kinematics)."""
        p = self.p
        pos, quat, q, g = self.split(s)
        Rw, ow, J = self.kinematics(pos, quat, q)
        dJ = self.jdot_qdot(s)
        M = np.zeros((self.nd, self.nd))
        f = np.zeros(self.nd)
        if tau is not None:
            f[6:] += tau
        kl, ka = float(p.lin_damping), float(p.ang_damping)
        for i, k in enumerate(self.links):
            Jw, Jv, _ = J[i]
            Iw = Rw[i] @ np.diag(k["I"]) @ Rw[i].T
            M += k["m"] * Jv.T @ Jv + Jw.T @ Iw @ Jw
            w, vc = Jw @ g, Jv @ g
            F = np.zeros(3)
            T = np.zeros(3)
            if gravity:
                F[2] += k["m"] * float(p.gravity_z)
            if damping:
                F -= k["m"] * vc * (kl + kl * np.linalg.norm(vc))
                T -= Iw @ w * (ka + ka * np.linalg.norm(w))
            bias_v = k["m"] * dJ[i][1]
            bias_w = Iw @ dJ[i][0] + np.cross(w, Iw @ w)
            f += Jv.T @ (F - bias_v) + Jw.T @ (T - bias_w)
        return np.linalg.solve(M, f), M, (Rw, ow, J)


def plane_space(nrm):
    """btPlaneSpace1: the unit tangent t1 in the plane of the normal's two largest-reaching components (y-z when
    |n_z| > sqrt(1/2), else x-y), perpendicular to n; t2 = n x t1."""
    n = np.asarray(nrm, float)
    if abs(n[2]) > np.sqrt(0.5):
        t1 = np.array([0.0, -n[2], n[1]])
    else:
        t1 = np.array([-n[1], n[0], 0.0])
    t1 /= np.linalg.norm(t1)
    return t1, np.cross(n, t1)


def _hash_link(k, link):
    """The order key of contact_order k >= 3: the splitmix64 finaliser of k * 0x9E3779B97F4A7C15 + (link + 1) *
    0xBF58476D1CE4E5B9 (64-bit wrap-around)."""
    m = (1 << 64) - 1
    z = (k * 0x9E3779B97F4A7C15 + (link + 1) * 0xBF58476D1CE4E5B9) & m
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & m
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & m
    z ^= z >> 31
    return z


def quicksort_equal_keys(n):
    """The permutation btAlignedObjectArray::quickSort (Hoare partition, pivot = the middle element, `i <= j` swap)
    leaves on n equal keys: out[position] = original index."""
    d = list(range(n))

    def qs(lo, hi):
        i, j = lo, hi
        while True:
            if i <= j:
                d[i], d[j] = d[j], d[i]
                i += 1
                j -= 1
            if not i <= j:
                break
        if lo < j:
            qs(lo, j)
        if i < hi:
            qs(i, hi)
    if n > 1:
        qs(0, n - 1)
    return d


def cylinder_of_link(link):
    """Index in link order of the cylinder a link carries: IN_k is tree link 3k - 1, OUT_k is 3k + 1 (np_model)."""
    k, r = divmod(link + 1, 3)
    return 2 * (k - 1) if r == 0 else 2 * (k - 1) + 1


def manifold_order(C, contact_order, n):
    """Row order of the contact list C ([nc, 12] records, ground contacts first in link order) under `contact_order`:
    the ground manifolds (runs of one link among the ground contacts) permuted as whole runs -- 1 reversed, 2 by their
    cylinder's position after quickSort on 2n equal keys, k >= 3 by the hash of (k, link), ties kept -- the other
    contacts behind them as they were.  Returns the index permutation."""
    ground = [i for i in range(len(C)) if int(C[i, 5]) == -1]
    ng = len(ground)
    assert ground == list(range(ng))
    runs = []
    a0 = 0
    while a0 < ng:
        a1 = a0
        while a1 < ng and C[a1, 4] == C[a0, 4]:
            a1 += 1
        runs.append((a0, a1))
        a0 = a1
    if contact_order == 0 or ng <= 1:
        return list(range(len(C)))
    if contact_order == 1:
        key = lambda r: -r[0]                                        # noqa: E731
    elif contact_order == 2:
        pos = np.argsort(quicksort_equal_keys(2 * n))                 # cylinder -> its position after the sort
        key = lambda r: pos[cylinder_of_link(int(C[r[0], 4]))]        # noqa: E731
    else:
        key = lambda r: _hash_link(contact_order, int(C[r[0], 4]))    # noqa: E731
    out = []
    for a0, a1 in sorted(runs, key=key):                              # sorted() is stable
        out.extend(range(a0, a1))
    return out + list(range(ng, len(C)))


class Row:
    __slots__ = ("J", "Mi", "dinv", "rhs", "lo", "hi", "applied", "kind", "joint")

    def __init__(self, J, Minv_JT, target_minus_vel, lo, hi, kind, joint=-1):
        self.J = J
        self.Mi = Minv_JT
        d = float(J @ Minv_JT)
        self.dinv = 1.0 / d if d > np.finfo(float).eps else 0.0
        self.rhs = target_minus_vel * self.dinv
        self.lo, self.hi = lo, hi
        self.applied = 0.0
        self.kind, self.joint = kind, joint


def _resolve(r, dv):
    """One Gauss-Seidel step of a bounded row; returns dI / dinv (0 for a row with no effective mass)."""
    dI = r.rhs - float(r.J @ dv) * r.dinv
    s = r.applied + dI
    if s < r.lo:
        dI = r.lo - r.applied
        r.applied = r.lo
    elif s > r.hi:
        dI = r.hi - r.applied
        r.applied = r.hi
    else:
        r.applied = s
    dv += r.Mi * dI
    return dI / r.dinv if r.dinv != 0 else 0.0


def box_inertia(p):
    """The free box's inertia diagonal in its own axes."""
    if int(p.inertia_from_file):
        return np.array([1.0, 100.0, 1.0])
    hx, hy, hz = (float(x) for x in p.obstacle_half[:])
    return float(p.obstacle_mass) / 3.0 * np.array([hy * hy + hz * hz, hx * hx + hz * hz, hx * hx + hy * hy])


def integrate_quat(quat, w, dt):
    """The orientation after dt at the world angular velocity w: the exponential map with the angular motion limit and
    the third-order branch at small rates, normalised."""
    fa = np.linalg.norm(w)
    if fa * dt > ANGULAR_MOTION_THRESHOLD:
        fa = ANGULAR_MOTION_THRESHOLD / dt
    if fa < 1e-3:
        sc = 0.5 * dt - dt ** 3 / 48.0 * fa * fa      # sin(fa dt / 2) / fa to third order
    else:
        sc = np.sin(0.5 * fa * dt) / fa
    nq = quat_mul(np.concatenate([w * sc, [np.cos(0.5 * fa * dt)]]), quat)
    return nq / np.linalg.norm(nq)


def substep(p, s, targets, contacts, mu_plane=1.0, n_iterations=None, residual_threshold=None, lam0=None, box=None):
    """One substep from state s = [pos, quat xyzw, w, v, q, qd] with motor targets, on the contact list `contacts`
    ([nc, 12]: P, dist, link, linkB (-1 ground, -2 the box, >= 0 a link), normal, PB; link < 0: the free box against the
    ground) in solve order; lam0 [nc]: the impulse each contact's cached point carried (read only under warm_start 1;
    None: all zero); box [13]: the free box's state [pos, quat xyzw, omega, v] (None: no free box; linkB -2 is then the
    static one).
    Returns a dict: state (after the substep), v_free, normal / friction / limit / motor impulses, motor torques
    (impulse / dt), iterations, and the rows themselves (for complementarity checks); with `box`, its new state under
    "box", and v_free, M and the rows carry its six components behind the snake's."""
    ch = Chain(p)
    n, nd = ch.n, ch.nd
    nsn = nd                                           # the snake's components; nd: all of them
    dt = float(p.dt)
    mx = float(p.max_coord_vel)
    n_it = int(p.n_iterations if n_iterations is None else n_iterations)
    thr = float(p.residual_threshold if residual_threshold is None else residual_threshold)
    pos, quat, q, g0 = ch.split(np.asarray(s, float))
    a, M, (Rw, ow, J) = ch.free_acceleration(s, tau=-float(p.joint_damping) * g0[6:])
    if box is not None:
        box = np.asarray(box, float)
        bc, bquat, bw, bv = box[0:3], box[3:7], box[7:10], box[10:13]
        bR = np_model.quat_to_mat(bquat)
        Iw = bR @ np.diag(box_inertia(p)) @ bR.T
        ka, kl = float(p.ang_damping), float(p.lin_damping)
        Iw_w = Iw @ bw
        alpha = np.linalg.solve(Iw, -np.cross(bw, Iw_w) - Iw_w * (ka + ka * np.linalg.norm(bw)))
        lin = np.array([0.0, 0.0, float(p.gravity_z)]) - bv * (kl + kl * np.linalg.norm(bv))
        nd = nsn + 6
        Mf = np.zeros((nd, nd))
        Mf[:nsn, :nsn] = M
        Mf[nsn:nsn + 3, nsn:nsn + 3] = Iw
        Mf[nsn + 3:, nsn + 3:] = float(p.obstacle_mass) * np.eye(3)
        M = Mf
        g0 = np.concatenate([g0, bw, bv])
        a = np.concatenate([a, alpha, lin])
    v = np.clip(g0 + a * dt, -mx, mx)

    def unit_row(j, sign):
        e = np.zeros(nd)
        e[6 + j] = sign
        return e

    # non-contact rows: violated limits (a limit constraint only while q is at or beyond it), then motors
    noncontact = []
    lo_q, hi_q = float(p.joint_lo), float(p.joint_hi)
    for j in range(n):
        for sign, pen in ((1.0, q[j] - lo_q), (-1.0, hi_q - q[j])):
            if pen > 0:
                continue
            Jr = unit_row(j, sign)
            noncontact.append(Row(Jr, np.linalg.solve(M, Jr), -Jr @ v - pen * float(p.limit_erp) / dt,
                                  0.0, float(p.limit_max_impulse), "limit", j))
    for j in range(n):
        Jr = unit_row(j, 1.0)
        # POSITION_CONTROL: target velocity kp (target - q) / dt + qd + kd (0 - qd)
        want = float(p.kp) * (targets[j] - q[j]) / dt + v[6 + j] - float(p.kd) * v[6 + j]
        mi = float(p.max_motor_impulse)
        noncontact.append(Row(Jr, np.linalg.solve(M, Jr), want - v[6 + j], -mi, mi, "motor", j))

    def point_jac(link, P):
        out = np.zeros((3, nd))
        if link >= 0:
            Jw, Jv, c = J[link]
            out[:, :nsn] = Jv - skew(np.asarray(P) - c) @ Jw         # v_P = v_c + w x (P - c)
        else:                                              # the free box: v_P = v + omega x (P - c)
            out[:, nsn:nsn + 3] = -skew(np.asarray(P) - bc)
            out[:, nsn + 3:] = np.eye(3)
        return out

    def aniso(link, d):
        return Rw[link] @ (np.asarray(p.aniso, float) * (Rw[link].T @ d))

    contacts = np.asarray(contacts, float).reshape(-1, 12)
    mu_ground = min(float(p.mu_link) * mu_plane, MAX_FRICTION)
    mu_self = min(float(p.mu_link) ** 2, MAX_FRICTION)
    mu_box = min(float(p.mu_link) * float(p.mu_obstacle), MAX_FRICTION)
    mu_box_ground = min(float(p.mu_obstacle) * mu_plane, MAX_FRICTION)
    normals, pairs, mus = [], [], []
    for c in contacts:
        P, dist, la, lb, nrm, PB = c[0:3], c[3], int(c[4]), int(c[5]), c[6:9], c[9:12]
        assert la >= 0 or (box is not None and lb == -1), "a contact of the free box itself: with the ground, `box` given"
        Jp = point_jac(la, P)
        if lb >= 0:
            Jp = Jp - point_jac(lb, PB)
        elif lb == -2 and box is not None:
            Jp = Jp - point_jac(-1, PB)
        mus.append(mu_box_ground if la < 0 else mu_self if lb >= 0 else (mu_box if lb == -2 else mu_ground))
        Jn = nrm @ Jp
        Mn = np.linalg.solve(M, Jn)
        pen = dist + float(p.linear_slop)
        if pen > 0:
            err = -pen / dt                                # speculative contact: close the gap in one substep
        else:
            erp = float(p.contact_erp)
            if int(p.contact_erp_rule) and pen > SPLIT_IMPULSE_DEPTH:
                erp = 0.2                                  # m_erp (btContactSolverInfo default) [U]
            err = -pen * erp / dt
        normals.append(Row(Jn, Mn, -Jn @ v + err, 0.0, 1e10, "normal"))
        fr = []
        for f, t in enumerate(plane_space(nrm)):
            d = aniso(la, t) if la >= 0 else t             # (the box has no anisotropic friction)
            if lb >= 0:
                d = aniso(lb, d)
            Jf = d @ Jp
            r = Row(Jf, np.linalg.solve(M, Jf), -Jf @ v, 0.0, 0.0, "friction")
            fr.append(r)
        pairs.append(fr)

    dv = np.zeros(nd)
    if int(p.warm_start) and lam0 is not None:
        for r0, l0 in zip(normals, np.asarray(lam0, float)):
            r0.applied = float(p.warmstarting_factor) * l0
            dv += r0.Mi * r0.applied
    iters = 0
    nn = len(noncontact)
    one_dir = int(p.friction_directions) == 1
    cone = int(p.cone_friction) != 0
    for it in range(n_it):
        lsq = 0.0
        for j in range(nn):
            r = _resolve(noncontact[nn - 1 - j if it % 2 == 0 else j], dv)
            lsq = max(lsq, r * r)
        for r0 in normals:
            r = _resolve(r0, dv)
            lsq = max(lsq, r * r)
        for ci, (A, B) in enumerate(pairs):
            lim = mus[ci] * normals[ci].applied
            if one_dir:
                if lim > 0:
                    A.lo, A.hi = -lim, lim
                    r = _resolve(A, dv)
                    lsq = max(lsq, r * r)
            elif cone:
                sA = A.applied + A.rhs - float(A.J @ dv) * A.dinv
                sB = B.applied + B.rhs - float(B.J @ dv) * B.dinv
                rr = np.hypot(sA, sB)
                if rr > lim:
                    sc = lim / rr if rr > 0 else 0.0
                    sA, sB = sA * sc, sB * sc
                dA, dB = sA - A.applied, sB - B.applied
                A.applied, B.applied = sA, sB
                dv += A.Mi * dA + B.Mi * dB
                for d_, rw in ((dA, A), (dB, B)):
                    r = d_ / rw.dinv if rw.dinv != 0 else 0.0
                    lsq = max(lsq, r * r)
            elif lim > 0:
                for rw in (A, B):
                    rw.lo, rw.hi = -lim, lim
                    r = _resolve(rw, dv)
                    lsq = max(lsq, r * r)
        iters = it + 1
        if lsq <= thr:
            break

    vn = np.clip(v + dv, -mx, mx)
    out = np.asarray(s, float).copy()
    out[7:13] = vn[0:6]
    out[13 + n:] = vn[6:nsn]
    out[13:13 + n] = q + dt * vn[6:nsn]
    out[0:3] = pos + dt * vn[3:6]
    out[3:7] = integrate_quat(quat, vn[0:3], dt)
    box_out = None
    if box is not None:
        box_out = np.concatenate([bc + dt * vn[nsn + 3:], integrate_quat(bquat, vn[nsn:nsn + 3], dt), vn[nsn:]])
    tau_motor = np.zeros(n)
    for r in noncontact:
        if r.kind == "motor":
            tau_motor[r.joint] = r.applied / dt
    return dict(state=out, v_free=v, acc=a, M=M, iterations=iters, tau_motor=tau_motor,
                normal=np.array([r.applied for r in normals]),
                friction=np.array([[A.applied, B.applied] for A, B in pairs]).reshape(-1, 2),
                noncontact=noncontact, normals=normals, pairs=pairs, mus=np.array(mus), dv=dv, box=box_out)
