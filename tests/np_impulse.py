"""The applied forces of the unmerged URDF tree from tests/np_model.py (test helper, not product code): what
snk_apply_impulse adds to the velocity, written from include/snk.h ("The applied forces"), not from the kernel.

    Q     = gen_force + sum_p J_p^T [f_p ; tau_p]       J_p: np_dynamics' point Jacobian of the link at the point
    delta = T x M(q)^-1 Q                               M: np_model.mass_matrix

gen_force_of(state, n, ...)  float64 Q of a call's arguments
reference(state, n, Q, T)    float64 delta = T x solve(M, Q), dense, by np_model's mass matrix
twin(state, n, ..., dtype)   the recursion the kernel uses -- articulated-body inertias inward, a 6 x 6 solve at the base,
                   accelerations outward, in world axes with each link about its own joint origin -- with every constant,
                   intermediate and result in `dtype` (float32: the yardstick of the float32 gate; float64: must reproduce
                   reference, tests/test_np_impulse.py).  Over the 3n + 2 links, as everything here; the kernel runs it over
                   the n + 1 composite bodies.
gate_case(n, P, frame)       the inputs of the GPU gate (tests/test_gpu_impulse.py) and of the CPU test that measures the
                   twin on them
"""
import numpy as np

import np_dynamics as nd_
import np_model as npm

LINK_FRAME, DRY = 1, 2
ENVS = 5
MASK = np.array([1, 1, 0, 1, 0], np.uint8)      # envs 2 and 4 are masked off
POINT_COUNTS = (1, 5, 9)


def _skew(r, dt):
    return np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], dtype=dt)


def _force_of(Rw, J, gen_force, rows, wrenches, link_frame, dt):
    """Q in dtype `dt` from kinematics already in it: J the per-link (Jw, Jv_com, COM)"""
    nd = J[0][0].shape[1]
    Q = np.zeros(nd, dt) if gen_force is None else np.asarray(gen_force, dt).copy()
    for r, w in zip(rows, np.asarray(wrenches, dt).reshape(-1, 9)):
        if not 0 <= r < len(J):
            continue
        Jw, Jv, cw = J[r]
        f, tau, x = w[0:3], w[3:6], w[6:9]
        if link_frame:
            f, tau, arm = Rw[r] @ f, Rw[r] @ tau, Rw[r] @ x
        else:
            arm = x - cw
        Jp = Jv - _skew(arm, dt) @ Jw            # the point's linear velocity per unit of u
        Q = Q + Jp.T @ f + Jw.T @ tau
    return Q


def gen_force_of(state, n, gen_force=None, rows=(), wrenches=(), link_frame=False):
    links, Rw, ow, J = nd_._kin64(state, n)[:4]
    return _force_of(Rw, J, gen_force, rows, wrenches, link_frame, np.dtype(np.float64))


def reference(state, n, Q, T):
    """(delta [nd] float64, M [nd, nd] float64)"""
    links, Rw, ow, J, pos, quat, gvel, q = nd_._kin64(state, n)
    M = npm.mass_matrix(links, pos, quat, q)
    return T * np.linalg.solve(M, np.asarray(Q, np.float64)), M


def twin(state, n, gen_force=None, rows=(), wrenches=(), link_frame=False, T=1.0, dtype=np.float32, Q=None):
    """delta [nd] in `dtype` by the articulated-body recursion at zero velocity: per link i about its own origin o_i, world
    axes, motion [alpha ; a], force [moment ; force]:
        IA_i = [[I_com + m (s.s 1 - s s^T), m [s]x], [-m [s]x, m 1]],  s = COM - o_i;   pA_i = 0 (the root: -Q[0:6])
      inward   a revolute i (S = [axis ; 0]):  U = IA S, D = S.U, u = Q_i - S.pA,  Ia = IA - U U^T / D,  pa = pA + U u / D
               (a fixed one: Ia = IA, pa = pA);  the parent takes X^T Ia X and X^T pa,  X = [[1, 0], [-[r]x, 1]], r = o_i - o_p
      base     [alpha ; a]_0 = -IA_0^-1 pA_0
      outward  a' = X a_parent;  qdd = (u - U.a') / D;  a_i = a' + S qdd
    Q given: it is used as it is (in `dtype`) instead of being formed from the arguments."""
    dtp = np.dtype(dtype)
    t = dtp.type
    links, Rw, ow, J, gvel = nd_._kin_twin(state, n, dtype)
    Q = _force_of(Rw, J, gen_force, rows, wrenches, link_frame, dtp) if Q is None else np.asarray(Q, dtype)
    L = len(links)
    eye = np.eye(3, dtype=dtype)
    ey = np.array([0, 1, 0], dtype=dtype)
    IA, pA, X = [], [], [None] * L
    for i, k in enumerate(links):
        s = J[i][2] - ow[i]
        m = t(k["m"])
        Iw = Rw[i] @ np.diag(k["I"]) @ Rw[i].T
        sx = _skew(s, dtp)
        I6 = np.zeros((6, 6), dtype)
        I6[0:3, 0:3] = Iw + m * ((s @ s) * eye - np.outer(s, s))
        I6[0:3, 3:6] = m * sx
        I6[3:6, 0:3] = -m * sx
        I6[3:6, 3:6] = m * eye
        IA.append(I6)
        pA.append(np.zeros(6, dtype))
        if i > 0:
            Xi = np.eye(6, dtype=dtype)
            Xi[3:6, 0:3] = -_skew(ow[i] - ow[k["parent"]], dtp)
            X[i] = Xi
    pA[0] = pA[0] - Q[0:6]
    U, D, uu, S = [None] * L, [None] * L, [None] * L, [None] * L
    for i in range(L - 1, 0, -1):
        k = links[i]
        Ia, pa = IA[i], pA[i]
        if k["rev"]:
            S[i] = np.concatenate([Rw[i] @ ey, np.zeros(3, dtype)])
            U[i] = IA[i] @ S[i]
            D[i] = S[i] @ U[i]
            uu[i] = Q[6 + k["dof"]] - S[i] @ pA[i]
            Ia = IA[i] - np.outer(U[i], U[i]) / D[i]
            pa = pA[i] + U[i] * (uu[i] / D[i])
        p = k["parent"]
        IA[p] = IA[p] + X[i].T @ Ia @ X[i]
        pA[p] = pA[p] + X[i].T @ pa
    acc = [None] * L
    acc[0] = -np.linalg.solve(IA[0], pA[0])
    out = np.zeros(6 + n, dtype)
    out[0:6] = acc[0]
    for i in range(1, L):
        k = links[i]
        a = X[i] @ acc[k["parent"]]
        if k["rev"]:
            qdd = (uu[i] - U[i] @ a) / D[i]
            out[6 + k["dof"]] = qdd
            a = a + S[i] * qdd
        acc[i] = a
    out = t(T) * out
    assert out.dtype == dtp and Q.dtype == dtp and IA[0].dtype == dtp
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the inputs and the figures of the gates: shared by the CPU test of the twin and the GPU test of the kernel
# ----------------------------------------------------------------------------------------------------------------------
def gate_rows(n, P):
    """P link rows: the head, a cylinder near the root, the root, mid-chain links, and the head a second time"""
    return np.array([3 * n + 1, 2, 0, 3 * (n // 2), 3 * n - 1, 5, 3 * n + 1, 7, 3 * n][:P], np.int32)


_CASES = {}


def gate_case(n, P, frame):
    """dict(S [5, state] f32, gen_force [5, nd] f32, rows [P] i32, wrenches [5, P, 9] f32, T, ref [5, nd] f64 delta, Q [5, nd]
    f64, M [5, nd, nd] f64, twin [5, nd] f32 delta) for `frame` "world" or "link": gate_states' first five, forces of a few
    newtons, torques of tenths of a newton metre, points within 5 cm of the link's COM; computed once."""
    key = (n, P, frame)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(2500 + 10 * n + P + (100 if frame == "link" else 0))
    S = nd_.gate_states(n)[:ENVS]
    nd = n + 6
    gf = np.concatenate([rng.uniform(-1, 1, (ENVS, 3)), rng.uniform(-5, 5, (ENVS, 3)), rng.uniform(-0.2, 0.2, (ENVS, n))], axis=1)
    rows = gate_rows(n, P)
    W = np.zeros((ENVS, P, 9))
    W[:, :, 0:3] = rng.uniform(-10, 10, (ENVS, P, 3))
    W[:, :, 3:6] = rng.uniform(-0.5, 0.5, (ENVS, P, 3))
    W[:, :, 6:9] = rng.uniform(-0.05, 0.05, (ENVS, P, 3))
    if frame == "world":      # a world point near the link's COM
        for e in range(ENVS):
            J = nd_._kin64(S[e], n)[3]
            for p, r in enumerate(rows):
                W[e, p, 6:9] += J[r][2]
    gf, W = gf.astype(np.float32), W.astype(np.float32)
    T = float(np.float32(1.0 / 240.0))
    lf = frame == "link"
    c = dict(n=n, P=P, frame=frame, S=S, gen_force=gf, rows=rows, wrenches=W, T=T, Q=[], ref=[], M=[], twin=[])
    for e in range(ENVS):
        Q = gen_force_of(S[e], n, gf[e], rows, W[e], lf)
        d, M = reference(S[e], n, Q, T)
        c["Q"].append(Q)
        c["ref"].append(d)
        c["M"].append(M)
        c["twin"].append(twin(S[e], n, gf[e], rows, W[e], lf, T, np.float32))
    for k in ("Q", "ref", "M", "twin"):
        c[k] = np.stack(c[k])
    _CASES[key] = c
    return c


def delta_error(delta, case, envs=None):
    """worst over the envs of |delta - ref|_inf / |ref|_inf: the error normalised by the row's largest component"""
    envs = range(ENVS) if envs is None else envs
    d = np.asarray(delta, np.float64)
    return max(float(np.max(np.abs(d[e] - case["ref"][e])) / np.max(np.abs(case["ref"][e]))) for e in envs)


def residual_error(delta, case, envs=None):
    """worst over the envs of |M delta - T Q|_inf / |T Q|_inf: free of M's conditioning"""
    envs = range(ENVS) if envs is None else envs
    d = np.asarray(delta, np.float64)
    return max(float(np.max(np.abs(case["M"][e] @ d[e] - case["T"] * case["Q"][e])) / np.max(np.abs(case["T"] * case["Q"][e])))
               for e in envs)


# The float32 twin's own worst figures over the gate's cases (tests/test_np_impulse.py,
# test_float32_twin_against_the_model, prints them and holds them under these): the floor of the GPU gate, below which a
# figure is the round-off of float32 arithmetic over this tree, whoever does it; the hard caps are ten times these.
# Measured: delta 4.63e-5 of the row's largest component (16 links, world frame, 1 point) and 5.25e-5 (32 links, world frame, 9
# points); residual 6.89e-5 of |T Q| (16 links) and 1.46e-4 (32 links, link frame, 5 points).
FLOOR_DELTA = {16: 4.7e-5, 32: 5.3e-5}
FLOOR_RESIDUAL = {16: 7.0e-5, 32: 1.5e-4}
