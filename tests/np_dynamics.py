"""Mass matrix, bias forces and link Jacobians of the unmerged URDF tree from tests/np_model.py (test helper, not product
code): what snk_dynamics and snk_jacobians return, written from include/snk.h ("The dynamics queries"), not from the kernel.

    u = [omega_world 3 | v_world of the root origin 3 | qd n],   M du/dt + h = Q
    M = sum_links  m Jv^T Jv + Jw^T I_w Jw                                         (np_model.mass_matrix)
    h = sum_links  Jv^T m (a - g) + Jw^T (I_w alpha + omega x I_w omega)
        (a, alpha): the velocity-product accelerations of each link's COM, by the analytic parent-to-child recursion at
        du/dt = 0 (the root's origin does not accelerate, its omega does not change); flags 1: these terms at the state's u
        (g = 0), flags 2: minus the generalised gravity force (u = 0), flags 3: both
    J of a point x = COM + R_link local of link row r:  rows 0-2  Jv_com - [x - COM]x Jw,  rows 3-5  Jw

reference(state, n, flags)  float64 (M, h), by np_model's functions themselves, on the float32 state the GPU was handed
jacobian(state, n, row, local)  float64 [6, nd]
twin(state, n, flags, dtype)    the SAME formulas with every constant, intermediate and result in `dtype` (float32: the
                   yardstick of the float32 gate, conftest.f32_gate -- what float32 arithmetic over the 3n + 2-link tree
                   costs, measured, not the kernel; float64: must reproduce reference, tests/test_np_dynamics.py)
The kernels sum over the n + 1 composite bodies; everything here sums over the 3n + 2 links.
"""
import numpy as np

import np_model as npm
from np_link_states import split_state

VELOCITY, GRAVITY = 1, 2
GZ = -9.8


# ----------------------------------------------------------------------------------------------------------------------
# velocity-product accelerations (any dtype: every operand already has it)
# ----------------------------------------------------------------------------------------------------------------------
def vp_accelerations(links, Rw, ow, cws, gvel):
    """Per link (omega, alpha, a_com) at du/dt = 0: parent to child,
        omega_i = omega_p + axis_i qd_i,                alpha_i = alpha_p + omega_p x axis_i qd_i          (revolute i)
        a(o_i)  = a(o_p) + alpha_p x d + omega_p x (omega_p x d),   d = o_i - o_p     (o_i is fixed in the parent)
        a_com   = a(o_i) + alpha_i x s + omega_i x (omega_i x s),   s = COM_i - o_i"""
    dt = ow[0].dtype
    ey = np.array([0, 1, 0], dtype=dt)
    zero = np.zeros(3, dt)
    om, al, ao, out = [gvel[0:3]], [zero], [zero], []
    for i, k in enumerate(links):
        if i > 0:
            p = k["parent"]
            d = ow[i] - ow[p]
            ao.append(ao[p] + np.cross(al[p], d) + np.cross(om[p], np.cross(om[p], d)))
            if k["rev"]:
                rate = (Rw[i] @ ey) * gvel[6 + k["dof"]]
                om.append(om[p] + rate)
                al.append(al[p] + np.cross(om[p], rate))
            else:
                om.append(om[p])
                al.append(al[p])
        s = cws[i] - ow[i]
        out.append((om[i], al[i], ao[i] + np.cross(al[i], s) + np.cross(om[i], np.cross(om[i], s))))
    return out


def _bias(links, Rw, ow, J, gvel, flags, dt):
    """h of the module docstring, in the operands' dtype"""
    nd = J[0][0].shape[1]
    u = gvel if flags & VELOCITY else np.zeros(nd, dt)
    g = np.array([0, 0, GZ if flags & GRAVITY else 0.0], dtype=dt)
    acc = vp_accelerations(links, Rw, ow, [j[2] for j in J], u)
    h = np.zeros(nd, dt)
    for i, k in enumerate(links):
        Jw, Jv, _ = J[i]
        om, al, a = acc[i]
        Iw = Rw[i] @ np.diag(np.asarray(k["I"], dt)) @ Rw[i].T
        h += Jv.T @ (dt.type(k["m"]) * (a - g)) + Jw.T @ (Iw @ al + np.cross(om, Iw @ om))
    return h


def _point_jacobian(links, Rw, J, row, local, dt):
    Jw, Jv, cw = J[row]
    out = np.zeros((6, Jw.shape[1]), dt)
    out[0:3] = Jv
    out[3:6] = Jw
    if local is not None:
        r = Rw[row] @ np.asarray(local, dt)
        out[0:3] -= np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], dtype=dt) @ Jw
    return out


# ----------------------------------------------------------------------------------------------------------------------
# float64, by np_model
# ----------------------------------------------------------------------------------------------------------------------
def _kin64(state, n):
    links = npm.build_tree(n)
    pos, quat, gvel, q = split_state(np.asarray(state, np.float64), n)
    Rw, ow = npm.fk(links, pos, quat, q)
    return links, Rw, ow, npm.link_jacobians(links, Rw, ow), pos, quat, gvel, q


def reference(state, n, flags=VELOCITY | GRAVITY):
    """(M [nd, nd], h [nd]) float64; flags a tuple: (M, {flags: h})"""
    links, Rw, ow, J, pos, quat, gvel, q = _kin64(state, n)
    M = npm.mass_matrix(links, pos, quat, q)
    if isinstance(flags, tuple):
        return M, {f: _bias(links, Rw, ow, J, gvel, f, np.dtype(np.float64)) for f in flags}
    return M, _bias(links, Rw, ow, J, gvel, flags, np.dtype(np.float64))


def jacobian(state, n, row, local=None):
    """[6, nd] float64 of the point `local` (COM frame; None: the COM) of link row `row`"""
    links, Rw, ow, J = _kin64(state, n)[:4]
    return _point_jacobian(links, Rw, J, row, local, np.dtype(np.float64))


def accelerations(state, n):
    """Per link (omega, alpha, a_com) float64 at the state's u (what tests/test_np_dynamics.py differentiates J u against)"""
    links, Rw, ow, J, pos, quat, gvel, q = _kin64(state, n)
    return vp_accelerations(links, Rw, ow, [j[2] for j in J], gvel)


def link_twists(state, n):
    """Per link (v_com, omega) = (Jv u, Jw u) float64"""
    links, Rw, ow, J, pos, quat, gvel, q = _kin64(state, n)
    return [(Jv @ gvel, Jw @ gvel) for Jw, Jv, _ in J]


def flow(state, n, t):
    """The state after time t along the flow of its own FIXED u: pos + v t, quat <- exp(omega t) (x) quat, q + qd t"""
    s = np.array(state, np.float64)
    w = s[7:10]
    s[0:3] += s[10:13] * t
    ang = np.linalg.norm(w) * t
    if ang != 0.0:
        ax = w / np.linalg.norm(w)
        dx, dy, dz, dw = (*(np.sin(ang / 2) * ax), np.cos(ang / 2))
        x, y, z, qw = s[3:7]
        s[3:7] = [dw * x + dx * qw + dy * z - dz * y, dw * y - dx * z + dy * qw + dz * x,
                  dw * z + dx * y - dy * x + dz * qw, dw * qw - dx * x - dy * y - dz * z]
    s[13:13 + n] += s[13 + n:13 + 2 * n] * t
    return s


# ----------------------------------------------------------------------------------------------------------------------
# the twin: np_model.quat_to_mat, rot_y, fk, link_jacobians and mass_matrix restated line by line in `dtype`
# ----------------------------------------------------------------------------------------------------------------------
def _kin_twin(state, n, dtype):
    dt = np.dtype(dtype).type
    links = [dict(k, R=k["R"].astype(dtype), p=k["p"].astype(dtype), c=k["c"].astype(dtype), I=np.asarray(k["I"]).astype(dtype))
             for k in npm.build_tree(n)]
    pos, quat, gvel, q = (np.asarray(a, dtype) for a in split_state(state, n))
    x, y, z, w = quat / np.linalg.norm(quat)
    one, two = dt(1), dt(2)
    R0 = np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                   [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                   [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=dtype)

    def rot_y(a):
        c, s = np.cos(a), np.sin(a)          # (numpy keeps a float32 scalar's dtype)
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=dtype)

    Rw, ow = [R0], [pos]
    for i in range(1, len(links)):
        k = links[i]
        R = k["R"] @ rot_y(q[k["dof"]]) if k["rev"] else k["R"]
        Rw.append(Rw[k["parent"]] @ R)
        ow.append(ow[k["parent"]] + Rw[k["parent"]] @ k["p"])
    nd = 6 + n
    ey = np.array([0, 1, 0], dtype=dtype)
    J = []
    for i, k in enumerate(links):
        cw = ow[i] + Rw[i] @ k["c"]
        Jw = np.zeros((3, nd), dtype)
        Jv = np.zeros((3, nd), dtype)
        Jw[:, 0:3] = np.eye(3, dtype=dtype)
        Jv[:, 3:6] = np.eye(3, dtype=dtype)
        r = cw - ow[0]
        Jv[:, 0:3] = -np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], dtype=dtype)
        j = i
        while j > 0:
            kj = links[j]
            if kj["rev"]:
                a = Rw[j] @ ey
                Jw[:, 6 + kj["dof"]] = a
                Jv[:, 6 + kj["dof"]] = np.cross(a, cw - ow[j])
            j = kj["parent"]
        J.append((Jw, Jv, cw))
    return links, Rw, ow, J, gvel


def twin(state, n, flags=VELOCITY | GRAVITY, dtype=np.float32, points=()):
    """(M, h, [J of every (row, local) of `points`]) in `dtype` throughout; flags a tuple: h is {flags: h}"""
    dtp = np.dtype(dtype)
    links, Rw, ow, J, gvel = _kin_twin(state, n, dtype)
    M = np.zeros((6 + n, 6 + n), dtype)
    for i, k in enumerate(links):
        Jw, Jv, _ = J[i]
        Iw = Rw[i] @ np.diag(k["I"]) @ Rw[i].T
        M += dtp.type(k["m"]) * Jv.T @ Jv + Jw.T @ Iw @ Jw
    many = isinstance(flags, tuple)
    hs = {f: _bias(links, Rw, ow, J, gvel, f, dtp) for f in (flags if many else (flags,))}
    h = hs if many else hs[flags]
    Js = [_point_jacobian(links, Rw, J, row, local, dtp) for row, local in points]
    assert M.dtype == dtp and all(v.dtype == dtp for v in hs.values()) and all(j.dtype == dtp for j in Js) and all(m.dtype == dtp for m in Rw)
    return M, h, Js


# ----------------------------------------------------------------------------------------------------------------------
# the states and the figures of the gates: shared by the CPU test of the twin and the GPU test of the kernels
# ----------------------------------------------------------------------------------------------------------------------
def gate_states(n, count=24):
    """test_gpu_world's family: a tumbled base, joints across their range, non-zero twists -- rounded to float32, as the
    handle holds them"""
    from conftest import random_state
    rng = np.random.default_rng(2600 + n)
    return np.stack([random_state(rng, n, z=0.3, qamp=1.5, vamp=1.0) for _ in range(count)]).astype(np.float32)


def gate_points(n):
    """(link row, local point) of the Jacobian gates: the COMs of the 2n cylinder links (rows 3k - 1 and 3k + 1, k = 1 .. n)
    and a point 0.05 m off the head's COM (the head: the last OUTPUT_BODY, row 3n + 1)"""
    rows = sorted([3 * k - 1 for k in range(1, n + 1)] + [3 * k + 1 for k in range(1, n + 1)])
    return [(r, None) for r in rows] + [(3 * n + 1, (0.03, -0.04, 0.0))]


def points_arrays(points):
    """(link_rows int32 [P], local float32 [P, 3]) of a list of gate_points' kind"""
    rows = np.array([r for r, _ in points], np.int32)
    local = np.array([(0.0, 0.0, 0.0) if l is None else l for _, l in points], np.float32)
    return rows, local


BLOCKS = ("base", "base-joint", "joint")
H_BLOCKS = (("moment", slice(0, 3)), ("force", slice(3, 6)), ("joints", slice(6, None)))


def mass_errors(M, Mref):
    """worst |dM_ij| / sqrt(M_ii M_jj) (the diagonal from the float64 reference) over the base block, the base-joint
    block and the joint block with its diagonal"""
    d = np.sqrt(np.diag(Mref))
    E = np.abs(np.asarray(M, np.float64) - Mref) / np.outer(d, d)
    return {"base": float(E[:6, :6].max()), "base-joint": float(max(E[:6, 6:].max(), E[6:, :6].max())),
            "joint": float(E[6:, 6:].max())}


def bias_errors(h, href):
    """worst absolute error per block, and the block's largest component"""
    e = np.abs(np.asarray(h, np.float64) - href)
    return {k: (float(e[s].max()), float(np.abs(href[s]).max())) for k, s in H_BLOCKS}


def jac_errors(J, Jref):
    """worst absolute error of the linear rows and of the angular rows over [P, 6, nd], and their largest components"""
    e = np.abs(np.asarray(J, np.float64) - Jref)
    return {"linear": (float(e[:, 0:3].max()), float(np.abs(Jref[:, 0:3]).max())),
            "angular": (float(e[:, 3:6].max()), float(np.abs(Jref[:, 3:6]).max()))}


def figures(n, S, M, H, J, ref):
    """Every figure of the accuracy gate as {name: (worst error over the states, largest component or None)}: M [E, nd,
    nd], H {flags: [E, nd]}, J [E, P, 6, nd] against `ref` = references(n, S)"""
    out = {}
    for e in range(len(S)):
        for k, v in mass_errors(M[e], ref["M"][e]).items():
            key = "M " + k
            out[key] = (max(out.get(key, (0.0, None))[0], v), None)
        for f in (1, 2, 3):
            for k, (err, big) in bias_errors(H[f][e], ref["H"][f][e]).items():
                key = "h flags %d %s" % (f, k)
                old = out.get(key, (0.0, 0.0))
                out[key] = (max(old[0], err), max(old[1], big))
        for k, (err, big) in jac_errors(J[e], ref["J"][e]).items():
            key = "J " + k
            old = out.get(key, (0.0, 0.0))
            out[key] = (max(old[0], err), max(old[1], big))
    return out


_CACHE = {}


def references(n, S=None):
    """float64 reference and float32 twin of the gate's states (computed once per chain length):
    dict(S, points, M, H {1, 2, 3}, J) and the same under "twin" """
    if S is None and n in _CACHE:
        return _CACHE[n]
    states = gate_states(n) if S is None else S
    pts = gate_points(n)
    ref = dict(S=states, points=pts, M=[], H={1: [], 2: [], 3: []}, J=[])
    tw = dict(M=[], H={1: [], 2: [], 3: []}, J=[])
    for s in states:
        M, hs = reference(s, n, (1, 2, 3))
        Mt, hts, Jt = twin(s, n, (1, 2, 3), np.float32, pts)
        for f in (1, 2, 3):
            ref["H"][f].append(hs[f])
            tw["H"][f].append(hts[f])
        ref["M"].append(M)
        links, Rw, ow, J = _kin64(s, n)[:4]
        ref["J"].append(np.stack([_point_jacobian(links, Rw, J, r, l, np.dtype(np.float64)) for r, l in pts]))
        tw["M"].append(Mt)
        tw["J"].append(np.stack(Jt))
    for d in (ref, tw):
        d["M"] = np.stack(d["M"])
        d["J"] = np.stack(d["J"])
        d["H"] = {f: np.stack(v) for f, v in d["H"].items()}
    ref["twin"] = tw
    if S is None:
        _CACHE[n] = ref
    return ref
