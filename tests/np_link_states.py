"""Link states of the unmerged URDF tree from tests/np_model.py (test helper, not product code): what snk_link_states
returns -- per link [COM 3 | quaternion xyzw 4 | link-frame origin 3 | COM velocity 3 | angular velocity 3], row r = Bullet
link r - 1 -- from the independent model's own formulas:

    COM = ow + Rw c,  orientation = Rw,  origin = ow,  v = Jv gvel,  w = Jw gvel     (np_model.fk, np_model.link_jacobians)

reference(state)   float64, by np_model's functions themselves, on the float32 state the GPU was handed
twin(state)        the SAME formulas restated with every constant, intermediate and result in float32: the yardstick of the
                   float32 gate (conftest.f32_gate) -- what float32 arithmetic over the 3n + 2-link tree costs, measured,
                   not the kernel.  twin(state, np.float64) must reproduce reference(state) exactly (the CPU test holds
                   the restatement to that).
"""
import numpy as np

import np_model as npm


def quat_of(R):
    """xyzw quaternion of a rotation matrix (link -> world), w >= 0, in R's dtype: the branch of the largest of (trace,
    m00, m11, m22), then normalised."""
    dt = R.dtype.type
    one = dt(1)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    k = int(np.argmax([tr, R[0, 0], R[1, 1], R[2, 2]]))
    if k == 0:
        q = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], one + tr]
    elif k == 1:
        q = [one + R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0], R[2, 1] - R[1, 2]]
    elif k == 2:
        q = [R[0, 1] + R[1, 0], one - R[0, 0] + R[1, 1] - R[2, 2], R[1, 2] + R[2, 1], R[0, 2] - R[2, 0]]
    else:
        q = [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], one - R[0, 0] - R[1, 1] + R[2, 2], R[1, 0] - R[0, 1]]
    q = np.array(q, dtype=R.dtype)
    q = q / np.sqrt(q.dot(q))
    return -q if q[3] < 0 else q


def _pack(links, Rw, ow, J, gvel, dtype):
    out = np.zeros((len(links), 16), dtype)
    for i in range(len(links)):
        Jw, Jv, cw = J[i]
        out[i, 0:3] = cw
        out[i, 3:7] = quat_of(np.asarray(Rw[i], dtype))
        out[i, 7:10] = ow[i]
        out[i, 10:13] = Jv @ gvel
        out[i, 13:16] = Jw @ gvel
    return out


def split_state(state, n):
    """(pos, quat, gvel = [omega_w, v_w(root origin), qd], q) of a state row [pos3 quat4 omega3 vel3 q qd]."""
    s = np.asarray(state)
    return s[0:3], s[3:7], np.concatenate([s[7:13], s[13 + n:13 + 2 * n]]), s[13:13 + n]


def reference(state, n):
    """[3n + 2, 16] float64 by np_model.fk and np_model.link_jacobians."""
    links = npm.build_tree(n)
    pos, quat, gvel, q = split_state(np.asarray(state, np.float64), n)
    Rw, ow = npm.fk(links, pos, quat, q)
    return _pack(links, Rw, ow, npm.link_jacobians(links, Rw, ow), gvel, np.float64)


def _cast_tree(n, dtype):
    links = npm.build_tree(n)
    return [dict(k, R=k["R"].astype(dtype), p=k["p"].astype(dtype), c=k["c"].astype(dtype)) for k in links]


def twin(state, n, dtype=np.float32):
    """The same in `dtype` throughout: np_model.quat_to_mat, rot_y, fk and link_jacobians restated line by line."""
    dt = np.dtype(dtype).type
    links = _cast_tree(n, dtype)
    pos, quat, gvel, q = (np.asarray(a, dtype) for a in split_state(state, n))
    # np_model.quat_to_mat
    x, y, z, w = quat / np.linalg.norm(quat)
    one, two = dt(1), dt(2)
    R0 = np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                   [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                   [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=dtype)

    def rot_y(a):
        c, s = np.cos(a), np.sin(a)          # (numpy keeps a float32 scalar's dtype)
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=dtype)

    # np_model.fk
    Rw, ow = [R0], [pos]
    for i in range(1, len(links)):
        k = links[i]
        R = k["R"] @ rot_y(q[k["dof"]]) if k["rev"] else k["R"]
        Rw.append(Rw[k["parent"]] @ R)
        ow.append(ow[k["parent"]] + Rw[k["parent"]] @ k["p"])
    # np_model.link_jacobians
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
    out = _pack(links, Rw, ow, J, gvel, dtype)
    assert out.dtype == np.dtype(dtype) and all(m.dtype == np.dtype(dtype) for m in Rw)
    return out


def errors(got, ref, gvel):
    """The five figures the gate compares, as worst values over the links of one env, `ref` float64:
    COM [m], origin [m], orientation 1 - |q . q'|, COM velocity and angular velocity relative to the largest component
    of the generalised velocity."""
    g = np.asarray(got, np.float64)
    scale = float(np.max(np.abs(gvel)))
    qd = np.abs(np.sum(g[:, 3:7] * ref[:, 3:7], axis=1))
    return dict(com=float(np.max(np.linalg.norm(g[:, 0:3] - ref[:, 0:3], axis=1))),
                origin=float(np.max(np.linalg.norm(g[:, 7:10] - ref[:, 7:10], axis=1))),
                quat=float(np.max(1.0 - qd)),
                vel=float(np.max(np.linalg.norm(g[:, 10:13] - ref[:, 10:13], axis=1))) / scale,
                omega=float(np.max(np.linalg.norm(g[:, 13:16] - ref[:, 13:16], axis=1))) / scale)
