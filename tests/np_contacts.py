"""The reported contacts (include/snk.h, "The reported contacts": snk_contacts) from tests/np_model.py -- a test helper, not
product code, written from the header's text and not from the kernel:

    slot 4 c + j = cached point j of cylinder c (link order), the last four the free box's;
    a slot = [point on the body 3 | point on the ground 3 | normal 3 | distance | force N | impulse | c | j | live | 0]
    point on cylinder c = centre_c + Rw_c (a - (0, 0, cyl_zoff)),  centre_c = ow + Rw (0, 0, cyl_zoff)  on the cylinder's
                          LINK frame (Rw, ow) of np_model's unmerged tree (a cylinder's frame is its link's, its centre
                          cyl_zoff along the link's z: snake.urdf:806-811, 862-867)
    point on the box    = pos + R(quat) a

reference(state, manifold, box, params)   float64, link frames by np_model.fk itself
twin(...)                                  the SAME formulas with every constant, intermediate and result in float32: the
                                           yardstick of the float32 gate (conftest.f32_gate), not the kernel.
                                           twin(..., dtype=np.float64) must reproduce reference(...) exactly.

state [13 + 2n] = [pos3 quat4 omega3 vel3 q qd]; manifold [2n, 29] = per cylinder [count, 4 x (a3, b3, impulse)]
(snk_get_manifold's layout); box = None or (state [13], manifold [29]) (snk_get_box's); params = dict(n=, dt=, cyl_zoff=):
dt the time step AS THE HANDLE HOLDS IT (float32(dt) for a GPU handle), cyl_zoff = snk_params_derived's out[3].
Returns (points [slots, 16], force [2n + 1], count)."""
import numpy as np

import np_model as npm

FLOATS = 16


def cylinder_links(n):
    """Indices into np_model.build_tree(n) of the links that carry a collision cylinder, in link order; index - 1 is the
    Bullet link index."""
    return [i for i, k in enumerate(npm.build_tree(n)) if "cyl" in k]


def _fk(n, pos, quat, q, dtype):
    """np_model.quat_to_mat, rot_y and fk restated in `dtype` (float64: np_model.fk itself)."""
    if np.dtype(dtype) == np.float64:
        return npm.fk(npm.build_tree(n), pos, quat, q)
    dt = np.dtype(dtype).type
    links = [dict(k, R=k["R"].astype(dtype), p=k["p"].astype(dtype)) for k in npm.build_tree(n)]
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
    assert all(m.dtype == np.dtype(dtype) for m in Rw)
    return Rw, ow


def _slots(out, first, c, count, cache, R, origin, off, dt, dtype):
    """The four slots of one unit (cylinder c, or the box: c = 2n) into out[first : first + 4]; returns (force, live)."""
    t = np.dtype(dtype).type
    live = int(min(max(int(count), 0), 4))
    force = t(0)
    for j in range(live):
        a, b, lam = cache[7 * j:7 * j + 3], cache[7 * j + 3:7 * j + 6], cache[7 * j + 6]
        w = origin + R @ (a - off)
        row = out[first + j]
        row[0:3] = w
        row[3:6] = [b[0], b[1], 0]
        row[6:9] = [0, 0, 1]
        row[9] = row[2] - row[5]
        row[10] = lam / dt
        row[11] = lam
        row[12], row[13], row[14] = c, j, 1
        force = force + row[10]
    return force, live


def twin(state, manifold, box, params, dtype=np.float32):
    n = int(params["n"])
    t = np.dtype(dtype).type
    s = np.asarray(state, dtype)
    M = np.asarray(manifold, dtype)
    dt, zoff = t(params["dt"]), np.array([0, 0, params["cyl_zoff"]], dtype=dtype)
    Rw, ow = _fk(n, s[0:3], s[3:7], s[13:13 + n], dtype)
    slots = 8 * n + (4 if box is not None else 0)
    out = np.zeros((slots, FLOATS), dtype)
    force = np.zeros(2 * n + 1, dtype)
    count = 0
    for c, i in enumerate(cylinder_links(n)):
        R = np.asarray(Rw[i], dtype)
        centre = np.asarray(ow[i], dtype) + R @ zoff
        force[c], live = _slots(out, 4 * c, c, M[c, 0], M[c, 1:], R, centre, zoff, dt, dtype)
        count += live
    if box is not None:
        bs, bm = np.asarray(box[0], dtype), np.asarray(box[1], dtype)
        R = _fk(n, bs[0:3], bs[3:7], s[13:13 + n], dtype)[0][0]        # (the root's frame: R(quat))
        force[2 * n], live = _slots(out, 8 * n, 2 * n, bm[0], bm[1:], np.asarray(R, dtype), bs[0:3], np.zeros(3, dtype), dt,
                                    dtype)
        count += live
    assert out.dtype == np.dtype(dtype) and force.dtype == np.dtype(dtype)
    return out, force, count


def reference(state, manifold, box, params):
    return twin(state, manifold, box, params, dtype=np.float64)
