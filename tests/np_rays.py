"""Independent numpy model of the ray test (test helper, not product code).

Written from the contract text in include/snk.h ("The ray test"), not from the kernels: the solids are np_render.scene's (the
unmerged URDF tree of tests/np_model.py, where the kernels run merged composite bodies), the ray / solid intervals
np_render._cyl_interval and _box_interval, the parent frames the link frames of the same tree as np_link_states has them
(orientation Rw, origin the COM ow + Rw c); every ray of a row one numpy array operation.  dtype=np.float64 is the model;
dtype=np.float32 runs the SAME code in float32, forward kinematics included -- the "float32 twin", the yardstick a float32
kernel is held against.

ray_test() returns the records and, apart, the id and the distance along the ray.  retained() is the contract's "is this
ray's hit decided well away from an edge": the float64 model gives the same primitive id for the ray itself, for four rays
whose `to` is displaced by +-DELTA |to - from| along two unit vectors perpendicular to it, and with the tie margin at
1.8e-4 and 2.2e-4 m.

DELTA was determined by tests/test_np_rays.py (test_float32_twin_determines_delta), as np_render.DELTA was: the smallest of
{1e-6, 1e-5, 1e-4} at which the float32 twin flips no id on retained rays over every (kind, set) of tests/ray_sets.py.
Counts of that run over the 21393 rays of all sets, "twin's flips among retained rays / rays left out / the smallest share
a set other than `degenerate` keeps":
    1e-6:  0 / 17 / 99.92 %        1e-5:  0 / 22 / 99.61 %        1e-4:  0 / 73 / 98.44 %
"""
import numpy as np

import np_model
import np_render as R

GROUND, SNAKE, BOX = 1, 2, 4            # SNK_RAYS_GROUND / _SNAKE / _BOX
ALL = GROUND | SNAKE | BOX
TIE = R.TIE
MISS = np.array([1, 0, 0, 0, 0, 0, 0, -1], np.float64)
DELTA = 1e-6


def parent_frame(n, state, parent_row, dtype=np.float64):
    """(R [3, 3] frame -> world, origin [3]) of row `parent_row` of snk_link_states, in `dtype`; -1: the world's."""
    T = dtype
    if parent_row < 0:
        return np.eye(3, dtype=T), np.zeros(3, T)
    state = np.asarray(state, T)
    links = np_model.build_tree(n)
    Rw, ow = R._fk(links, state[0:3], state[3:7], state[13:13 + n], T)
    Rl = np.asarray(Rw[parent_row], T)
    return Rl, np.asarray(ow[parent_row], T) + Rl @ links[parent_row]["c"].astype(T)


def ray_test(n, state, box, rays, parent_row=-1, flags=ALL, dtype=np.float64, tie=TIE):
    """rays [k, 6], [from 3 | to 3] in the frame of `parent_row`, on the env whose state row (snk_get_state's) and box
    (np_render.scene's argument) are given.  Returns dict(hits [k, 8] of `dtype`, id [k] int, t [k] metres along the ray
    (inf: a miss), length [k])."""
    T = dtype
    rays = np.asarray(rays, T).reshape(-1, 6)
    valid = np.isfinite(rays).all(-1)
    rays = np.where(valid[:, None], rays, T(0))
    Rp, op = parent_frame(n, state, parent_row, T)
    o = op + rays[:, 0:3] @ Rp.T
    p = op + rays[:, 3:6] @ Rp.T
    d = p - o
    tf = np.sqrt((d * d).sum(-1))
    valid &= (tf > 0) & np.isfinite(tf)
    d = d / np.where(valid, tf, T(1))[:, None]
    sc = R.scene(n, state, box, dtype=T)
    C, A = sc["C"].astype(T), sc["A"].astype(T)
    r, hl = T(sc["r"]), T(sc["hl"])
    k = len(rays)
    tbest = np.full(k, np.inf, T)
    pid = np.full(k, -1, np.int64)
    nrm = np.zeros((k, 3), T)
    nrm[:, 2] = 1
    if flags & GROUND:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -o[:, 2] / d[:, 2]
        ok = valid & (d[:, 2] != 0) & (t >= 0) & (t <= tf)
        tbest = np.where(ok, t, tbest)
        pid = np.where(ok, 0, pid)
    if flags & SNAKE:
        for c in range(len(C)):
            m = o - C[c]
            tin, _, cap, dp = R._cyl_interval(m, d, A[c], r, hl)
            ok = valid & (tin >= 0) & (tin <= tf) & (tin < tbest - T(tie))
            q = m + d * np.where(np.isfinite(tin), tin, 0).astype(T)[:, None]
            side = (q - (q @ A[c])[:, None] * A[c]) / r
            capn = np.where(dp > 0, -1.0, 1.0).astype(T)[:, None] * A[c]
            tbest = np.where(ok, tin, tbest)
            pid = np.where(ok, 1 + c, pid)
            nrm = np.where(ok[:, None], np.where(cap[:, None], capn, side), nrm)
    if (flags & BOX) and sc["box"] is not None:
        bc, bR, bh = (v.astype(T) for v in sc["box"])
        tin, _, nb = R._box_interval(o - bc, d, bR, bh)
        ok = valid & (tin >= 0) & (tin <= tf) & (tin < tbest - T(tie))
        tbest = np.where(ok, tin, tbest)
        pid = np.where(ok, 1 + len(C), pid)
        nrm = np.where(ok[:, None], nb, nrm)
    hit = pid >= 0
    th = np.where(hit, tbest, 0).astype(T)
    hits = np.empty((k, 8), T)
    hits[:, 0] = th / np.where(valid, tf, T(1))
    hits[:, 1:4] = o + d * th[:, None]
    hits[:, 4:7] = nrm
    hits[:, 7] = pid
    hits = np.where(hit[:, None], hits, MISS.astype(T))
    assert hits.dtype == np.dtype(T)
    return dict(hits=hits, id=pid, t=np.where(hit, tbest, np.inf), length=np.where(valid, tf, 0))


def _perpendiculars(d):
    """two unit vectors perpendicular to each row of d [k, 3] (float64) and to each other; any pair for a zero row"""
    n = np.linalg.norm(d, axis=-1)
    u = np.where((n > 0)[:, None], d / np.where(n > 0, n, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
    e = np.eye(3)[np.argmin(np.abs(u), axis=-1)]          # the coordinate axis the ray is least along
    a = np.cross(u, e)
    a = a / np.linalg.norm(a, axis=-1)[:, None]
    return a, np.cross(u, a)


def retained(n, state, box, rays, parent_row=-1, flags=ALL, delta=None, base=None):
    """bool [k]: the float64 model's id is the same for the ray, its four displaced neighbours and both tie margins."""
    delta = DELTA if delta is None else delta
    rays = np.asarray(rays, np.float64).reshape(-1, 6)
    fin = np.isfinite(rays).all(-1)
    safe = np.where(fin[:, None], rays, 0.0)
    ids = (base if base is not None else ray_test(n, state, box, rays, parent_row, flags))["id"]
    keep = np.ones(len(rays), bool)
    for tie in (1.8e-4, 2.2e-4):
        keep &= ray_test(n, state, box, rays, parent_row, flags, tie=tie)["id"] == ids
    d = safe[:, 3:6] - safe[:, 0:3]
    a, b = _perpendiculars(d)
    step = delta * np.linalg.norm(d, axis=-1)[:, None]
    for v in (a, -a, b, -b):
        moved = rays.copy()
        moved[:, 3:6] = np.where(fin[:, None], safe[:, 3:6] + step * v, rays[:, 3:6])
        keep &= ray_test(n, state, box, moved, parent_row, flags)["id"] == ids
    return keep


def errors(hits, ref, mask=None):
    """The three figures of the gates for the rays (of `mask`) that the float64 model `ref` (ray_test's dict) hits:
    (distance along the ray [m], position [m], angle between the normals [rad]), `hits` being anyone's records [..., 8]."""
    h = np.asarray(hits, np.float64)
    on = (ref["id"] >= 0) if mask is None else (ref["id"] >= 0) & mask
    g, w = h[on], np.asarray(ref["hits"], np.float64)[on]
    dist = np.abs(g[:, 0] * ref["length"][on] - ref["t"][on])
    pos = np.linalg.norm(g[:, 1:4] - w[:, 1:4], axis=-1)
    ang = np.arctan2(np.linalg.norm(np.cross(g[:, 4:7], w[:, 4:7]), axis=-1), (g[:, 4:7] * w[:, 4:7]).sum(-1))
    return dist, pos, ang
