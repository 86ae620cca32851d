"""Independent numpy model of the rendered scene (test helper, not product code).

Written from the contract text in include/snk.h ("The rendered scene"), not from the kernels: link frames from
tests/np_model.py (build_tree, fk: the unmerged URDF tree, where the kernels run merged composite bodies), cylinder
dimensions from the URDF numbers, every pixel as a numpy array operation.  dtype=np.float64 is the model; dtype=np.float32
runs the SAME code in float32 -- the "float32 twin", the yardstick a float32 kernel is held against, as the float32 build
of the oracle is for the physics.

render() returns, per pixel: rgba (uint8), depth, seg (primitive id), and the three facts the retention mask is made of:
the id, the checker parity (ground hits), the lit flag.  retention_mask() is the contract's "is this pixel's structure
decided well away from an edge": the float64 model gives the same id, parity and lit flag at the pixel centre and at four
rays displaced by +-delta pixel in i and in j.
"""
import numpy as np

import np_model

R_CYL = 0.026               # snake.urdf:806-811, 862-867 (snk_params_derived reports the same: test_np_render.py)
HL_CYL = 0.033 / 2
TIE = 2e-4                  # a later primitive replaces the kept hit only when nearer by more than this [m]
SHADOW_OFFSET = 1e-4
LIGHT = np.array([0.4, -0.3, 0.85]) / np.sqrt(0.4 ** 2 + 0.3 ** 2 + 0.85 ** 2)
ALB_GROUND = np.array([[0.95, 0.95, 0.95], [0.55, 0.65, 0.85]])
ALB_CYL = np.array([[0.85, 0.35, 0.15], [0.25, 0.25, 0.28]])
ALB_BOX = np.array([0.45, 0.75, 0.45])
BACKGROUND = np.array([200, 215, 235, 255], np.uint8)
DELTA = 1e-3                # the retention mask's displacement in pixels (determined and asserted in test_np_render.py)


# ---- cameras (PyBullet's two helpers, from its documentation and bullet3's formulas) ----
def view_matrix_ypr(target, distance, yaw, pitch, roll=0.0, up_axis=2):
    """computeViewMatrixFromYawPitchRoll as a column-major 16-vector (roll is ignored, as bullet3 does)."""
    yaw, pitch = np.deg2rad(yaw), np.deg2rad(pitch)

    def rx(a):
        return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])

    def ry(a):
        return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])

    def rz(a):
        return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    if up_axis == 2:
        R, eye0, up0 = rz(yaw) @ rx(pitch), np.array([0.0, -distance, 0.0]), np.array([0.0, 0.0, 1.0])
    else:
        R, eye0, up0 = ry(yaw) @ rx(-pitch), np.array([0.0, 0.0, -distance]), np.array([0.0, 1.0, 0.0])
    target = np.asarray(target, float)
    return look_at(R @ eye0 + target, target, R @ up0)


def look_at(eye, target, up):
    eye, target, up = (np.asarray(v, float) for v in (eye, target, up))
    f = target - eye
    f = f / np.linalg.norm(f)
    s = np.cross(f, up / np.linalg.norm(up))
    s = s / np.linalg.norm(s)
    u = np.cross(s, f)
    V = np.eye(4)
    V[0, :3], V[1, :3], V[2, :3] = s, u, -f
    V[:3, 3] = [-s @ eye, -u @ eye, f @ eye]
    return V.T.reshape(16).copy()          # column-major


def projection_fov(fov, aspect, near, far):
    y = 1.0 / np.tan(np.deg2rad(fov) / 2.0)
    P = np.zeros((4, 4))
    with np.errstate(divide="ignore", invalid="ignore"):
        P[0, 0], P[1, 1] = y / aspect, y
        P[2, 2] = np.float64(near + far) / np.float64(near - far)
        P[2, 3] = np.float64(2.0 * far * near) / np.float64(near - far)
    P[3, 2] = -1.0
    return P.T.reshape(16).copy()


def eye_distance(depth, near, far):
    """PyBullet's documented inversion of the depth buffer: distance along the view axis."""
    depth = np.asarray(depth, np.float64)
    return far * near / (far - (far - near) * depth)


# ---- the scene of one environment ----
def _fk(links, pos, quat, q, T):
    """np_model.fk, in dtype T: the float64 model calls np_model.fk itself; the float32 twin needs the same recurrence with
    every product rounded to float32, as a float32 kernel's forward kinematics is."""
    if T == np.float64:
        return np_model.fk(links, pos, quat, q)
    x, y, z, w = (np.asarray(quat, T) / np.sqrt((np.asarray(quat, T) ** 2).sum())).astype(T)
    one, two = T(1), T(2)
    Rw = [np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                    [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                    [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], T)]
    ow = [np.asarray(pos, T)]
    for i in range(1, len(links)):
        k = links[i]
        R = k["R"].astype(T)
        if k["rev"]:
            c, s = np.cos(T(q[k["dof"]])), np.sin(T(q[k["dof"]]))
            R = R @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], T)
        Rw.append(Rw[k["parent"]] @ R)
        ow.append(ow[k["parent"]] + Rw[k["parent"]] @ k["p"].astype(T))
    return Rw, ow


def scene(n, state, box=None, dtype=np.float64):
    """state: [pos3, quat xyzw 4, ..., q n at 13:13+n] (snk_get_state's row).  box: None, or (centre 3, quat xyzw 4 or None
    for axis aligned, half extents 3).  Arrays of `dtype`, computed in it: cylinder centres [2n, 3], unit axes [2n, 3]."""
    T = dtype
    state = np.asarray(state, T)
    links = np_model.build_tree(n)
    Rw, ow = _fk(links, state[0:3], state[3:7], state[13:13 + n], T)
    C, A = [], []
    for i, k in enumerate(links):
        if "cyl" in k:
            C.append(ow[i] + Rw[i] @ k["cyl"].astype(T))
            A.append(Rw[i][:, 2])
    sc = dict(n=n, C=np.array(C, T), A=np.array(A, T), r=R_CYL, hl=HL_CYL, box=None)
    if box is not None:
        c, q, h = box
        R = np.eye(3) if q is None else np_model.quat_to_mat(np.asarray(q, np.float64))
        sc["box"] = (np.asarray(c, np.float64), R, np.asarray(h, np.float64))
    return sc


# ---- ray against solid: the interval [tin, tout] inside, miss = (inf, -inf) ----
def _cyl_interval(m, d, A, r, hl):
    """m = o - centre [..., 3], d [..., 3], A [3].  Returns tin, tout, cap (entry through a cap), dp = d.A."""
    dp = d @ A
    mp = m @ A
    dq = d - dp[..., None] * A
    mq = m - mp[..., None] * A
    a = (dq * dq).sum(-1)
    b = (mq * dq).sum(-1)
    c = (mq * mq).sum(-1) - r * r
    inf = np.array(np.inf, m.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        disc = b * b - a * c
        sq = np.sqrt(np.where(disc >= 0, disc, 0))
        para = ~(a > 0)
        s_in = np.where(para, -inf, (-b - sq) / a)
        s_out = np.where(para, inf, (-b + sq) / a)
        miss = np.where(para, c > 0, ~(disc >= 0))
        t1 = (-hl - mp) / dp
        t2 = (hl - mp) / dp
        flat = dp == 0
        c_in = np.where(flat, -inf, np.minimum(t1, t2))
        c_out = np.where(flat, inf, np.maximum(t1, t2))
        miss = miss | (flat & ~(np.abs(mp) <= hl))
    cap = c_in > s_in
    tin = np.where(cap, c_in, s_in)
    tout = np.minimum(s_out, c_out)
    miss = miss | ~(tin <= tout)
    return np.where(miss, inf, tin), np.where(miss, -inf, tout), cap, dp


def _box_interval(m, d, R, h):
    """Returns tin, tout, normal [..., 3] of the face the ray enters through."""
    inf = np.array(np.inf, m.dtype)
    tin = np.full(m.shape[:-1], -np.inf, m.dtype)
    tout = np.full(m.shape[:-1], np.inf, m.dtype)
    nrm = np.zeros(m.shape, m.dtype)
    miss = np.zeros(m.shape[:-1], bool)
    for k in range(3):
        ak = R[:, k]
        ok, dk = m @ ak, d @ ak
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (-h[k] - ok) / dk, (h[k] - ok) / dk
        flat = dk == 0
        lo = np.where(flat, -inf, np.minimum(t1, t2))
        hi = np.where(flat, inf, np.maximum(t1, t2))
        miss |= flat & ~(np.abs(ok) <= h[k])
        later = lo > tin
        tin = np.where(later, lo, tin)
        sign = np.where(dk > 0, -1.0, 1.0).astype(m.dtype)
        nrm = np.where(later[..., None], sign[..., None] * ak, nrm)
        tout = np.minimum(tout, hi)
    miss |= ~(tin <= tout)
    return np.where(miss, inf, tin), np.where(miss, -inf, tout), nrm


def render(sc, view, proj, width, height, shadow=False, dtype=np.float64, di=0.0, dj=0.0):
    """One image of scene `sc`.  view / proj: column-major 16-vectors.  di, dj: displacement of every sample from its
    pixel centre, in pixels (the retention mask's rays).  Returns a dict of [height, width] arrays."""
    T = dtype
    V = np.asarray(view, np.float64).reshape(4, 4).T
    P = np.asarray(proj, np.float64).reshape(4, 4).T
    M64 = P @ V
    Minv = np.linalg.inv(M64).astype(T)            # the contract: inverted in float64, then rounded
    M = M64.astype(T)
    C, A = sc["C"].astype(T), sc["A"].astype(T)
    r, hl = T(sc["r"]), T(sc["hl"])
    L = LIGHT.astype(T)
    i = (np.arange(width, dtype=T) + T(0.5) + T(di))[None, :]
    j = (np.arange(height, dtype=T) + T(0.5) + T(dj))[:, None]
    x = np.broadcast_to(T(2) * i / T(width) - T(1), (height, width))
    y = np.broadcast_to(T(1) - T(2) * j / T(height), (height, width))
    one = np.ones((height, width), T)
    a = np.stack([x, y, -one, one], -1) @ Minv.T
    b = np.stack([x, y, one, one], -1) @ Minv.T
    o = a[..., :3] / a[..., 3:]
    f = b[..., :3] / b[..., 3:]
    d = f - o
    tf = np.sqrt((d * d).sum(-1))
    d = d / tf[..., None]

    inf = np.array(np.inf, T)
    tbest = np.full((height, width), np.inf, T)
    seg = np.full((height, width), -1, np.int32)
    nrm = np.zeros((height, width, 3), T)
    nrm[..., 2] = 1
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -o[..., 2] / d[..., 2]
    ok = (d[..., 2] != 0) & (t >= 0) & (t <= tf)
    tbest = np.where(ok, t, tbest)
    seg = np.where(ok, 0, seg)
    for c in range(len(C)):
        m = o - C[c]
        tin, _, cap, dp = _cyl_interval(m, d, A[c], r, hl)
        ok = (tin >= 0) & (tin <= tf) & (tin < tbest - T(TIE))
        q = m + d * np.where(np.isfinite(tin), tin, 0)[..., None]
        side = (q - (q @ A[c])[..., None] * A[c]) / r
        capn = np.where(dp > 0, -1.0, 1.0).astype(T)[..., None] * A[c]
        nc = np.where(cap[..., None], capn, side)
        tbest = np.where(ok, tin, tbest)
        seg = np.where(ok, 1 + c, seg)
        nrm = np.where(ok[..., None], nc, nrm)
    if sc["box"] is not None:
        bc, bR, bh = (v.astype(T) for v in sc["box"])
        tin, _, nb = _box_interval(o - bc, d, bR, bh)
        ok = (tin >= 0) & (tin <= tf) & (tin < tbest - T(TIE))
        tbest = np.where(ok, tin, tbest)
        seg = np.where(ok, 1 + len(C), seg)
        nrm = np.where(ok[..., None], nb, nrm)

    hit = seg >= 0
    X = o + d * np.where(hit, tbest, 0)[..., None]
    parity = ((np.floor(X[..., 0] / T(0.5)).astype(np.int64) + np.floor(X[..., 1] / T(0.5)).astype(np.int64)) & 1).astype(np.int32)
    parity = np.where(seg == 0, parity, 0)
    alb = np.zeros((height, width, 3), T)
    alb = np.where((seg == 0)[..., None], ALB_GROUND.astype(T)[parity], alb)
    iscyl = (seg >= 1) & (seg <= len(C))
    alb = np.where(iscyl[..., None], ALB_CYL.astype(T)[(seg - 1) & 1], alb)
    alb = np.where((seg == 1 + len(C))[..., None], ALB_BOX.astype(T), alb)
    ndl = np.maximum(T(0), nrm @ L)
    lit = np.ones((height, width), np.int32)
    if shadow:
        so = X + nrm * T(SHADOW_OFFSET)
        Ld = np.broadcast_to(L, so.shape)
        occ = np.zeros((height, width), bool)
        for c in range(len(C)):
            tin, tout, _, _ = _cyl_interval(so - C[c], Ld, A[c], r, hl)
            occ |= (tin <= tout) & (tout >= 0)
        if sc["box"] is not None:
            tin, tout, _ = _box_interval(so - bc, Ld, bR, bh)
            occ |= (tin <= tout) & (tout >= 0)
        lit = np.where((ndl > 0) & ~occ, 1, 0).astype(np.int32)
    lit = np.where(hit, lit, 1)
    k = T(0.4) + T(0.6) * ndl * lit.astype(T)
    col = np.floor(T(255) * (alb * k[..., None]) + T(0.5)).astype(np.uint8)
    rgba = np.empty((height, width, 4), np.uint8)
    rgba[..., :3] = col
    rgba[..., 3] = 255
    rgba = np.where(hit[..., None], rgba, BACKGROUND)
    Xh = np.concatenate([X, np.ones((height, width, 1), T)], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = T(0.5) * ((Xh @ M[2]) / (Xh @ M[3])) + T(0.5)
    depth = np.where(hit, depth, T(1)).astype(T)
    return dict(rgba=rgba, depth=depth, seg=seg.astype(np.int32), parity=parity, lit=lit, ndl=ndl, t=np.where(hit, tbest, inf))


def structure(img):
    """The three facts of a pixel the retention mask compares, as one integer array."""
    return img["seg"].astype(np.int64) * 4 + img["parity"] * 2 + img["lit"]


def retention_mask(sc, view, proj, width, height, shadow=False, delta=DELTA, centre=None):
    """True where the float64 model gives the same primitive id, checker parity and lit flag at the pixel centre and at
    the four rays displaced by +-delta pixel in i and in j."""
    base = structure(centre if centre is not None else render(sc, view, proj, width, height, shadow))
    keep = np.ones((height, width), bool)
    for di, dj in ((delta, 0), (-delta, 0), (0, delta), (0, -delta)):
        keep &= structure(render(sc, view, proj, width, height, shadow, di=di, dj=dj)) == base
    return keep
