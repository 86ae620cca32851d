"""The ground-contact cache update in plain float64 numpy (test helper, not product code).

An independent restatement of what one substep does to the persistent contact manifold of a (plane, link cylinder) pair
and of the (plane, free box) pair, written from the rules as DESIGN.md 3 and the comments of include/snk.h state them
and from Bullet's published algorithm names, on top of np_model.fk and the `cyl` entries of np_model.build_tree:

* refreshContactPoints: every cached point's world position on the body from the new pose, its distance along the
  plane's normal; then from the LAST point to the first: remove it when the distance is above the threshold, or when
  the point on the plane drifted from the projection of the point on the body by more than the threshold; a removed
  point's place is taken by the last one;
* the convex-plane algorithm's one new point: the support vertex of the shape towards the plane (32-gon prism: 64
  vertices, (+z, -z) per rim vertex, first maximum; btCylinderShapeZ's support function for the implicit cylinder;
  both plus the margin along the direction; the box: its nominal corner, `>= 0` per axis), accepted when its distance
  is below the threshold;
* getCacheEntry: the nearest cached point (body coordinates) closer than the threshold, first minimum ->
  replaceContactPoint (the applied impulse stays); else addManifoldPoint: appended while fewer than four are held,
  otherwise sortCachedPoints in its three-point area form picks the one to overwrite (impulse 0).

The threshold is recomputed here from the URDF numbers (`link_threshold`, `box_threshold`).

Every decision is returned with its MARGIN: how far the compared quantity was from its threshold or from the
runner-up, as a length (or area, or direction cosine) relative to the scale of the coordinates that entered it.  A
float32 computation tips a decision whose margin is at round-off: tests leave a case out of the STRUCTURAL comparison
when its smallest margin is below MARGIN_BOUND, and assert that this happens to at most MAX_LEFT_OUT of a family.

MARGIN_BOUND is the smallest power of ten at which the float64 and the float32 oracle both agree with this model on
counts and slot order of every retained case of every family of tests/test_np_manifold.py (measured there, on the CPU):
  bound 1e-7: no retained case disagrees, float64 or float32 oracle, twelve link families (3 switch sets x 16 / 32
  links x synthesised / trajectory, 2048 + 15360 cylinder cases each), two box families (192 cases each);
  left-out shares 0.00 % ... 0.05 % of a family's cylinder cases, 0 % of the box cases;
  at 1e-8 the float32 oracle disagrees on one retained case (hull+manifold@0.02, 32 links, synthesised);
  for scale: 1e-4 would leave out 0.2 % ... 8.2 %, 1e-5 0.0 % ... 0.8 %, 1e-6 0.0 % ... 0.15 %.

The case generators of tests/test_np_manifold.py and tests/test_gpu_np_manifold.py live here too.
"""
import functools

import numpy as np

import np_model

CYL_R, CYL_HL = 0.026, 0.033 / 2           # snake.urdf's <cylinder radius length>
MARGIN_BOUND = 1e-7
MAX_LEFT_OUT = 0.10
# The float32 oracle's distance to this model (cached a, b; m), (median, worst): the MAXIMUM over the families of a chain
# length (3 switch sets x synthesised / trajectory) and over the box's two switch sets.  tests/test_gpu_np_manifold.py
# uses them as the floors of its gates; tests/test_np_manifold.py measures them and fails when they go stale.
F32_FLOOR = {16: (3.8e-8, 5.1e-7), 32: (8.7e-8, 1.1e-6), "box": (3.8e-8, 1.2e-7)}


# ----------------------------------------------------------------------------------------------------------------------
# thresholds and shapes
# ----------------------------------------------------------------------------------------------------------------------
def link_threshold(p):
    """breaking_threshold, or with relative_breaking_threshold: x the link collider's angular-motion disc = distance
    of the cylinder's centre from the link frame + half diagonal of its AABB (margin included)."""
    if not int(p.relative_breaking_threshold):
        return float(p.breaking_threshold)
    links, cyl = _tree(int(p.n_modules))
    half = np.array([CYL_R, CYL_R, CYL_HL]) + float(p.collision_margin)       # the cylinder's AABB in its own frame
    return float(p.breaking_threshold) * float(np.linalg.norm(links[cyl[0]]["cyl"]) + np.linalg.norm(half))


def box_threshold(p):
    if not int(p.relative_breaking_threshold):
        return float(p.breaking_threshold)
    return float(p.breaking_threshold) * float(np.linalg.norm(np.array(p.obstacle_half[:], float)))


@functools.lru_cache(maxsize=None)
def hull_vertices(sides):
    """The prism's vertices in the importer's order: rim vertex s at angle 2 pi s / sides from +y towards +x, its +z
    copy, then its -z copy."""
    v = []
    for s in range(sides):
        th = 2.0 * np.pi * s / sides
        for z in (CYL_HL, -CYL_HL):
            v.append([CYL_R * np.sin(th), CYL_R * np.cos(th), z])
    return np.array(v)


def _first_max(vals):
    """(index of the first maximum, its lead over the runner-up)."""
    best = 0
    for i in range(1, len(vals)):
        if vals[i] > vals[best]:
            best = i
    second = max((vals[i] for i in range(len(vals)) if i != best), default=-np.inf)
    return best, vals[best] - second


def cylinder_support(p, dl):
    """Support point of the link's collision shape along the unit direction dl (cylinder frame, centred) with the
    margin added, and the margins of the decisions it took."""
    m = float(p.collision_margin)
    sides = int(p.hull_sides)
    dec = []
    if sides > 0:
        V = hull_vertices(sides)
        k, lead = _first_max([float(dl @ v) for v in V])
        dec.append(("support", lead / np.linalg.norm(V[0])))
        sv = V[k].copy()
    else:
        rr = np.hypot(dl[0], dl[1])
        dec.append(("support", abs(dl[2])))               # which end cap
        dec.append(("support", rr))                       # the axis pointing straight down
        sv = np.array([CYL_R * dl[0] / rr, CYL_R * dl[1] / rr, 0.0]) if rr != 0 else np.array([CYL_R, 0.0, 0.0])
        sv[2] = -CYL_HL if dl[2] < 0 else CYL_HL
    return sv + m * dl, dec


def box_support(p, dl):
    h = np.array(p.obstacle_half[:], float)
    sv = np.where(dl >= 0, h, -h)
    return sv, [("support", abs(float(x))) for x in dl]


# ----------------------------------------------------------------------------------------------------------------------
# one manifold
# ----------------------------------------------------------------------------------------------------------------------
def _area(a1, a0, b1, b0):
    c = np.cross(a1 - a0, b1 - b0)
    return float(c @ c)


def sort_cached_points(pts, new):
    """Which of four cached points the new one overwrites: the deepest of the five is never given up (the new point
    itself when it is the deepest); of the others, the one whose removal leaves the largest area spanned by the new
    point and the remaining three, in the three-point form; first maximum.
    Returns (index, deepest index or -1 for the new point, index without the exception, margins)."""
    depth = [new["d"]] + [q["d"] for q in pts]
    deepest = 0
    for i in range(1, 5):
        if depth[i] < depth[deepest]:
            deepest = i
    lead_d = min(depth[i] for i in range(5) if i != deepest) - depth[deepest]
    a = [q["a"] for q in pts]
    n = new["a"]
    pair = [((n, a[1]), (a[3], a[2])), ((n, a[0]), (a[3], a[2])), ((n, a[0]), (a[3], a[1])), ((n, a[0]), (a[2], a[1]))]
    full = [_area(u[0], u[1], v[0], v[1]) for u, v in pair]
    res = [0.0 if i == deepest - 1 else full[i] for i in range(4)]
    scale = max((u[0] - u[1]) @ (u[0] - u[1]) * ((v[0] - v[1]) @ (v[0] - v[1])) for u, v in pair)
    k, lead = _first_max(res)
    k0, _ = _first_max(full)
    return k, deepest - 1, k0, [("deepest", lead_d), ("area", lead / scale if scale > 0 else 0.0)]


def update_manifold(cache, R, o, thr, a_new, support_dec):
    """One update of a 29-float cache [count, 4 x (a body coordinates 3, b world 3, lam)] for the body frame (R, o)
    and the new support point a_new (body coordinates).  The plane is z = 0, normal +z.
    Returns dict(cache, points = [(world point on the body, distance, lam0)] in slot order, margin, events)."""
    nrm = np.array([0.0, 0.0, 1.0])
    n0 = min(max(int(cache[0]), 0), 4)
    pts = [dict(a=np.array(cache[1 + 7 * j:4 + 7 * j], float), b=np.array(cache[4 + 7 * j:7 + 7 * j], float),
                lam=float(cache[7 + 7 * j])) for j in range(n0)]
    w_new = o + R @ a_new
    scale_w = max(np.abs(w_new).max(), np.abs(o).max(), CYL_R)
    scale_b = max(np.abs(a_new).max(), CYL_R)
    dec = [(k, v, 1.0) for k, v in support_dec]
    ev = dict(drops=[], action="none", evict=-1, deepest=-2, unprotected=-1, n0=n0)
    for q in pts:                                                   # refreshContactPoints, first loop
        q["w"] = o + R @ q["a"]
        q["d"] = float((q["w"] - q["b"]) @ nrm)
    for j in range(len(pts) - 1, -1, -1):                           # second loop, last to first
        q = pts[j]
        lift = q["d"] - thr
        drift = np.linalg.norm(q["b"] - (q["w"] - nrm * q["d"]))
        if q["d"] > thr or drift * drift > thr * thr:
            dec.append(("drop", max(lift, drift - thr), scale_w))
            ev["drops"].append((j, len(pts)))
            last = pts.pop()
            if j < len(pts):
                pts[j] = last
        else:
            dec.append(("keep", min(-lift, thr - drift), scale_w))
    new = dict(a=np.array(a_new, float), w=w_new, d=float(w_new[2]), b=np.array([w_new[0], w_new[1], 0.0]), lam=0.0)
    dec.append(("accept", abs(new["d"] - thr), scale_w))
    if new["d"] < thr:
        dist = [np.linalg.norm(q["a"] - new["a"]) for q in pts]
        nearest = -1
        shortest = thr * thr
        for j, dd in enumerate(dist):                               # getCacheEntry
            if dd * dd < shortest:
                shortest = dd * dd
                nearest = j
        if nearest >= 0:
            others = [dd for j, dd in enumerate(dist) if j != nearest]
            dec.append(("nearest", min([thr - dist[nearest]] + [dd - dist[nearest] for dd in others]), scale_b))
            new["lam"] = pts[nearest]["lam"]                       # replaceContactPoint keeps the applied impulse
            pts[nearest] = new
            ev["action"] = "replace"
        else:
            if dist:
                dec.append(("nearest", min(dd - thr for dd in dist), scale_b))
            if len(pts) < 4:
                pts.append(new)
                ev["action"] = "append"
            else:
                k, deepest, k0, d2 = sort_cached_points(pts, new)
                dec.append(("deepest", d2[0][1], scale_w))
                dec.append(("area", d2[1][1], 1.0))
                pts[k] = new
                ev.update(action="evict", evict=k, deepest=deepest, unprotected=k0)
    out = np.zeros(29)
    out[0] = len(pts)
    for j, q in enumerate(pts):
        out[1 + 7 * j:4 + 7 * j] = q["a"]
        out[4 + 7 * j:7 + 7 * j] = q["b"]
        out[7 + 7 * j] = q["lam"]
    margin = min(abs(v) / s for _, v, s in dec)
    return dict(cache=out, points=[(q["w"], q["d"], q["lam"]) for q in pts], margin=margin, events=ev, decisions=dec)


# ----------------------------------------------------------------------------------------------------------------------
# the two collider kinds
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tree(n):
    links = np_model.build_tree(n)
    return links, [i for i, k in enumerate(links) if "cyl" in k]


def cylinder_frames(n, s):
    """[(link index, world rotation, world origin of the LINK frame, world centre of the cylinder)] in link order."""
    links, cyl = _tree(n)
    s = np.asarray(s, float)
    Rw, ow = np_model.fk(links, s[0:3], s[3:7], s[13:13 + n])
    return [(i, Rw[i], ow[i], ow[i] + Rw[i] @ links[i]["cyl"]) for i in cyl]


def update_link_cylinder(p, R, o, zoff, cache):
    """The (plane, link) manifold: R, o the link's world frame (np_model.fk), zoff the cylinder's centre in it."""
    dl = R.T @ np.array([0.0, 0.0, -1.0])
    loc, dec = cylinder_support(p, dl)
    return update_manifold(cache, R, o, link_threshold(p), loc + zoff, dec)


def update_box(p, box_state, cache):
    """The (plane, free box) manifold: box_state = [centre 3, quat xyzw 4, ...]."""
    R = np_model.quat_to_mat(np.asarray(box_state[3:7], float))
    o = np.asarray(box_state[0:3], float)
    dl = R.T @ np.array([0.0, 0.0, -1.0])
    a_new, dec = box_support(p, dl)
    return update_manifold(cache, R, o, box_threshold(p), a_new, dec)


def update_env(p, s, M):
    """Every link cylinder of one environment.  Returns dict(M [2n, 29], contacts [nc, 6] = world point, distance,
    link, lam0 in cylinder order then slot order, margin [2n], events [2n])."""
    n = int(p.n_modules)
    links, _ = _tree(n)
    out, C, mg, ev = [], [], [], []
    for c, (i, R, o, _) in enumerate(cylinder_frames(n, s)):
        r = update_link_cylinder(p, R, o, links[i]["cyl"], np.asarray(M[c], float))
        out.append(r["cache"])
        C += [[w[0], w[1], w[2], d, i, lam] for w, d, lam in r["points"]]
        mg.append(r["margin"])
        ev.append(r["events"])
    return dict(M=np.array(out), contacts=np.array(C).reshape(-1, 6), margin=np.array(mg), events=ev)


def stateless_contacts(p, s):
    """contact_model 0: per cylinder the lowest rim point of both end caps (-z first), margin along world-down, active
    below the threshold.  Returns (active [2n, 2], margin [2n])."""
    n = int(p.n_modules)
    thr, m, sides = link_threshold(p), float(p.collision_margin), int(p.hull_sides)
    act, mg = [], []
    for i, R, o, centre in cylinder_frames(n, s):
        dl = R.T @ np.array([0.0, 0.0, -1.0])
        if sides > 0:
            rim = hull_vertices(sides)[0::2, :2]
            k, lead = _first_max([float(dl[:2] @ v) for v in rim])
            xy, mrg = rim[k], lead / CYL_R
        else:
            rr = np.hypot(dl[0], dl[1])
            xy, mrg = (CYL_R * dl[:2] / rr if rr > 1e-12 else np.zeros(2)), rr
        row = []
        for z in (-CYL_HL, CYL_HL):
            w = centre + R @ (np.array([xy[0], xy[1], z]) + m * dl)
            row.append(w[2] < thr)
            mrg = min(mrg, abs(w[2] - thr) / max(np.abs(w).max(), CYL_R))
        act.append(row)
        mg.append(mrg)
    return np.array(act), np.array(mg)


# ----------------------------------------------------------------------------------------------------------------------
# case generators (float32-representable states and caches; everything downstream rounds nothing further)
# ----------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def _axis_quat(axis, ang):
    return np.concatenate([np.asarray(axis, float) * np.sin(0.5 * ang), [np.cos(0.5 * ang)]])


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


@functools.lru_cache(maxsize=None)
def _pitch_joints(n):
    """Which joints lift links off the plane when the snake lies along world x unrolled."""
    links, _ = _tree(n)
    Rw, _ = np_model.fk(links, np.zeros(3), np.array([0.0, 0, 0, 1]), np.zeros(n))
    return np.array([abs((Rw[i] @ np.array([0.0, 1, 0]))[2]) < 0.5 for i, k in enumerate(links) if k["rev"]])


def _settle(p, s, frac, at):
    """Moves the root along z so that the share `frac` of the cylinders has its new support point below `at`."""
    n = int(p.n_modules)
    links, _ = _tree(n)
    d = []
    for i, R, o, centre in cylinder_frames(n, s):
        loc, _ = cylinder_support(p, R.T @ np.array([0.0, 0.0, -1.0]))
        d.append((centre + R @ loc)[2])
    s = s.copy()
    s[2] += at - np.quantile(d, frac)
    return s


def pose(p, yaw, roll, pitch, q, frac=0.7, at=None):
    """State [13 + 2n] of a snake at rest: lying along world x, rolled about its long axis, pitched, turned by yaw,
    joints q, set down so that `frac` of its cylinders reach below `at` (default: half the threshold)."""
    n = int(p.n_modules)
    s = np.zeros(13 + 2 * n)
    s[3:7] = _qmul(_axis_quat([0, 0, 1], yaw), _qmul(_axis_quat([0, 1, 0], pitch), _axis_quat([1, 0, 0], roll)))
    s[13:13 + n] = q
    s = _f32(s)
    return _f32(_settle(p, s, frac, 0.5 * link_threshold(p) if at is None else at))


def ground_poses(p, rng, B):
    """Random resting poses: even environments curled in the plane (yaw joints up to 0.35 rad, a few degrees of roll),
    odd ones nearly straight and rolled by any angle; out-of-plane joint angles and the pitch sized so that neighbouring
    cylinders differ in height by about the threshold.  No cylinder lies exactly flat or on a rim edge other than by
    chance (the margin filter takes those out)."""
    n = int(p.n_modules)
    thr = link_threshold(p)
    A = 0.6 * thr / 0.064
    pj = _pitch_joints(n)
    S = []
    for i in range(B):
        q = rng.uniform(-A, A, n)
        if i % 2 == 0:
            q = np.where(pj, q, rng.uniform(-0.35, 0.35, n))
            roll = rng.uniform(-0.02, 0.02)
        else:
            roll = rng.uniform(-np.pi, np.pi)
        S.append(pose(p, rng.uniform(-np.pi, np.pi), roll, rng.uniform(-A, A) / 4, q, frac=rng.uniform(0.5, 0.95)))
    return np.array(S)


KINDS = ("valid", "lifted", "drifted", "near", "far")


def synth_caches(p, rng, S, dense_every=8):
    """Per cylinder a drawn number 0 ... 4 of cached points (four for 40 % of them) near the lower surface, each of
    one of KINDS relative to the pose and its coming support point.  Every `dense_every`-th environment holds four
    points that stay on every cylinder (more than 64 in all).  b.z is 0: the plane's."""
    n = int(p.n_modules)
    thr = link_threshold(p)
    links, _ = _tree(n)
    V = hull_vertices(32)
    Ms = []
    for e, s in enumerate(S):
        dense = dense_every and e % dense_every == dense_every - 1
        M = np.zeros((2 * n, 29))
        for c, (i, R, o, centre) in enumerate(cylinder_frames(n, s)):
            dl = R.T @ np.array([0.0, 0.0, -1.0])
            loc, _ = cylinder_support(p, dl)
            a_new = loc + links[i]["cyl"]
            cnt = 4 if dense else int(rng.choice([0, 1, 2, 3, 4, 4, 4]))
            kinds = ["far"] * 4 if (dense or (cnt == 4 and rng.uniform() < 0.5)) else list(rng.choice(KINDS, cnt))
            for j in range(cnt):
                kind = kinds[j]
                for _ in range(20):
                    if kind == "near":
                        u = rng.normal(size=3)
                        a = a_new + u / np.linalg.norm(u) * rng.uniform(0.05, 0.7) * thr
                        w = o + R @ a
                    else:
                        low = [v for v in V if dl @ v > 0]
                        w = centre + R @ low[rng.integers(len(low))]
                        w[2] = rng.uniform(1.3, 3.0) * thr if kind == "lifted" else rng.uniform(-0.5, 0.7) * thr
                        a = R.T @ (w - o)
                    if kind == "near" or np.linalg.norm(a - a_new) > (1.3 * thr if kind == "far" else 0.0):
                        break
                ang = rng.uniform(0, 2 * np.pi)
                r = rng.uniform(1.3, 3.0) * thr if kind == "drifted" else rng.uniform(0.0, 0.7) * thr
                M[c, 1 + 7 * j:4 + 7 * j] = a
                M[c, 4 + 7 * j:6 + 7 * j] = w[:2] + r * np.array([np.cos(ang), np.sin(ang)])
                M[c, 7 + 7 * j] = rng.uniform(0.0, 0.02)
            M[c, 0] = cnt
        Ms.append(M)
    return _f32(np.array(Ms))


def trajectory(p, rng, B, K=40):
    """[K, B, 13 + 2n]: every environment a nearly straight snake rolled about its long axis by a fixed increment per
    pose (a third of the threshold of rim travel, times 0.5 ... 1.5: never a multiple of the hull's 11.25 degrees) while
    its pitch and its height swing, so that caches fill, replace, drop and empty.

    EVICTION is reached on trajectories at the relative threshold only (default switch set, 1.2 mm: 0.3-0.7 % of the
    cylinder cases, always with the new point the deepest, never decided by the deepest-point exception).  At the
    absolute 0.02 m the roll step is 7-22 degrees per pose and the next support vertex (5.1 mm along the rim) lies
    within the threshold of a cached one, so it replaces; a fifth point 20 mm from four live ones does not fit on the
    lower side of a 52 x 33 mm cylinder that spins in place, whose points drift out first.  The eviction indices and
    both arms of the exception are the synthesised families' business (asserted there, every switch set)."""
    n = int(p.n_modules)
    thr = link_threshold(p)
    A = 0.6 * thr / 0.064
    out = np.zeros((K, B, 13 + 2 * n))
    for e in range(B):
        q = rng.uniform(-A, A, n)
        yaw, roll0 = rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi, np.pi)
        droll = thr / (3 * CYL_R) * rng.uniform(0.5, 1.5)
        amp, om, ph = rng.uniform(0.5, 2.0) * A, rng.uniform(0.2, 0.9), rng.uniform(0, 2 * np.pi)
        for k in range(K):
            out[k, e] = pose(p, yaw, roll0 + k * droll, amp * np.sin(om * k + ph), q, frac=0.8,
                             at=thr * (0.3 + 0.5 * np.sin(0.7 * om * k + 2 * ph)))
    return out


def box_cases(p, rng, B):
    """Tilted boxes near the ground with synthesised caches of the five kinds: (states [B, 13], caches [B, 29])."""
    h = np.array(p.obstacle_half[:], float)
    thr = box_threshold(p)
    S, M = np.zeros((B, 13)), np.zeros((B, 29))
    for e in range(B):
        ax = rng.normal(size=3)
        quat = _f32(_axis_quat(ax / np.linalg.norm(ax), rng.uniform(0.01, 0.12) * rng.choice([-1, 1])))
        if e % 5 == 4:                                             # lying on another face
            quat = _f32(_qmul(quat, _axis_quat([1.0, 0, 0] if e % 2 else [0, 1.0, 0], np.pi / 2 * rng.choice([-1, 1, 2]))))
        R = np_model.quat_to_mat(quat)
        dl = R.T @ np.array([0.0, 0.0, -1.0])
        a_new, _ = box_support(p, dl)
        pos = np.array([rng.uniform(1.5, 2.5), rng.uniform(-0.5, 0.5), 0.0])
        pos[2] = rng.uniform(-0.5, 1.2) * thr - (R @ a_new)[2]
        pos = _f32(pos)
        S[e, 0:3], S[e, 3:7] = pos, quat
        cnt = int(rng.choice([0, 1, 2, 3, 4, 4, 4]))
        kinds = ["far"] * 4 if cnt == 4 and rng.uniform() < 0.5 else list(rng.choice(KINDS, cnt))
        for j in range(cnt):
            kind = kinds[j]
            if kind == "near":
                u = rng.normal(size=3)
                a = a_new + u / np.linalg.norm(u) * rng.uniform(0.05, 0.7) * thr
                w = pos + R @ a
            else:
                a = np.where(rng.uniform(size=3) < 0.5, -h, h) * np.where(rng.uniform(size=3) < 0.3, rng.uniform(0, 1, 3), 1)
                if kind == "far" and np.linalg.norm(a - a_new) < 1.3 * thr:
                    a = a * np.array([-1.0, 1, 1])
                w = pos + R @ a
                w[2] = rng.uniform(1.3, 3.0) * thr if kind == "lifted" else rng.uniform(-0.5, 0.7) * thr
                a = R.T @ (w - pos)
            ang = rng.uniform(0, 2 * np.pi)
            r = rng.uniform(1.3, 3.0) * thr if kind == "drifted" else rng.uniform(0.0, 0.7) * thr
            M[e, 1 + 7 * j:4 + 7 * j] = a
            M[e, 4 + 7 * j:6 + 7 * j] = w[:2] + r * np.array([np.cos(ang), np.sin(ang)])
            M[e, 7 + 7 * j] = rng.uniform(0.0, 0.5)
        M[e, 0] = cnt
    return _f32(S), _f32(M)


# ----------------------------------------------------------------------------------------------------------------------
# comparison helpers shared by the CPU and the GPU file
# ----------------------------------------------------------------------------------------------------------------------
SWITCH_SETS = {
    "default": dict(),
    "hull+manifold@0.02": dict(hull_sides=32, contact_model=1, relative_breaking_threshold=0),
    "manifold": dict(hull_sides=0, contact_model=1, relative_breaking_threshold=0),
}


def cache_distance(M, ref):
    """Worst |a|, |b| difference of one 29-float cache against a reference with the same count (nan without points)."""
    cnt = int(ref[0])
    if cnt == 0:
        return np.nan
    g, r = np.asarray(M[1:1 + 7 * cnt], float).reshape(cnt, 7), np.asarray(ref[1:1 + 7 * cnt], float).reshape(cnt, 7)
    return np.abs(g[:, :5] - r[:, :5]).max()


# m: ten times float32 round-off of these coordinates (~1e-6 at worst, 32 links), and a sixth of the closest two points
# a generator puts into one cache ('near': no closer than 0.05 x 1.2 mm = 6e-5 to the coming support point), so that a
# kernel that replaced the wrong one of two near points fails the STRUCTURAL check
SAME_POINT = 1e-5


def same_structure(M, ref):
    """Counts equal and every slot holds the reference's point, not another one (within SAME_POINT; how close is the
    value comparison's business)."""
    cnt = int(ref[0])
    if int(M[0]) != cnt:
        return False
    for j in range(cnt):
        if np.abs(np.asarray(M[1 + 7 * j:6 + 7 * j], float) - ref[1 + 7 * j:6 + 7 * j]).max() > SAME_POINT:
            return False
    return True


def _seed(*key):
    import zlib
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=None)
def reference(switch, n, family):
    """The model's answer for one family of cases, computed once per process: dict(p, launches), every launch a dict
    (S [B, 13 + 2n], M [B, 2n, 29] float32-representable inputs, res = update_env per environment).  On a trajectory
    every launch starts from the model's cache of the pose before, rounded to float32."""
    import oracle
    p = oracle.default_params(n_modules=n, self_collision=0, **SWITCH_SETS[switch])
    rng = np.random.default_rng(_seed(switch, n, family))
    launches = []
    if family == "synth":
        S = ground_poses(p, rng, 64 if n == 16 else 32)
        M = synth_caches(p, rng, S)
        launches.append(dict(S=S, M=M))
    else:
        T = trajectory(p, rng, 12 if n == 16 else 6)
        M = np.zeros((T.shape[1], 2 * n, 29))
        for k in range(len(T)):
            launches.append(dict(S=T[k], M=M))
            M = _f32(np.array([update_env(p, T[k, e], M[e])["M"] for e in range(T.shape[1])]))
    for L in launches:
        L["res"] = [update_env(p, L["S"][e], L["M"][e]) for e in range(len(L["S"]))]
    return dict(p=p, launches=launches)


def retained(res):
    return res["margin"] >= MARGIN_BOUND


def coverage(events):
    """What the model's own outputs say a family reached: shares and sets the tests assert on."""
    ev = [e for e in events]
    n = max(len(ev), 1)
    drops = [e["drops"] for e in ev]
    slot_kind = set()
    for d in drops:
        for j, cnt in d:
            slot_kind.add("only" if cnt == 1 else "first" if j == 0 else "last" if j == cnt - 1 else "middle")
    evs = [e for e in ev if e["action"] == "evict"]
    return dict(evict_share=len(evs) / n, evicted=set(e["evict"] for e in evs),
                deepest_cached=sum(e["deepest"] >= 0 for e in evs), deepest_new=sum(e["deepest"] == -1 for e in evs),
                exception_decided=sum(e["unprotected"] != e["evict"] for e in evs),
                drop_slots=slot_kind, double_drops=sum(len(d) >= 2 for d in drops),
                actions={a: sum(e["action"] == a for e in ev) for a in ("none", "replace", "append", "evict")})


@functools.lru_cache(maxsize=None)
def box_reference(switch, B=192):
    """Free-box cases (obstacle 2) and the model's answers: dict(p, S [B, 13], M [B, 29], res)."""
    import oracle
    p = oracle.default_params(obstacle=2, self_collision=0, **SWITCH_SETS[switch])
    S, M = box_cases(p, np.random.default_rng(_seed("box", switch)), B)
    return dict(p=p, S=S, M=M, res=[update_box(p, S[e], M[e]) for e in range(B)])


@functools.lru_cache(maxsize=None)
def stateless_reference(name, n, B=32):
    """contact_model 0 handles (conftest.ROUND1, and the same with hulls): poses and the model's active points."""
    import oracle
    over = dict(hull_sides=0 if name == "ROUND1" else 32, contact_model=0, relative_breaking_threshold=0)
    p = oracle.default_params(n_modules=n, self_collision=0, **over)
    S = ground_poses(p, np.random.default_rng(_seed(name, n)), B)
    return dict(over=over, p=p, S=S, res=[stateless_contacts(p, s) for s in S])


@functools.lru_cache(maxsize=None)
def oracle_answers(switch, n, family, f32):
    """The oracle's update of every case of reference(switch, n, family), once per process: per launch and environment
    (cache [2n, 29], contact list [nc, 12], count)."""
    import oracle
    ref = reference(switch, n, family)
    o = oracle.OracleEnv(f32=f32, n_modules=n, self_collision=0, max_contacts=0, **SWITCH_SETS[switch])
    out = []
    for L in ref["launches"]:
        row = []
        for e in range(len(L["S"])):
            o.hard_reset()
            o.set_manifold(L["M"][e])
            o.set_state(L["S"][e])
            o.substep(np.zeros(n))
            row.append((o.get_manifold(), o.last_contacts_full(), o.last_num_contacts))
        out.append(row)
    return out


def cache_distances(ref, caches):
    """Distances to the model of the retained cylinder cases that hold points and have the model's structure; caches =
    per launch [B, 2n, 29].  Returns (distances, retained cases that differ in structure as (launch, env, cylinder))."""
    dist, bad = [], []
    for k, (L, Ms) in enumerate(zip(ref["launches"], caches)):
        for e, r in enumerate(L["res"]):
            for c in np.nonzero(retained(r))[0]:
                if not same_structure(Ms[e][c], r["M"][c]):
                    bad.append((k, e, int(c)))
                    continue
                d = cache_distance(Ms[e][c], r["M"][c])
                if not np.isnan(d):
                    dist.append(d)
    return np.array(dist), bad
