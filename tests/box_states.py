"""States with the free box (`obstacle 2`) for the tests of its physics (test helper, not product code): the gait run into
the box, synthesised ground states with the box placed beside a link, both in the air, twists -- and the selection of the
states a float32 program can be held to.  The link-box narrow phase is not under test here: the float64 oracle's contact
list is an input (np_substep), and it is what places the box."""
import numpy as np

import np_manifold as nm
import np_model
from conftest import random_state

MIRROR = dict(max_contacts=0, max_self_contacts=32)      # the kernels' room for link-link / box contacts
FREE_BOX = dict(obstacle=2, obstacle_pos=[0.100, 0.0, 0.1])

_gait = {}


def gait_box(oracle_mod, n, k, over):
    """(S, T, M, box states, box manifolds) of gait runs into the box in front of the snake's head."""
    from bench import gait_actions
    key = (n, k) + tuple(sorted((a, str(b)) for a, b in over.items()))
    if key in _gait:
        return _gait[key]
    rng = np.random.default_rng(1600 + n + over["obstacle"])
    e = oracle_mod.OracleEnv(n_modules=n, **MIRROR, **over)
    S, M, BS, BM = [], [], [], []
    for i in range(k):
        e.hard_reset()
        e.reset()
        for j in range(8 + i % 6):
            e.env_step(gait_actions(np.array([i + 1]), j, e.act_dim)[0], vec_mode=True)
        S.append(e.get_state())
        M.append(e.get_manifold())
        b = e.get_box() if over["obstacle"] == 2 else (np.zeros(13), np.zeros(29))
        BS.append(b[0])
        BM.append(b[1])
    _gait[key] = (np.array(S), rng.uniform(-0.5, 0.5, (k, n)), np.array(M), np.array(BS), np.array(BM))
    return _gait[key]


def twisted(rng, BS, w=5.0, v=2.0):
    """The box states with a random twist added: |omega| up to w, |v| up to v."""
    out = np.array(BS, float)
    for b in out:
        for sl, amp in ((slice(7, 10), w), (slice(10, 13), v)):
            d = rng.normal(size=3)
            b[sl] += d / np.linalg.norm(d) * amp * rng.uniform(0.2, 1.0)
    return out


def at_the_clamp(rng, BS):
    """Every box velocity component at +-99.5 ... 100 (max_coord_vel 100)."""
    out = np.array(BS, float)
    out[:, 7:13] = rng.choice([-1, 1], (len(out), 6)) * rng.uniform(99.5, 100.0, (len(out), 6))
    return out


def _axis_quat(axis, ang):
    return np.concatenate([np.sin(0.5 * ang) * np.asarray(axis, float), [np.cos(0.5 * ang)]])


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _ground_state(rng, n):
    s = random_state(rng, n, z=0.026, qamp=0.3, vamp=0.3, flat=True)
    s[9] *= 0.1
    s[7:9] *= 0.1
    return s


def link_box_distances(C):
    return C[C[:, 5] == -2, 3]


def beside_link(oracle_mod, rng, k, over, touching=0.75):
    """k ground states (empty contact caches) with the box at rest beside a randomly chosen link: random yaw, tilted by 1
    to 4 degrees about a random horizontal axis (a flat face on the ground ties its four corners), its lowest corner within
    half a millimetre of the ground, slid along its own x axis towards the link until the closest link-box pair is at a
    distance just below one drawn from [-1 mm, half the pair's breaking threshold] (`touching` of the states) or 5 mm further out (the
    rest: no link-box contact).  Returns (S [k, 13 + 2n], T [k, n], None, box states [k, 13], empty box caches [k, 29])."""
    n = 16
    e = oracle_mod.OracleEnv(n_modules=n, **MIRROR, **over)
    p = e.params
    h = np.array(p.obstacle_half[:], float)
    thr = nm.link_threshold(p)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * h
    S, BS = [], []
    for i in range(k):
        s = _ground_state(rng, n)
        frames = nm.cylinder_frames(n, s)
        c = frames[int(rng.integers(len(frames)))][3]
        th = rng.uniform(0, 2 * np.pi)
        quat = _qmul(_axis_quat([np.cos(th), np.sin(th), 0.0], np.radians(rng.uniform(1.0, 4.0))),
                     _axis_quat([0, 0, 1], rng.uniform(-np.pi, np.pi)))
        R = np_model.quat_to_mat(quat)
        z = -(corners @ R.T)[:, 2].min() + rng.uniform(-5e-4, 5e-4)
        u = np.array([R[0, 0], R[1, 0], 0.0]) * rng.choice([-1, 1])
        u /= np.linalg.norm(u)
        target = rng.uniform(-1e-3, 0.5 * thr)

        def box_at(d):
            return np.concatenate([[c[0] + u[0] * d, c[1] + u[1] * d, z], quat, np.zeros(6)])

        def closest(d):
            e.hard_reset()
            e.set_box(box_at(d), np.zeros(29))
            e.set_state(s)
            dist = link_box_distances(e.contacts_full())
            return dist.min() if len(dist) else np.inf
        lo, hi = 0.0, 2.0                       # at 0 the box holds the link's centre, at 2 m it is out of reach
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            if closest(mid) < target:
                lo = mid
            else:
                hi = mid
        d = lo
        if not i < touching * k:
            d = hi + 5e-3 + thr
            while np.isfinite(closest(d)):          # (another link in the way: further out, until no pair is in reach)
                d += 5e-3
        S.append(s)
        BS.append(box_at(d))
    return np.array(S), rng.uniform(-0.5, 0.5, (k, n)), None, np.array(BS), np.zeros((k, 29))


def in_the_air(rng, k):
    """Snake and box a metre apart and a metre up: no contact of any kind."""
    n = 16
    S = np.array([random_state(rng, n, z=1.0, qamp=0.5, vamp=1.0) for _ in range(k)])
    BS = np.zeros((k, 13))
    for b in BS:
        b[0:3] = [1.5, rng.uniform(-0.2, 0.2), 1.0]
        q = rng.normal(size=4)
        b[3:7] = q / np.linalg.norm(q)
    return S, rng.uniform(-0.5, 0.5, (k, n)), None, BS, np.zeros((k, 29))


def run_oracle(e, s, t, M, box, mu):
    """One substep of an oracle env from a clean slate."""
    e.hard_reset()
    e.set_plane_friction(mu)
    if M is not None:
        e.set_manifold(M)
    e.set_box(*box)
    e.set_state(s)
    e.substep(t)


def start_impulses(p, s, M, box, C):
    """lam0 of np_substep for the contact list C (ground, link-link, link-box, box-ground): the snake's ground contacts'
    from the cache model on M (None: empty caches), the box's own from the cache model on its manifold, the others zero."""
    n = int(p.n_modules)
    lam = nm.update_env(p, s, np.zeros((2 * n, 29)) if M is None else M)["contacts"][:, 5]
    own = np.array([pt[2] for pt in nm.update_box(p, box[0], box[1])["points"]])
    assert len(lam) == ((C[:, 4] >= 0) & (C[:, 5] == -1)).sum() and len(own) == (C[:, 4] < 0).sum(), (len(lam), len(own))
    assert (C[:len(lam), 5] == -1).all() and (C[len(C) - len(own):, 4] < 0).all()
    return np.concatenate([lam, np.zeros(len(C) - len(lam) - len(own)), own])


def select_for_float32(oracle_mod, over, S, T, M, BS, BM, mu=1.0, want=16):
    """The first `want` candidates a float32 program can be held to, from float32-rounded inputs: the float64 and float32
    oracles solve the same contact list (count, link pairs) and every link-box distance is at least 1e-5 m away from the
    pair's breaking threshold.  Returns (indices kept, number of candidates looked at)."""
    f = lambda a: None if a is None else np.asarray(a, np.float32).astype(np.float64)      # noqa: E731
    o = oracle_mod.OracleEnv(n_modules=16, **MIRROR, **over)
    o32 = oracle_mod.OracleEnv(n_modules=16, f32=True, **MIRROR, **over)
    thr = nm.link_threshold(o.params)
    keep, seen = [], 0
    for i in range(len(S)):
        if len(keep) == want:
            break
        seen += 1
        for e in (o, o32):
            run_oracle(e, f(S[i]), f(T[i]), None if M is None else f(M[i]), (f(BS[i]), f(BM[i])), float(np.float32(mu)))
        C, C32 = o.last_contacts_full(), o32.last_contacts_full()
        if len(C) != len(C32) or not np.array_equal(C[:, 4:6], C32[:, 4:6]):
            continue
        if (np.abs(link_box_distances(C) - thr) < 1e-5).any():
            continue
        keep.append(i)
    return keep, seen
