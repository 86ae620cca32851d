"""The float64 oracle's substep against tests/np_substep.py, a float64 numpy model written from the rules (CPU).

Until this file the oracle's substep was held to an independent derivation only at zero velocity (mass matrix,
momentum, gravity: tests/test_oracle_physics.py); everything after free motion -- velocity-product and damping terms,
the contact / limit / motor rows, btPlaneSpace1 tangents and their anisotropic scaling, the cone projection, the sweep
order, the residual exit -- was checked by invariants only, and the GPU is gated against the oracle.  Both programs
here run the same sequence in float64, so any difference above round-off is a finding, not noise.

The last section does the same for the free box (obstacle 2), which np_substep models as a second body behind the snake's
velocity components: states from tests/box_states.py, the box's six velocities and its pose measured with the snake's.

Every test prints `BOUND <what>: largest <observed> <= <bound>`.
"""
import numpy as np
import pytest

import np_substep as ns
from conftest import ROUND1, random_state

TOL_VEL = 1e-8        # post-substep velocities, relative: |d| / (1 + |v|)
TOL_POSE = 1e-10      # base position, quaternion, joint angles, relative to 1 + max |v| (the pose moves by dt v)
TOL_IMP = 1e-8        # normal impulses, relative to the substep's largest
TOL_TAU = 1e-8        # motor torques (impulse / dt), relative to max(1, the largest)
BOUNDS = dict(vel=TOL_VEL, pose=TOL_POSE, normal=TOL_IMP, tau=TOL_TAU)
BOX = dict(obstacle=1, obstacle_pos=[0.100, 0.0, 0.1])        # its face 2 mm in front of the resting snake's head


class Worst:
    """The largest error per bound over a test's substeps, printed and asserted at the end."""

    def __init__(self, name, bounds=None):
        self.name = name
        self.bounds = BOUNDS if bounds is None else bounds
        self.e = dict(vel=0.0, pose=0.0, normal=0.0, tau=0.0)
        self.count = 0
        self.contacts = 0
        self.iters = []
        self.bifurcations = []

    def add(self, d):
        if d["excused"]:
            self.bifurcations.append(d["excused"])
        for k in self.e:
            if k not in d["excused"]:
                self.e[k] = max(self.e[k], d[k])
        self.count += 1
        self.contacts += d["nc"]
        self.iters.append(d["iters"])

    def check(self):
        print("  [%s] %d substeps, %d contacts, iterations %s" % (self.name, self.count, self.contacts,
                                                                 sorted(set(self.iters))))
        for b in self.bifurcations:
            for k, (err, spread) in b.items():
                print("  [%s] bifurcation: %s off by %.2e, the model's own spread under 1e-15 input noise %.2e"
                      % (self.name, k, err, spread))
        for k, b in self.bounds.items():
            print("  BOUND %-58s largest %.2e <= %.1e" % ("%s: %s" % (self.name, k), self.e[k], b))
        for k, b in self.bounds.items():
            assert self.e[k] <= b, (self.name, k, self.e[k], b)
        assert len(self.bifurcations) <= 1, self.bifurcations


def _errors(n, x, N, tau, ref, Nref, tauref, box=None, boxref=None):
    """(box, boxref: the free box's 13 floats; its six velocities and its pose join the snake's, measured the same way)"""
    d = {}
    d["vel"] = max((np.abs(x[7:13] - ref[7:13]) / (1 + np.abs(ref[7:13]))).max(),
                   (np.abs(x[13 + n:] - ref[13 + n:]) / (1 + np.abs(ref[13 + n:]))).max())
    vs = 1 + max(np.abs(ref[7:13]).max(), np.abs(ref[13 + n:]).max())
    if boxref is not None:
        d["vel"] = max(d["vel"], (np.abs(box[7:13] - boxref[7:13]) / (1 + np.abs(boxref[7:13]))).max())
        vs = max(vs, 1 + np.abs(boxref[7:13]).max())
    d["pose"] = max(np.abs(x[0:7] - ref[0:7]).max(), np.abs(x[13:13 + n] - ref[13:13 + n]).max()) / vs
    if boxref is not None:
        d["pose"] = max(d["pose"], np.abs(box[0:7] - boxref[0:7]).max() / vs)
    d["normal"] = np.abs(N - Nref).max() / max(np.abs(Nref).max(), 1e-6) if len(Nref) else 0.0
    d["tau"] = np.abs(tau - tauref).max() / max(1.0, np.abs(tauref).max())
    return d


def compare(e, s, T, mu_plane=1.0, manifold=None, lam0=None, box=None, bounds=None):
    """One oracle substep from (s, manifold) and the numpy model on the contacts the oracle solved.  box: (state [13],
    manifold [29]) of the free box (obstacle 2); lam0 then covers the whole list (box_states.start_impulses); bounds: the
    figures beyond which a state is looked at as a bifurcation (BOUNDS).

    A figure beyond its bound is a finding unless the state is a bifurcation for THAT figure: the numpy model itself, run
    from inputs moved by 1e-15 relative, spreads in that figure by at least a tenth of the difference (a contact on the
    edge between sticking and slipping amplifies round-off by 1e10 and more over 50 unconverged sweeps).  Only the
    figures so measured are excused (`excused`: {figure: (difference, spread)}), every other figure of the state still
    counts, and a test may hold at most one such state."""
    n = e.n
    bounds = BOUNDS if bounds is None else bounds
    e.hard_reset()
    e.set_plane_friction(mu_plane)
    if manifold is not None:
        e.set_manifold(manifold)
    if box is not None:
        e.set_box(*box)
    e.set_state(s)
    e.substep(T)
    C = e.last_contacts_full()
    ref = e.get_state()
    tau = e.get_aux()[0]
    N = e.last_normal_impulses()
    assert len(N) == len(C)
    if lam0 is not None:
        lam0 = np.concatenate([lam0, np.zeros(len(C) - len(lam0))])      # link-link / box contacts carry none
    b0 = None if box is None else np.asarray(box[0], float)
    bref = None if box is None else e.get_box()[0]
    r = ns.substep(e.params, s, T, C, mu_plane=mu_plane, lam0=lam0, box=b0)
    d = _errors(n, r["state"], r["normal"], r["tau_motor"], ref, N, tau, r["box"], bref)
    d.update(nc=len(C), iters=r["iterations"], r=r, C=C, ref=ref, boxref=bref, excused={})
    assert r["iterations"] == e.last_iterations, (r["iterations"], e.last_iterations)
    if any(d[k] > b for k, b in bounds.items()):
        rng = np.random.default_rng(0)
        spread = dict.fromkeys(bounds, 0.0)
        for _ in range(2):
            s2 = s * (1 + 1e-15 * rng.uniform(-1, 1, s.shape))
            r2 = ns.substep(e.params, s2, T, C, mu_plane=mu_plane, lam0=lam0, box=b0)
            e2 = _errors(n, r2["state"], r2["normal"], r2["tau_motor"], r["state"], r["normal"], r["tau_motor"],
                         r2["box"], r["box"])
            for k in bounds:
                spread[k] = max(spread[k], e2[k])
        d["excused"] = {k: (d[k], spread[k]) for k, b in bounds.items() if d[k] > b and spread[k] >= 0.1 * d[k]}
    return d


def ground_states(rng, n, k, **kw):
    out = []
    for _ in range(k):
        s = random_state(rng, n, z=0.026, qamp=kw.get("qamp", 0.3), vamp=kw.get("vamp", 0.3), flat=True)
        s[9] *= 0.1
        s[7:9] *= 0.1
        out.append(s)
    return out


def gait_states(oracle_mod, n, k, steps=(3, 6), **over):
    """(state, manifold) pairs the gait produces: oracle env-steps under bench.gait_actions from the reset."""
    from bench import gait_actions
    e = oracle_mod.OracleEnv(n_modules=n, **over)
    out = []
    for i in range(k):
        e.hard_reset()
        e.reset()
        for j in range(steps[i % len(steps)]):
            e.env_step(gait_actions(np.array([i + 1]), j, e.act_dim)[0], vec_mode=True)
        out.append((e.get_state(), e.get_manifold() if e.params.contact_model == 1 else None))
    return out


# ------------------------------------------------------------------------------------------------------------------
# free motion alone
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 32])
def test_free_motion_at_velocity(oracle_mod, n):
    """forward_dynamics(tau = -joint_damping qd, damping on) at nonzero v, w, qd against the numpy acceleration (bias by
    a central difference of the Jacobians, link damping k + k|.| on the COM velocity and on w)."""
    rng = np.random.default_rng(70 + n)
    e = oracle_mod.OracleEnv(n_modules=n)
    ch = ns.Chain(e.params)
    worst = 0.0
    for i in range(5):
        s = random_state(rng, n, z=1.0, qamp=0.8, vamp=[1.0, 3.0, 10.0, 1.0, 3.0][i])
        e.set_state(s)
        tau = -e.params.joint_damping * s[13 + n:]
        acc = e.forward_dynamics(tau, gravity=True, damping=True)
        a = ch.free_acceleration(s, tau=tau)[0]
        worst = max(worst, np.abs(a - acc).max() / (1 + np.abs(acc).max()))
        # the velocity-dependent part on its own (no gravity) is not small against the comparison
        a0 = e.forward_dynamics(tau, gravity=False, damping=True)
        assert np.abs(a0).max() > 1e-2
    print("  BOUND free motion %d links: relative acceleration largest %.2e <= 1e-08" % (n, worst))
    assert worst <= 1e-8


# ------------------------------------------------------------------------------------------------------------------
# one substep: random ground states under every switch set
# ------------------------------------------------------------------------------------------------------------------
SWITCHES = {
    "default": {},
    "round1": ROUND1,
    "cone_friction 0": dict(cone_friction=0),
    "friction_directions 1": dict(friction_directions=1),
    "contact_order 1": dict(contact_order=1),
    "contact_order 2": dict(contact_order=2),
    "contact_order 3": dict(contact_order=3),
}


@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_substep_random_ground(oracle_mod, n, switch):
    rng = np.random.default_rng(100 + 7 * n + list(SWITCHES).index(switch))
    w = Worst("%d links ground, %s" % (n, switch))
    k = 3 if n == 16 else 2
    for thr in (0.0, 1e-7):
        e = oracle_mod.OracleEnv(n_modules=n, residual_threshold=thr, **SWITCHES[switch])
        for s in ground_states(rng, n, k):
            w.add(compare(e, s, rng.uniform(-0.5, 0.5, n)))
    assert w.contacts >= 3 * w.count
    w.check()


# ------------------------------------------------------------------------------------------------------------------
# states the gait produces (populated manifolds), and the manifold order derived in numpy
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 32])
def test_substep_gait_states(oracle_mod, n):
    rng = np.random.default_rng(200 + n)
    w = Worst("%d links, gait states" % n)
    for over in ({}, dict(residual_threshold=0.0)):
        e = oracle_mod.OracleEnv(n_modules=n, **over)
        for s, m in gait_states(oracle_mod, n, 3 if n == 16 else 2):
            w.add(compare(e, s, rng.uniform(-0.5, 0.5, n), manifold=m))
    w.check()


def warm_states(oracle_mod, n, k):
    """(state, cache, lam0) from a short gait run under warm_start 1: populated caches with non-zero impulses; lam0 per
    ground contact from the cache model (np_manifold), which must hold the points the oracle then solves."""
    import np_manifold as nm
    out = []
    p = oracle_mod.default_params(n_modules=n, warm_start=1)
    for s, m in gait_states(oracle_mod, n, k, warm_start=1):
        c = nm.update_env(p, s, m)["contacts"]
        assert np.abs(m[:, 7::7]).max() > 1e-4 and np.abs(c[:, 5]).max() > 1e-4
        out.append((s, m, c[:, 5]))
    return out


@pytest.mark.parametrize("n", [16, 32])
def test_substep_warm_start(oracle_mod, n):
    """warm_start 1 from gait states with their caches, both chain lengths (the float64 oracle is one program for the
    three GPU paths; tests/test_gpu_np_substep.py runs the same states on each of them)."""
    rng = np.random.default_rng(250 + n)
    w = Worst("%d links, warm start" % n)
    moved = 0.0
    for over in ({}, dict(residual_threshold=0.0)):
        e = oracle_mod.OracleEnv(n_modules=n, warm_start=1, **over)
        for s, m, lam0 in warm_states(oracle_mod, n, 3 if n == 16 else 2):
            T = rng.uniform(-0.5, 0.5, n)
            d = compare(e, s, T, manifold=m, lam0=lam0)
            assert (d["C"][:len(lam0), 5] == -1).all() and (d["C"][len(lam0):, 5] != -1).all()
            w.add(d)
            cold = ns.substep(e.params, s, T, d["C"], lam0=None)["state"]
            moved = max(moved, np.abs(cold[13 + n:] - d["r"]["state"][13 + n:]).max())
    assert moved > 1e-6, moved                 # the start impulses are not a no-op on these states
    w.check()


@pytest.mark.parametrize("n", [16, 32])
def test_manifold_order_from_the_written_rule(oracle_mod, n):
    """contact_order 1 / 2 / k >= 3: the order of last_contacts_full equals the link-ordered list permuted in numpy
    (runs of one link reversed / by quickSort on 2n equal keys / by the hash of (k, link)); and the substep on it agrees."""
    rng = np.random.default_rng(300 + n)
    w = Worst("%d links, contact_order on gait states" % n)
    e0 = oracle_mod.OracleEnv(n_modules=n)
    moved = 0
    for s, m in gait_states(oracle_mod, n, 2, steps=(4,)):
        e0.hard_reset()
        e0.set_manifold(m)
        e0.set_state(s)
        T = rng.uniform(-0.5, 0.5, n)
        e0.substep(T)
        C0 = e0.last_contacts_full()
        assert len(np.unique(C0[C0[:, 5] == -1, 4])) >= 4
        for k in (1, 2, 3, 4):
            e = oracle_mod.OracleEnv(n_modules=n, contact_order=k)
            d = compare(e, s, T, manifold=m)
            perm = ns.manifold_order(C0, k, n)
            assert np.array_equal(d["C"], C0[perm]), k
            moved += perm != list(range(len(C0)))
            w.add(d)
    assert moved == 8
    w.check()


# ------------------------------------------------------------------------------------------------------------------
# the edges: limits, folded snakes, the static box, the velocity clamp, friction coefficients, the ERP rule
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 32])
def test_substep_joints_past_both_limits(oracle_mod, n):
    rng = np.random.default_rng(400 + n)
    w = Worst("%d links past the limits" % n)
    sides = set()
    for z in (1.0, 0.026):
        e = oracle_mod.OracleEnv(n_modules=n, residual_threshold=0.0)
        for _ in range(2):
            s = random_state(rng, n, z=z, qamp=1.0, vamp=0.3, flat=z < 0.5)
            s[13:13 + n] = rng.choice([-1, 1], n) * rng.uniform(1.575, 1.8, n) * (rng.uniform(size=n) < 0.5)
            d = compare(e, s, rng.uniform(-0.5, 0.5, n))
            sides |= {float(r.J[6 + r.joint]) for r in d["r"]["noncontact"] if r.kind == "limit"}
            w.add(d)
    assert sides == {-1.0, 1.0}
    w.check()


def _folded_with_link_contacts(oracle_mod, rng, k, **over):
    e = oracle_mod.OracleEnv(**over)
    out = []
    while len(out) < k:
        s = ground_states(rng, 16, 1, qamp=1.7)[0]
        e.set_state(s)
        C = e.contacts_full()
        if len(C) and (C[:, 5] >= 0).sum() >= 2:
            out.append(s)
    return out


@pytest.mark.parametrize("mu_link", [2.0, 6.0])
def test_substep_folded_link_link(oracle_mod, mu_link):
    """Snakes folded onto themselves (self_collision 1): two-body rows J_A(P_A) - J_B(P_B), tangents scaled by link A's
    then link B's anisotropy.  mu_link 6: the pair's product 36 is clamped at 10 like every other pair's."""
    rng = np.random.default_rng(500 + int(mu_link))
    w = Worst("16 links folded, mu_link %g" % mu_link)
    e = oracle_mod.OracleEnv(mu_link=mu_link)
    for s in _folded_with_link_contacts(oracle_mod, rng, 6):
        d = compare(e, s, rng.uniform(-0.5, 0.5, 16))
        assert (d["C"][:, 5] >= 0).any()
        w.add(d)
    w.check()


def test_substep_static_box(oracle_mod):
    """obstacle 1 (16 links): one-body rows against the box, mu_link x mu_obstacle; states the gait pushes into it."""
    rng = np.random.default_rng(600)
    w = Worst("16 links against the static box")
    e = oracle_mod.OracleEnv(**BOX)
    boxed = 0
    for s, m in gait_states(oracle_mod, 16, 4, steps=(10, 14), **BOX):
        d = compare(e, s, rng.uniform(-0.5, 0.5, 16), manifold=m)
        boxed += int((d["C"][:, 5] == -2).sum())
        w.add(d)
    assert boxed >= 4
    w.check()


@pytest.mark.parametrize("n", [16, 32])
def test_substep_velocity_clamp(oracle_mod, n):
    """In air, weak motors (max_motor_impulse 0.05) and qd near +-100: the clamp to max_coord_vel fires on v + a dt
    and on v_free + dv."""
    rng = np.random.default_rng(700 + n)
    w = Worst("%d links at the velocity clamp" % n)
    e = oracle_mod.OracleEnv(n_modules=n, max_motor_impulse=0.05)
    clamped = 0
    for _ in range(3):
        s = random_state(rng, n, z=1.0, qamp=0.5, vamp=1.0)
        s[13 + n:] = rng.choice([-1, 1], n) * rng.uniform(99.0, 100.0, n)
        d = compare(e, s, rng.uniform(-0.5, 0.5, n))
        clamped += int((np.abs(d["r"]["v_free"]) == e.params.max_coord_vel).sum())
        clamped += int((np.abs(d["ref"][13 + n:]) == e.params.max_coord_vel).sum())
        w.add(d)
    assert clamped >= 4
    w.check()


@pytest.mark.parametrize("mu_plane", [0.0, 1.5, 6.0])
def test_substep_ground_friction(oracle_mod, mu_plane):
    """mu = mu_link x mu_plane: 0 (a zero cone), 3, and 12 clamped to 10 (MAX_FRICTION)."""
    rng = np.random.default_rng(800 + int(10 * mu_plane))
    w = Worst("16 links, plane friction %g" % mu_plane)
    for over in ({}, dict(cone_friction=0)):
        e = oracle_mod.OracleEnv(residual_threshold=0.0, **over)
        for s in ground_states(rng, 16, 2, vamp=1.0):
            w.add(compare(e, s, rng.uniform(-0.5, 0.5, 16), mu_plane=mu_plane))
    w.check()


def test_substep_contact_erp_rule(oracle_mod):
    """contact_erp_rule 1: m_erp (0.2) for contacts shallower than the split-impulse threshold, contact_erp below it;
    snakes tilted into the ground so that one substep holds contacts on both sides of 4 cm."""
    rng = np.random.default_rng(900)
    w = Worst("16 links, contact_erp_rule 1")
    e = oracle_mod.OracleEnv(contact_erp_rule=1, contact_model=0, residual_threshold=0.0)
    found = 0
    while found < 3:
        s = ground_states(rng, 16, 1)[0]
        s[2] = rng.uniform(0.0, 0.03)
        th = rng.uniform(0, 2 * np.pi)
        s[3:7] = ns.rotate_quat(s[3:7], rng.uniform(0.01, 0.04) * np.array([np.cos(th), np.sin(th), 0.0]))
        e.set_state(s)
        pen = e.contacts_full()[:, 3] + e.params.linear_slop
        if not ((pen < -0.045).any() and ((pen > -0.035) & (pen <= 0)).any()):
            continue
        found += 1
        w.add(compare(e, s, rng.uniform(-0.5, 0.5, 16)))
    w.check()


# ------------------------------------------------------------------------------------------------------------------
# solver-free: the rows pinned by complementarity on the oracle's converged result
# ------------------------------------------------------------------------------------------------------------------
def _complementarity(e, r):
    """The numpy-built rows `r` (ns.substep with no sweeps: rows at v_free) against the oracle's converged result:
    normals lambda >= 0, J v+ >= target and lambda (J v+ - target) = 0; motor rows met unless at their bound; friction
    inside the cone (cone_friction 0: each row inside +-mu lambda_n), J v+ = 0 where strictly inside, and on the rim
    the impulse opposes the slip (cone: the pair parallel to -(dinv_A J_A v+, dinv_B J_B v+), the fixed point of the
    radial projection; box: each row's sign against its slip).  Velocities relative to 1 + max |v+|, impulses to the
    largest normal impulse."""
    n = e.n
    ref = e.get_state()
    vplus = np.concatenate([ref[7:13], ref[13 + n:]])
    vs = 1 + np.abs(vplus).max()
    N = e.last_normal_impulses()
    F = e.last_friction_impulses()
    Ns = max(np.abs(N).max(), 1e-9) if len(N) else 1.0
    out = dict(normal=0.0, motor=0.0, stick=0.0, slip=0.0, cone=0.0)
    for row, lam in zip(r["normals"], N):
        slack = row.J @ vplus - (row.J @ r["v_free"] + row.rhs / row.dinv)
        assert lam >= 0
        out["normal"] = max(out["normal"], -slack / vs, min(abs(slack) / vs, lam / Ns))
    tau = e.get_aux()[0]
    for row in r["noncontact"]:
        if row.kind == "motor" and abs(tau[row.joint] * e.params.dt) < e.params.max_motor_impulse * (1 - 1e-9):
            target = row.J @ r["v_free"] + row.rhs / row.dinv
            out["motor"] = max(out["motor"], abs(row.J @ vplus - target) / vs)
    box = int(e.params.cone_friction) == 0
    for ci, (A, B) in enumerate(r["pairs"]):
        lim = r["mus"][ci] * N[ci]
        lam = F[ci]
        u = np.array([A.J @ vplus, B.J @ vplus])
        if box:
            if lim <= 0:
                continue         # rows with a zero bound are not swept: they keep what they held
            out["cone"] = max(out["cone"], (np.abs(lam).max() - lim) / Ns)
            for x, ux in zip(lam, u):
                if abs(x) < lim * (1 - 1e-6):
                    out["stick"] = max(out["stick"], abs(ux) / vs)
                elif abs(ux) > 1e-9 * vs:
                    out["slip"] = max(out["slip"], float(np.sign(x) == np.sign(ux)))
            continue
        rad = np.hypot(*lam)
        out["cone"] = max(out["cone"], (rad - lim) / Ns)
        if rad < lim * (1 - 1e-6):
            out["stick"] = max(out["stick"], np.abs(u).max() / vs)
        elif lim > 1e-6 * Ns:
            du = -np.array([A.dinv, B.dinv]) * u
            if np.hypot(*du) > 1e-9:
                out["slip"] = max(out["slip"], 1 - lam @ du / (rad * np.hypot(*du)))
    return out


def test_converged_complementarity(oracle_mod):
    """A few states of each kind, swept by the oracle until its result no longer moves (20000 sweeps, no residual exit;
    1000 are not enough: a gait state's motor rows are still 4e-5 off their targets after 1000): the conditions the
    numpy-built rows define, evaluated on the oracle's result (its velocities, normal, friction and motor impulses,
    orc_last_friction_impulses) -- no dependence on the sweep order.  A state counts where 25000 sweeps leave v+ where
    20000 did (to 1e-9); some never settle -- a folded snake whose link-link contacts fight unbounded motors cycles --
    and are reported, but every kind must have one that does.  (The 32-link chain's gait states were still moving by
    1e-3 after 20000 sweeps: its rows are pinned by the per-substep comparisons only.)"""
    rng = np.random.default_rng(1000)
    over = dict(n_iterations=20000, residual_threshold=0.0)
    cases = [("gait", {}, gait_states(oracle_mod, 16, 2, steps=(4, 7))),
             ("cone_friction 0", dict(cone_friction=0), gait_states(oracle_mod, 16, 1, steps=(5,))),
             ("folded", {}, [(s, None) for s in _folded_with_link_contacts(oracle_mod, rng, 2)]),
             ("box", BOX, gait_states(oracle_mod, 16, 1, steps=(10,), **BOX))]
    bounds = dict(normal=1e-8, motor=1e-8, stick=1e-8, slip=1e-6, cone=1e-12)
    worst = dict.fromkeys(bounds, 0.0)
    kinds = set()
    settled = {}
    for name, sw, states in cases:
        e = oracle_mod.OracleEnv(**sw, **over)
        e2 = oracle_mod.OracleEnv(**dict(over, n_iterations=25000), **sw)
        for s, m in states:
            T = rng.uniform(-0.5, 0.5, e.n)
            for x in (e2, e):
                x.hard_reset()
                if m is not None:
                    x.set_manifold(m)
                x.set_state(s)
                x.substep(T)
            assert e.last_iterations == over["n_iterations"]
            moved = np.abs(e.get_state()[7:] - e2.get_state()[7:]).max()
            C = e.last_contacts_full()
            c = _complementarity(e, ns.substep(e.params, s, T, C, n_iterations=0))
            print("  %-16s %3d contacts, v+ moved %.1e by 5000 more sweeps: " % (name, len(C), moved)
                  + ", ".join("%s %.1e" % kv for kv in c.items()))
            if moved > 1e-9:
                continue
            settled[name] = settled.get(name, 0) + 1
            kinds |= set(C[:, 5].clip(-2, 0).astype(int))
            for k in worst:
                worst[k] = max(worst[k], c[k])
    assert len(settled) == len(cases), settled
    assert kinds == {-2, -1, 0}
    for k, b in bounds.items():
        print("  BOUND converged complementarity: %-32s largest %.2e <= %.0e" % (k, worst[k], b))
    for k, b in bounds.items():
        assert worst[k] <= b, (k, worst[k], b)


# ------------------------------------------------------------------------------------------------------------------
# the sweep ladder: both references mean the same thing by "k sweeps"
# ------------------------------------------------------------------------------------------------------------------
LADDER = (1, 2, 3, 5, 10, 25)


@pytest.mark.parametrize("k", LADDER)
@pytest.mark.parametrize("switch", ["default", "cone_friction 0", "friction_directions 1"])
@pytest.mark.parametrize("n", [16, 32])
def test_sweep_ladder(oracle_mod, n, switch, k):
    """n_iterations k without the residual exit, the same 8 ground states per (n, switch) at every k: sweep 1 takes the
    non-contact rows backward and meets the friction rows while most normal impulses are still zero, sweep 2 takes them
    forward with the bounds live.  Velocities to 1e-9 relative (largest observed 1.0e-10, on 32 links), both iteration counts k:
    tests/test_gpu_np_sweeps.py holds the kernels to the model at these k."""
    rng = np.random.default_rng(1900 + 7 * n + len(switch))
    e = oracle_mod.OracleEnv(n_modules=n, residual_threshold=0.0, n_iterations=k, **SWITCHES[switch])
    worst, contacts = 0.0, 0
    for s in ground_states(rng, n, 8):
        d = compare(e, s, rng.uniform(-0.5, 0.5, n))
        assert d["iters"] == k and e.last_iterations == k, (d["iters"], e.last_iterations, k)
        worst = max(worst, d["vel"])
        contacts += d["nc"]
    print("  BOUND %-58s largest %.2e <= 1e-09" % ("%d links, %s, %d sweeps: vel" % (n, switch, k), worst))
    assert contacts >= 3 * 8
    assert worst <= 1e-9, (n, switch, k, worst)


# ------------------------------------------------------------------------------------------------------------------
# the free box (obstacle 2): a second body behind the snake's velocity components
# ------------------------------------------------------------------------------------------------------------------
# velocities (the box's six among them) 1e-9 relative, poses (the box's among them) 7e-12, normal impulses 1.5e-9
BOX_BOUNDS = dict(vel=1e-9, pose=7e-12, normal=1.5e-9, tau=TOL_TAU)
_box_sets = {}


def box_set(oracle_mod, kind, **over):
    """(S, T, M, BS, BM) of box_states, built once per (kind, parameters)."""
    import box_states as bs
    key = (kind,) + tuple(sorted(over.items()))
    if key not in _box_sets:
        full = dict(bs.FREE_BOX, **over)
        if kind == "gait":
            _box_sets[key] = bs.gait_box(oracle_mod, 16, 8, full)
        elif kind == "beside":
            _box_sets[key] = bs.beside_link(oracle_mod, np.random.default_rng(2100), 12, full)
        else:
            _box_sets[key] = bs.in_the_air(np.random.default_rng(2101), 8)
    return _box_sets[key]


def run_box_case(oracle_mod, name, kind, over, mu_plane=1.0, motion=("found", "twisted"), seed=0, min_link_box=0.5,
                 set_over=None):
    """One substep per (state, box motion) of a set under `over`, every figure against BOX_BOUNDS; at least `min_link_box`
    of the substeps hold a link-box contact.  Returns the per-substep results."""
    import box_states as bs
    rng = np.random.default_rng(2200 + seed)
    S, T, M, BS, BM = box_set(oracle_mod, kind, **(over if set_over is None else set_over))
    e = oracle_mod.OracleEnv(**bs.MIRROR, **dict(bs.FREE_BOX, **over))
    w = Worst(name, BOX_BOUNDS)
    out, with_pair = [], 0
    for how in motion:
        B = dict(found=lambda: BS, twisted=lambda: bs.twisted(rng, BS), clamp=lambda: bs.at_the_clamp(rng, BS))[how]()
        for i in range(len(S)):
            m = None if M is None else M[i]
            lam0 = None
            if int(e.params.warm_start):
                e.hard_reset()
                if m is not None:
                    e.set_manifold(m)
                e.set_box(B[i], BM[i])
                e.set_state(S[i])
                lam0 = bs.start_impulses(e.params, S[i], m, (B[i], BM[i]), e.contacts_full())
            d = compare(e, S[i], T[i], mu_plane=mu_plane, manifold=m, lam0=lam0, box=(B[i], BM[i]), bounds=BOX_BOUNDS)
            with_pair += bool((d["C"][:, 5] == -2).any())
            d["how"] = how
            w.add(d)
            out.append(d)
    print("  [%s] %d of %d substeps with a link-box contact, %d box-ground contacts" %
          (name, with_pair, len(out), sum(int((d["C"][:, 4] < 0).sum()) for d in out)))
    assert 8 <= len(S) <= 16 and with_pair >= min_link_box * len(out), (with_pair, len(out))
    w.check()
    return out


@pytest.mark.parametrize("mass", [200.0, 0.5])
@pytest.mark.parametrize("mu_plane", [0.0, 1.0, 6.0])
def test_free_box_gait_states(oracle_mod, mu_plane, mass):
    """The 8 gait-into-the-box states with their caches (0.5 kg: of a gait run against the light box), the box as found and
    with a twist added (|omega| <= 5, |v| <= 2), so that it slides on its ground contacts.  The box-ground pair's coefficient
    is the product of the box's and the plane's, clamped after combining: 0, 0.5, and at plane friction 6 it is 3, not
    min(2 x 6, 10) x 0.5 / 2 = 2.5."""
    out = run_box_case(oracle_mod, "free box, gait states, %g kg, plane friction %g" % (mass, mu_plane), "gait",
                       dict(obstacle_mass=mass), mu_plane, seed=int(mu_plane) + int(mass))
    assert all((d["C"][:, 4] < 0).any() for d in out), "the box stands on the ground in every state"
    mus = np.concatenate([d["r"]["mus"][d["C"][:, 4] < 0] for d in out])
    assert np.all(mus == min(0.5 * mu_plane, 10.0))
    slip = max(np.abs(d["boxref"][10:12]).max() for d in out if d["how"] == "twisted")
    assert slip > 0.1, "the twisted box slides (%g)" % slip


@pytest.mark.parametrize("motion", ["found", "twisted"])
@pytest.mark.parametrize("from_file", [0, 1])
@pytest.mark.parametrize("mass", [200.0, 0.5])
def test_free_box_beside_a_link(oracle_mod, mass, from_file, motion):
    """The box placed beside a link, as found (at rest: the small-angle branch of its integration) or twisted.  At 0.5 kg
    the box's block of M^-1 J^T dominates a link-box row, so that a wrong sign or lever arm of its part shows;
    inertia_from_file 1: the box's (1, 100, 1) (and the snake's file inertias)."""
    over = dict(obstacle_mass=mass, inertia_from_file=from_file)
    out = run_box_case(oracle_mod, "free box beside a link, %s, %g kg, inertia_from_file %d" % (motion, mass, from_file),
                       "beside", over, motion=(motion,), seed=int(mass) + from_file, set_over=dict(inertia_from_file=from_file))
    small = sum(np.linalg.norm(d["boxref"][7:10]) < 1e-3 for d in out)
    if motion == "found":
        assert small >= 1, "the third-order branch of the exponential map is met"
    else:
        assert small == 0
    pushed = max(np.abs(d["boxref"][7:13] - d["r"]["v_free"][22:]).max() for d in out)
    assert pushed > 1e-3, "the contacts move the box (%g)" % pushed


BOX_SWITCHES = {"cone_friction 0": dict(cone_friction=0), "friction_directions 1": dict(friction_directions=1),
                "contact_erp_rule 1": dict(contact_erp_rule=1)}


@pytest.mark.parametrize("mass", [200.0, 0.5])
@pytest.mark.parametrize("switch", list(BOX_SWITCHES))
def test_free_box_switches(oracle_mod, switch, mass):
    over = dict(BOX_SWITCHES[switch], obstacle_mass=mass)
    run_box_case(oracle_mod, "free box beside a link, %g kg, %s" % (mass, switch), "beside", over, motion=("twisted",),
                 seed=20 + int(mass) + len(switch), set_over={})


@pytest.mark.parametrize("mass", [200.0, 0.5])
def test_free_box_warm_start(oracle_mod, mass):
    """warm_start 1 on gait states run under it: the box's own ground contacts start at the impulses of its cached points
    (np_manifold.update_box), like the snake's."""
    over = dict(warm_start=1, obstacle_mass=mass)
    S, T, M, BS, BM = box_set(oracle_mod, "gait", **over)
    assert np.abs(BM[:, 7::7]).max() > 1e-4, "the box's cache carries impulses"
    run_box_case(oracle_mod, "free box, gait states, %g kg, warm start" % mass, "gait", over, seed=30 + int(mass))


def test_free_box_free_fall(oracle_mod):
    """Snake and box in the air, no contact: the box's free motion alone -- the gyroscopic term, the k + k|.| damping on
    omega and v, gravity -- and its integration."""
    out = run_box_case(oracle_mod, "free box in free fall", "air", {}, motion=("twisted",), seed=40, min_link_box=0.0)
    assert all(d["nc"] == 0 for d in out)
    for d in out:                                   # the gyroscopic term is not small against the bound
        assert np.abs(d["boxref"][7:10]).max() > 0.5


def test_free_box_velocity_clamp(oracle_mod):
    """Every box velocity component at +-99.5 ... 100: max_coord_vel clamps v + a dt and v_free + dv per component, and the
    angular motion limit of pi / 4 per substep holds the rotation."""
    out = run_box_case(oracle_mod, "free box at the velocity clamp", "beside", {}, motion=("clamp",), seed=50)
    at = sum(int((np.abs(d["boxref"][7:13]) == 100.0).sum()) + int((np.abs(d["r"]["v_free"][22:]) == 100.0).sum()) for d in out)
    assert at >= len(out), at
