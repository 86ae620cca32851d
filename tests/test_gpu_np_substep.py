"""The HIP kernels against tests/np_substep.py (the float64 numpy model written from the rules) at the edges the other
GPU tests do not reach: ground friction 0 and above 5 (mu clamped at 10), velocities at the max_coord_vel clamp, joints
past both limits, folded snakes, the static box, cone_friction 0, friction_directions 1 -- on the register-resident
solve, the streamed-row solve (SNK_FORCE_STREAMED) and the 32-link chain.

One substep through the C ABI (set_state / set_manifold / substep(T, 1)) from float32 inputs; the numpy model runs on
the same float32-rounded inputs and the contacts the float64 oracle solved.  Contact and iteration counts must equal the
oracle's (residual_threshold 0, as test_single_substep_parity; the oracle with the kernels' room for link-link / box
contacts, max_self_contacts 32, as tests/test_obstacle.py runs it) -- except the iteration count at the velocity clamp,
where it is a round-off decision (test_velocity_clamp says why).  The yardstick of every gate is the float32 oracle's
distance to the numpy model on the same states (conftest.f32_gate: median 1.5 x, 90th percentile 2 x with the floors
1e-6 / 1e-5 of the single-substep parity test; the worst single value of a heavy-tailed sample 2 x or 5 % of a velocity,
the rule DESIGN.md 3 states for test_substep_parity_under_contact_switch).

Cases where the kernels sit further from the model than the float32 oracle does are kept as STRICT xfails with the
measured figure in their reason (open findings): they are tracked, and a fix turns them into failures
until the mark is removed.
"""
import numpy as np
import pytest

import np_manifold as nm
import np_substep as ns
from conftest import f32_gate, random_state

pytestmark = pytest.mark.gpu

def _ground(rng, n, B, qamp=0.3, vamp=0.3):
    S = np.zeros((B, 13 + 2 * n))
    for i in range(B):
        S[i] = random_state(rng, n, z=0.026, qamp=qamp, vamp=vamp, flat=True)
        S[i, 9] *= 0.1
        S[i, 7:9] *= 0.1
    return S


def _rel(x, ref, n):
    return max((np.abs(x[13 + n:] - ref[13 + n:]) / (1 + np.abs(ref[13 + n:]))).max(),
               (np.abs(x[7:13] - ref[7:13]) / (1 + np.abs(ref[7:13]))).max())


def _run(pkg, oracle_mod, name, n, S, T, over=None, mu=None, M=None, check_iters=True):
    """GPU, float64 oracle (contacts, counts) and float32 oracle from the same float32 inputs; per env the relative
    velocity and motor-torque errors of the GPU and of the float32 oracle against the numpy model."""
    over = dict(over or {})
    B = len(S)
    S32 = np.asarray(S, np.float32)
    T32 = np.asarray(T, np.float32)
    st = pkg.Stepper(B, n_modules=n, **over)
    if mu is not None:
        st.set_ground_friction(np.full(B, mu, np.float32))
    st.set_state(S32)
    if M is not None:
        st.set_manifold(np.asarray(M, np.float32))
    info = st.substep(T32, 1)
    G, GX = st.get_state()
    st.close()
    mirror = dict(max_contacts=0, max_self_contacts=32)
    o = oracle_mod.OracleEnv(n_modules=n, **mirror, **over)
    o32 = oracle_mod.OracleEnv(n_modules=n, f32=True, **mirror, **over)
    ev, ev32, et, et32, ncs = [], [], [], [], 0
    for i in range(B):
        s64, t64 = S32[i].astype(np.float64), T32[i].astype(np.float64)
        for e in (o, o32):
            e.hard_reset()
            e.set_plane_friction(1.0 if mu is None else float(np.float32(mu)))
            if M is not None:
                e.set_manifold(np.asarray(M[i], np.float32).astype(np.float64))
            e.set_state(s64)
            e.substep(t64)
        C = o.last_contacts_full()
        assert info[i, 1] == o.last_num_contacts == len(C), (name, i, info[i], len(C))
        if check_iters:
            assert info[i, 0] == o.last_iterations, (name, i, info[i], o.last_iterations)
        lam0 = None
        if over.get("warm_start"):
            # the impulse every ground contact starts from: the cache model on the same float32-rounded cache
            lam0 = nm.update_env(o.params, s64, np.asarray(M[i], np.float32).astype(np.float64))["contacts"][:, 5]
            assert len(lam0) == (C[:, 5] == -1).sum(), (name, i, len(lam0), len(C))
            lam0 = np.concatenate([lam0, np.zeros(len(C) - len(lam0))])
        r = ns.substep(o.params, s64, t64, C, mu_plane=1.0 if mu is None else float(np.float32(mu)), lam0=lam0)
        x = r["state"]
        sc = max(1.0, np.abs(r["tau_motor"]).max())
        ev.append(_rel(G[i].astype(np.float64), x, n))
        ev32.append(_rel(o32.get_state(), x, n))
        et.append(np.abs(GX[i, :n] - r["tau_motor"]).max() / sc)
        et32.append(np.abs(o32.get_aux()[0] - r["tau_motor"]).max() / sc)
        ncs += len(C)
    print("  [%s] %d envs, %d contacts, iterations %s" % (name, B, ncs, sorted(set(info[:, 0]))))
    ev, ev32, et, et32 = map(np.array, (ev, ev32, et, et32))
    for what, g, f in (("velocity", ev, ev32), ("motor torque", et, et32)):
        f32_gate("np model %s: %s median of %d" % (name, what, B), np.median(g), np.median(f), 1.5, 1e-6)
        f32_gate("np model %s: %s p90" % (name, what), np.percentile(g, 90), np.percentile(f, 90), 2.0, 1e-5)
        f32_gate("np model %s: %s worst" % (name, what), g.max(), f.max(), 2.0, 5e-2)
    return ncs


PATHS = [("register-resident", 16, False), ("streamed-row", 16, True), ("32 links", 32, False)]


def _open(reason):
    return pytest.mark.xfail(strict=True, raises=AssertionError, reason="open (DESIGN.md 3): " + reason)


def _path(monkeypatch, path):
    _, n, streamed = next(p for p in PATHS if p[0] == path)
    if streamed:
        monkeypatch.setenv("SNK_FORCE_STREAMED", "1")
    return n, streamed


GROUND = [("register-resident", "default"), ("streamed-row", "default"), ("32 links", "default"),
          pytest.param("register-resident", "cone_friction 0",
                       marks=_open("worst velocity 0.125 against the float32 oracle's 0.031 (4.0 x) over 128 states "
                                   "(sweep ladder, tests/test_gpu_np_sweeps.py: passes at 1, 2, 3 sweeps, first fails "
                                   "at 5 -- one state 0.20 against 1.0e-4 --, passes at 10; the model's own spread "
                                   "under one-ulp input noise at 50 sweeps is 6.1e-7 at worst: not a bifurcation, "
                                   "open from sweep 5)")),
          pytest.param("streamed-row", "cone_friction 0",
                       marks=_open("worst velocity 9.8 against the float32 oracle's 0.24 (41 x) over 128 states "
                                   "(sweep ladder, tests/test_gpu_np_sweeps.py: first fails at sweep 1, p90 4.8e-5 "
                                   "against 2.0e-5 (2.4 x), as the streamed-row solve does under every friction "
                                   "setting, mu 0 included; the model's own spread at 50 sweeps 1.1e-5 at worst: open "
                                   "from sweep 1)")),
          pytest.param("32 links", "cone_friction 0",
                       marks=_open("worst velocity 7.5 against the float32 oracle's 0.21 (36 x) over 64 states (sweep "
                                   "ladder, tests/test_gpu_np_sweeps.py: 8 states pass at 1 ... 25 sweeps, so it "
                                   "first fails between 26 and 50; the model's own spread at 50 sweeps 1.7e-6 at "
                                   "worst: amplification that one-ulp input noise does not explain, open)")),
          ("register-resident", "friction_directions 1"),
          pytest.param("streamed-row", "friction_directions 1",
                       marks=_open("velocity p90 3.7e-4 against the float32 oracle's 1.5e-4 (2.4 x) over 128 states "
                                   "(sweep ladder, tests/test_gpu_np_sweeps.py: passes at 1, first fails at 2 sweeps, "
                                   "p90 1.3e-4 against 3.3e-5 (4.0 x); the model's own spread at 50 sweeps 9.7e-7 "
                                   "at worst: open from sweep 2)")),
          ("32 links", "friction_directions 1")]


@pytest.mark.parametrize("path,switch", GROUND)
def test_ground_states_per_path(pkg, oracle_mod, monkeypatch, path, switch):
    n, streamed = _path(monkeypatch, path)
    over = dict(residual_threshold=0.0)
    over.update({"default": {}, "cone_friction 0": dict(cone_friction=0),
                 "friction_directions 1": dict(friction_directions=1)}[switch])
    rng = np.random.default_rng(1100 + n + 7 * streamed + 13 * len(switch))
    B = 128 if n == 16 else 64
    _run(pkg, oracle_mod, "%s, %s" % (path, switch), n, _ground(rng, n, B), rng.uniform(-0.5, 0.5, (B, n)), over)


@pytest.mark.parametrize("path,mu", [("register-resident", 0.0), ("register-resident", 6.0), ("streamed-row", 0.0),
                                     ("streamed-row", 6.0), ("32 links", 0.0),
                                     pytest.param("32 links", 6.0, marks=_open(
                                         "motor-torque median 3.3e-5 against the float32 oracle's 1.8e-5 (1.8 x) "
                                         "(sweep ladder, tests/test_gpu_np_sweeps.py: passes at 1, 2, 3, first fails "
                                         "at 5 sweeps, motor-torque p90 6.7e-5 against 2.2e-5 (3.0 x); the model's "
                                         "own velocity "
                                         "spread under one-ulp input noise at 50 sweeps: median 4.2e-5, worst 5.0e-2 "
                                         "-- the tail is a "
                                         "bifurcation, the median is not: open from sweep 5)"))])
def test_ground_friction_edges(pkg, oracle_mod, monkeypatch, path, mu):
    """mu = 2 x mu_plane: 0 (a zero cone radius) and 12, clamped at 10 (fminf(mu_link * mu_plane, 10))."""
    n, streamed = _path(monkeypatch, path)
    rng = np.random.default_rng(1200 + n + 7 * streamed + int(mu))
    B = 128 if n == 16 else 64
    _run(pkg, oracle_mod, "%s, plane friction %g" % (path, mu), n, _ground(rng, n, B, vamp=1.0),
         rng.uniform(-0.5, 0.5, (B, n)), dict(residual_threshold=0.0), mu=mu)


@pytest.mark.parametrize("path", ["register-resident", pytest.param("streamed-row", marks=_open(
    "worst velocity 0.39 against the float32 oracle's 0.14 (2.9 x) over 96 states (sweep ladder, "
    "tests/test_gpu_np_sweeps.py: 16 states pass at 1 ... 25 sweeps; the model's own spread at 50 sweeps 1.7e-6 at "
    "worst: a heavy tail of 96 states, open)")), "32 links"])
def test_velocity_clamp(pkg, oracle_mod, monkeypatch, path):
    """Weak motors (max_motor_impulse 0.05) and qd near +-100, in the air and on the ground: max_coord_vel clamps v + "
    "a dt
    and v_free + dv.  Velocities and torques are gated; the iteration count is not compared.  With every motor but one
    or two at its bound, the sweep's residual falls geometrically (1e4, 5e2, 1e-5, 1e-10, 6e-18, 5e-23 in (dI/dinv)^2)
    and the exit waits for it to be EXACTLY zero, i.e. for the last free motor's update to vanish in its accumulator's
    rounding: a round-off decision -- on one of these states the two float64 programs themselves stop at sweep 7 (numpy)
    and 8 (oracle), and float32 gets there sooner.  Once there nothing moves, so the velocities do not depend on it."""
    n, streamed = _path(monkeypatch, path)
    rng = np.random.default_rng(1300 + n + 7 * streamed)
    B = 96 if n == 16 else 48
    S = np.zeros((B, 13 + 2 * n))
    for i in range(B):
        S[i] = random_state(rng, n, z=1.0 if i % 2 else 0.026, qamp=0.3, vamp=0.3, flat=i % 2 == 0)
        S[i, 13 + n:] = rng.choice([-1, 1], n) * rng.uniform(99.5, 100.0, n)
    _run(pkg, oracle_mod, "%s, velocity clamp" % path, n, S, rng.uniform(-0.5, 0.5, (B, n)),
         dict(residual_threshold=0.0, max_motor_impulse=0.05), check_iters=False)


@pytest.mark.parametrize("path", [p[0] for p in PATHS])
def test_joints_past_both_limits(pkg, oracle_mod, monkeypatch, path):
    n, streamed = _path(monkeypatch, path)
    rng = np.random.default_rng(1400 + n + 7 * streamed)
    B = 96 if n == 16 else 48
    S = _ground(rng, n, B)
    for i in range(B):
        S[i, 13:13 + n] = rng.choice([-1, 1], n) * rng.uniform(1.575, 1.8, n) * (rng.uniform(size=n) < 0.4)
    _run(pkg, oracle_mod, "%s, past the limits" % path, n, S, rng.uniform(-0.5, 0.5, (B, n)),
         dict(residual_threshold=0.0))


def test_folded_snakes(pkg, oracle_mod):
    """16 links folded onto themselves: link-link two-body rows (the streamed-row solve takes these substeps)."""
    rng = np.random.default_rng(1500)
    e = oracle_mod.OracleEnv()
    S = []
    while len(S) < 24:
        s = _ground(rng, 16, 1, qamp=1.7)[0]
        e.set_state(s.astype(np.float32).astype(np.float64))
        C = e.contacts_full()
        if len(C) and (C[:, 5] >= 0).sum() >= 2:
            S.append(s)
    _run(pkg, oracle_mod, "16 links folded", 16, np.array(S), rng.uniform(-0.5, 0.5, (len(S), 16)),
         dict(residual_threshold=0.0))


@_open("contact count of env 10: 33 on the GPU against the oracle's 35")
def test_static_box(pkg, oracle_mod):
    """obstacle 1: gait states pushed into the box, handed over with their contact caches."""
    from bench import gait_actions
    BOX = dict(obstacle=1, obstacle_pos=[0.100, 0.0, 0.1])
    rng = np.random.default_rng(1600)
    e = oracle_mod.OracleEnv(**BOX)
    S, M = [], []
    for i in range(12):
        e.hard_reset()
        e.reset()
        for j in range(8 + i % 6):
            e.env_step(gait_actions(np.array([i + 1]), j)[0], vec_mode=True)
        S.append(e.get_state())
        M.append(e.get_manifold())
    nc = _run(pkg, oracle_mod, "16 links against the static box", 16, np.array(S), rng.uniform(-0.5, 0.5, (12, 16)),
              dict(BOX, residual_threshold=0.0), M=np.array(M))
    assert nc > 12


@pytest.mark.parametrize("path", [p[0] for p in PATHS])
def test_warm_start(pkg, oracle_mod, monkeypatch, path):
    """warm_start 1: states of a short gait run handed over with their caches, whose points carry non-zero impulses;
    the normal rows start at warmstarting_factor x those (np_substep's lam0, from the cache model np_manifold).

    State 6 of the 16-link runs is not such a state: its episode ended in the fourth env-step, so it is the reset pose
    itself (straight snake, zero velocity, 32 fresh points, every start impulse 0).  There the float32 oracle and the
    kernels sit 1.17 (under the torques drawn for the register-resident case) and 4.6e-2 (under the streamed-row
    case's) of a velocity from the model, alike: the roll rate about the long axis, which 32 collinear contact pairs leave to friction alone.  The model's
    own spread on that state under additive input noise of one float32 ulp is 1.0e-4 / 5.6e-5 at worst (3e-12 under
    1e-15), so by the rule of tests/test_np_substep.py it is no bifurcation of the model: it is float32 arithmetic
    inside the 50 sweeps, which oracle and kernels share; on the other eleven states the float32 oracle is within
    7.3e-4 of the model."""
    from bench import gait_actions
    n, streamed = _path(monkeypatch, path)
    rng = np.random.default_rng(1650 + n + 7 * streamed)
    e = oracle_mod.OracleEnv(n_modules=n, warm_start=1)
    S, M = [], []
    for i in range(12 if n == 16 else 8):
        e.hard_reset()
        e.reset()
        for j in range(3 + i % 5):
            e.env_step(gait_actions(np.array([i + 1]), j, e.act_dim)[0], vec_mode=True)
        S.append(e.get_state())
        M.append(e.get_manifold())
    assert np.abs(np.array(M)[:, :, 7::7]).max() > 1e-4
    _run(pkg, oracle_mod, "%s, warm start" % path, n, np.array(S), rng.uniform(-0.5, 0.5, (len(S), n)),
         dict(residual_threshold=0.0, warm_start=1), M=np.array(M))


@pytest.mark.parametrize("path", [p[0] for p in PATHS[:2]] + [pytest.param("32 links", marks=_open(
    "velocity median 4.1e-2 against the float32 oracle's 1.8e-4 (230 x) over 8 states (sweep ladder, "
    "tests/test_gpu_np_sweeps.py: the same states fail at 64 sweeps, median 1.9 x and p90 109 x, and at 128 the "
    "median is 4.2e-2 against 4.0e-3; the "
    "model's own spread under one-ulp input noise: worst 8.9e-7 at 64 sweeps, p90 1.5 / worst 4.8 at 128 -- the tail "
    "is a "
    "bifurcation from 128 sweeps on, the median, spread 2.8e-6, is not: open from sweep 64)"))])
def test_converged_solve(pkg, oracle_mod, monkeypatch, path):
    """1000 sweeps without the residual exit, a handful of ground states per path, gated the same way.  Observed on 16
    links: GPU and float32 oracle equally far from the model (ratios 0.4-1.3), and no closer than at 50 sweeps -- 1000
    sweeps do not reach the fixed point of these stiff solves."""
    n, streamed = _path(monkeypatch, path)
    rng = np.random.default_rng(1700 + n + 7 * streamed)
    B = 8
    _run(pkg, oracle_mod, "%s, 1000 sweeps" % path, n, _ground(rng, n, B), rng.uniform(-0.5, 0.5, (B, n)),
         dict(residual_threshold=0.0, n_iterations=1000))
