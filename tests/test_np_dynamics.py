"""The reference of the dynamics queries, validated on the CPU (tests/np_dynamics.py: what the GPU tests of snk_dynamics and
snk_jacobians compare with): its velocity-product accelerations against the differentiated Jacobians, the power identity,
gravity and momentum against np_model, the whole of M du/dt + h = Q against the oracle's forward dynamics, and the float32
twin against it."""
import numpy as np
import pytest

import np_dynamics as nd_
import np_model as npm
from conftest import random_state
from np_link_states import split_state

NS = (2, 16, 32)
STEP = 1e-5


def states(n, seed):
    rng = np.random.default_rng(seed + n)
    return [random_state(rng, n, z=0.3, qamp=1.5, vamp=1.0) for _ in range(8)]


@pytest.mark.parametrize("n", NS)
def test_velocity_product_accelerations_are_the_derivative_of_J_u_along_the_flow(n):
    """(a) The analytic (a_com, alpha) of every link equal the central difference of (Jv u, Jw u) along the flow of the
    state at FIXED u (pos + v t, quat <- exp(omega t) (x) quat, q + qd t), step 1e-5, to 1e-6 x the largest component:
    truncation is O(step^2) and round-off O(1e-16 / step), both below that."""
    for s in states(n, 3100):
        acc = nd_.accelerations(s, n)
        tp, tm = nd_.link_twists(nd_.flow(s, n, STEP), n), nd_.link_twists(nd_.flow(s, n, -STEP), n)
        a = np.array([x[2] for x in acc])
        al = np.array([x[1] for x in acc])
        fa = np.array([(p[0] - m[0]) / (2 * STEP) for p, m in zip(tp, tm)])
        fal = np.array([(p[1] - m[1]) / (2 * STEP) for p, m in zip(tp, tm)])
        assert np.max(np.abs(a - fa)) < 1e-6 * np.max(np.abs(a)), (np.max(np.abs(a - fa)), np.max(np.abs(a)))
        assert np.max(np.abs(al - fal)) < 1e-6 * np.max(np.abs(al)), (np.max(np.abs(al - fal)), np.max(np.abs(al)))
        # and the twists themselves are the recursion's omega
        assert np.allclose(np.array([x[0] for x in acc]), np.array([t[1] for t in nd_.link_twists(s, n)]), atol=1e-12)


@pytest.mark.parametrize("n", NS)
def test_power_identity(n):
    """(b) With no force acting the kinetic energy stays: u^T h_velocity = 1/2 u^T (dM/dt) u, dM/dt from the same flow
    difference, to 1e-6 x the largest of the two sides' terms."""
    links = npm.build_tree(n)
    for s in states(n, 3200):
        u = split_state(s, n)[2]
        _, h = nd_.reference(s, n, nd_.VELOCITY)
        Ms = []
        for t in (STEP, -STEP):
            f = nd_.flow(s, n, t)
            Ms.append(npm.mass_matrix(links, f[0:3], f[3:7], f[13:13 + n]))
        Md = (Ms[0] - Ms[1]) / (2 * STEP)
        lhs, rhs = u @ h, 0.5 * u @ Md @ u
        scale = max(np.max(np.abs(u * h)), np.max(np.abs(0.5 * u[:, None] * Md * u[None, :])))
        assert abs(lhs - rhs) < 1e-6 * scale, (lhs, rhs, scale)


@pytest.mark.parametrize("n", NS)
def test_gravity_and_momentum_against_np_model(n):
    """(c) h_gravity is minus np_model.gravity_force, exactly; M[0:6] u is np_model.momentum -- linear, and angular about
    the root origin -- to 1e-12; 1/2 u^T M u its kinetic energy."""
    links = npm.build_tree(n)
    for s in states(n, 3300):
        pos, quat, u, q = split_state(s, n)
        M, hg = nd_.reference(s, n, nd_.GRAVITY)
        assert np.array_equal(hg, -npm.gravity_force(links, pos, quat, q))
        P, Lw, K = npm.momentum(links, pos, quat, q, u)
        assert np.max(np.abs(M[3:6] @ u - P)) < 1e-12
        assert np.max(np.abs(M[0:3] @ u - (Lw - np.cross(pos, P)))) < 1e-12
        assert abs(0.5 * u @ M @ u - K) < 1e-12 * max(1.0, K)
        # flags 3 is the sum of its parts in exact arithmetic
        _, h1 = nd_.reference(s, n, nd_.VELOCITY)
        _, h3 = nd_.reference(s, n, 3)
        assert np.max(np.abs(h3 - (h1 + hg))) < 1e-12 * max(1.0, np.max(np.abs(h3)))


@pytest.mark.parametrize("n", NS)
def test_equation_of_motion_against_the_oracle(oracle_mod, n):
    """(d) M a + h = [0 (6), tau] for a = the oracle's forward dynamics (gravity, no damping), to 1e-7.  The oracle's
    base acceleration is CLASSICAL (oracle/snake_oracle.cpp, base_acc_world: spatial + omega x v of the origin, rotated
    to the world), which is this model's du/dt: nothing to convert."""
    e = oracle_mod.OracleEnv(n_modules=n)
    rng = np.random.default_rng(3400 + n)
    for s in states(n, 3400):
        e.set_state(s)
        tau = rng.normal(size=n) * 0.1
        acc = e.forward_dynamics(tau, gravity=True, damping=False)
        M, h = nd_.reference(s, n, 3)
        Q = np.concatenate([np.zeros(6), tau])
        assert np.max(np.abs(M @ acc + h - Q)) < 1e-7, np.max(np.abs(M @ acc + h - Q))


@pytest.mark.parametrize("n", NS)
def test_twin_restates_the_reference(n):
    """(e) In float64 the twin's formulas reproduce the reference to 1e-12 (relative to the largest entry); in float32 it
    stays a float32-sized distance away."""
    for s in states(n, 3500)[:3]:
        pts = nd_.gate_points(n)[-3:]
        M, h = nd_.reference(s, n, 3)
        M2, h2, J2 = nd_.twin(s, n, 3, np.float64, pts)
        assert np.max(np.abs(M2 - M)) < 1e-12 * np.max(np.abs(M)) and np.max(np.abs(h2 - h)) < 1e-12 * max(1.0, np.max(np.abs(h)))
        for (r, l), j in zip(pts, J2):
            assert np.max(np.abs(j - nd_.jacobian(s, n, r, l))) < 1e-12
        s32 = np.asarray(s, np.float32)
        M, h = nd_.reference(s32, n, 3)
        M3, h3, _ = nd_.twin(s32, n, 3, np.float32)
        em, eh = np.max(np.abs(M3 - M)) / np.max(np.abs(M)), np.max(np.abs(h3 - h)) / np.max(np.abs(h))
        print("  twin n=%d: float32 M %.2e, h %.2e of the largest entry" % (n, em, eh))
        assert 1e-9 < em < 1e-5 and 1e-9 < eh < 1e-4


@pytest.mark.parametrize("n", [16, 32])
def test_twin_is_ten_times_inside_the_caps_on_the_gate_states(n):
    """(e) On the 24 states of the GPU gate (tests/test_gpu_dynamics.py) the float32 twin alone is at least ten times inside
    every hard cap: 1e-4 normalised for M, 1e-3 of the block's largest component for h and J.  The figures printed here
    are where that test's floors come from."""
    ref = nd_.references(n)
    tw = ref["twin"]
    fig = nd_.figures(n, ref["S"], tw["M"], tw["H"], tw["J"], ref)
    for k in sorted(fig):
        err, big = fig[k]
        cap = 1e-4 if big is None else 1e-3 * big
        print("  twin n=%d: %-22s %.3e   (cap %.3e)" % (n, k, err, cap))
        assert err < 0.1 * cap, (k, err, cap)
