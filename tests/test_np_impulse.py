"""The float64 model of the applied forces (tests/np_impulse.py) on the CPU: against the oracle's independent M^-1
(its ABA delta pass), the identities the contract implies, the size of the deviation from Bullet's one-pass form, the float32
twin of the kernel's recursion -- whose figures are the floors of the GPU gate, tests/test_gpu_impulse.py -- and the new
entry points of the cross-compiled library, which refuse a null handle by name."""
import numpy as np
import pytest

import np_dynamics as nd_
import np_impulse as ni
from np_link_states import split_state


def _random_call(rng, S, n, P=4):
    """(gen_force [nd], rows [P], world wrenches [P, 9]) with points near the links' COMs"""
    J = nd_._kin64(S, n)[3]
    gf = np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-5, 5, 3), rng.uniform(-0.2, 0.2, n)])
    rows = rng.integers(0, 3 * n + 2, P)
    W = np.concatenate([rng.uniform(-10, 10, (P, 3)), rng.uniform(-0.5, 0.5, (P, 3)), rng.uniform(-0.05, 0.05, (P, 3))], axis=1)
    for p, r in enumerate(rows):
        W[p, 6:9] += J[r][2]
    return gf, rows, W


@pytest.mark.parametrize("n", [16, 32])
def test_model_agrees_with_the_oracles_minv(oracle_mod, n):
    """(a) delta = T x solve(M, Q), M and J from np_dynamics / np_model, against the oracle's minv_mul -- an articulated-body
    delta pass that shares no code with them -- to 1e-9 of the largest component, on the gate's 24 states; and the float64
    twin of the kernel's recursion reproduces the same."""
    rng = np.random.default_rng(77 + n)
    e = oracle_mod.OracleEnv(n_modules=n)
    T = 1.0 / 240.0
    worst, worst_twin = 0.0, 0.0
    for S in nd_.gate_states(n):
        gf, rows, W = _random_call(rng, S, n)
        Q = ni.gen_force_of(S, n, gf, rows, W)
        delta, _ = ni.reference(S, n, Q, T)
        e.set_state(S.astype(np.float64))
        orc = T * e.minv_mul(Q)
        worst = max(worst, np.max(np.abs(delta - orc)) / np.max(np.abs(orc)))
        tw = ni.twin(S, n, gf, rows, W, False, T, np.float64)
        worst_twin = max(worst_twin, np.max(np.abs(tw - delta)) / np.max(np.abs(delta)))
    print("  impulse n=%d: model against the oracle's minv_mul %.3e, float64 twin against the model %.3e (of the largest component)"
          % (n, worst, worst_twin))
    assert worst < 1e-9 and worst_twin < 1e-9


@pytest.mark.parametrize("n", [16, 32])
def test_identities(n):
    """(b) M[3:6] delta = T sum f; M[0:3] delta = T sum ((x - o_0) x f + tau); a LINK_FRAME wrench is the rotated WORLD_FRAME
    one; a link row named twice is the summed wrench -- each to float64 round-off."""
    rng = np.random.default_rng(5 + n)
    T = 1.0 / 240.0
    for S in nd_.gate_states(n)[:6]:
        links, Rw, ow, J = nd_._kin64(S, n)[:4]
        _, rows, W = _random_call(rng, S, n)
        Q = ni.gen_force_of(S, n, None, rows, W)
        delta, M = ni.reference(S, n, Q, T)
        f_sum = W[:, 0:3].sum(axis=0)
        m_sum = sum(np.cross(w[6:9] - ow[0], w[0:3]) + w[3:6] for w in W)
        scale_f, scale_m = np.abs(W[:, 0:3]).sum() * T, (np.abs(W[:, 0:3]).sum() + np.abs(W[:, 3:6]).sum()) * T
        assert np.max(np.abs(M[3:6] @ delta - T * f_sum)) < 1e-11 * scale_f
        assert np.max(np.abs(M[0:3] @ delta - T * m_sum)) < 1e-11 * scale_m
        # the same wrenches stated in the links' COM frames
        WL = np.array([np.concatenate([Rw[r].T @ w[0:3], Rw[r].T @ w[3:6], Rw[r].T @ (w[6:9] - J[r][2])]) for r, w in zip(rows, W)])
        QL = ni.gen_force_of(S, n, None, rows, WL, link_frame=True)
        assert np.max(np.abs(QL - Q)) < 1e-12 * np.max(np.abs(Q))
        # one row twice, at one point: the summed wrench
        r, x = int(rows[0]), W[0, 6:9]
        two = np.array([np.concatenate([W[0, 0:6], x]), np.concatenate([W[1, 0:6], x])])
        one = np.concatenate([W[0, 0:6] + W[1, 0:6], x])[None]
        assert np.max(np.abs(ni.gen_force_of(S, n, None, [r, r], two) - ni.gen_force_of(S, n, None, [r], one))) < 1e-12 * np.max(np.abs(Q))
        # a row outside the tree contributes nothing
        assert np.array_equal(ni.gen_force_of(S, n, None, [-1, 3 * n + 2], W[:2]), np.zeros(n + 6))


def _with_velocity(S, n, u):
    s = np.array(S, np.float64)
    s[7:13] = u[0:6]
    s[13 + n:] = u[6:]
    return s


def _split_deviation(S, n, dt):
    """(|difference|_inf, |Bullet-form velocity change|_inf) of one unconstrained step: u + dt M^-1 (Q - h(u)) against the
    kick form u' + dt M^-1 (-h(u')), u' = u + dt M^-1 Q; a 10 N sideways push on the head's COM and 0.1 N m on a mid joint"""
    J = nd_._kin64(S, n)[3]
    head = 3 * n + 1
    W = np.concatenate([[0.0, 10.0, 0.0], np.zeros(3), J[head][2]])[None]
    gf = np.zeros(n + 6)
    gf[6 + n // 2] = 0.1
    Q = ni.gen_force_of(S, n, gf, [head], W)
    pos, quat, u, q = split_state(np.asarray(S, np.float64), n)
    M, h = nd_.reference(S, n, nd_.VELOCITY | nd_.GRAVITY)
    bullet = u + dt * np.linalg.solve(M, Q - h)
    u1 = u + dt * np.linalg.solve(M, Q)
    h1 = nd_.reference(_with_velocity(S, n, u1), n, nd_.VELOCITY | nd_.GRAVITY)[1]
    kick = u1 + dt * np.linalg.solve(M, -h1)
    return np.max(np.abs(kick - bullet)), np.max(np.abs(bullet - u))


@pytest.mark.parametrize("n", [16, 32])
def test_splitting_deviation_is_second_order(n):
    """(c) What applying the force in front of the step, instead of inside its ABA pass, changes: dt M^-1 (h(u) - h(u + delta)),
    delta = dt M^-1 Q.  A measurement (DESIGN.md 3 quotes the printed figures), gated only in its order.  h is a quadratic
    form in u, so the deviation is exactly A dt^2 + B dt^3 (A from dh/du delta, B from the term quadratic in delta): halving dt
    divides a component by 4 where the first term carries it and by up to 8 where the second does -- a 10 N push on a 40 g
    head is 60 rad/s of delta at the tip joints, next to u of 1.  Asserted: the median ratio over the states within 3.5 .. 4.5,
    every state's within 3 .. 8."""
    dt = 1.0 / 240.0
    worst, worst_half, rel, ratios = 0.0, 0.0, 0.0, []
    for S in nd_.gate_states(n)[:8]:
        d1, c1 = _split_deviation(S, n, dt)
        d2, _ = _split_deviation(S, n, dt / 2)
        worst, worst_half, rel = max(worst, d1), max(worst_half, d2), max(rel, d1 / c1)
        ratios.append(d1 / d2)
    print("  impulse n=%d: kick form against Bullet's one-pass form, dt = 1/240: worst |du| %.3e rad/s or m/s, %.3e of the step's "
          "own velocity change; at dt / 2: %.3e; ratio per state %s, median %.2f"
          % (n, worst, rel, worst_half, " ".join("%.2f" % r for r in ratios), np.median(ratios)))
    assert 3.5 < np.median(ratios) < 4.5 and all(3.0 < r < 8.0 for r in ratios), ratios


@pytest.mark.parametrize("n", [16, 32])
def test_float32_twin_against_the_model(n):
    """(d) The recursion the kernel uses, in float32 over the unmerged tree, on the GPU gate's own inputs: its error against
    (a) per case, and that the floors tests/test_gpu_impulse.py takes from np_impulse hold the worst of them."""
    worst_d, worst_r = 0.0, 0.0
    for frame in ("world", "link"):
        for P in ni.POINT_COUNTS:
            c = ni.gate_case(n, P, frame)
            d, r = ni.delta_error(c["twin"], c), ni.residual_error(c["twin"], c)
            print("  impulse twin n=%d %s frame %d points: delta %.3e of the row's largest component, M delta - T Q %.3e of |T Q|"
                  % (n, frame, P, d, r))
            worst_d, worst_r = max(worst_d, d), max(worst_r, r)
    print("  impulse twin n=%d: worst delta %.3e (floor %.1e), worst residual %.3e (floor %.1e)"
          % (n, worst_d, ni.FLOOR_DELTA[n], worst_r, ni.FLOOR_RESIDUAL[n]))
    assert worst_d <= ni.FLOOR_DELTA[n] < 1.1 * worst_d and worst_r <= ni.FLOOR_RESIDUAL[n] < 1.1 * worst_r


def test_entry_points_exist_and_refuse_a_null_handle_by_name(pkg):
    """(e) snk_apply_impulse and snk_apply_impulse_host are exported by the cross-compiled library and refuse a null handle,
    each under its own name, before anything else is looked at; the constants of _lib.py are the header's."""
    lib = pkg.load()
    _lib = pkg._lib
    assert lib.snk_apply_impulse(None, None, None, None, None, 0, 0, 0.0, None, None) != 0
    assert "snk_apply_impulse: null handle" in _lib.last_error()
    assert lib.snk_apply_impulse_host(None, None, None, None, None, 0, 0, 0.0, None) != 0
    assert "snk_apply_impulse_host: null handle" in _lib.last_error()
    assert (_lib.IMPULSE_LINK_FRAME, _lib.IMPULSE_DRY, _lib.WRENCH_FLOATS, _lib.IMPULSE_MAX_POINTS) == (1, 2, 9, 256)
    assert (ni.LINK_FRAME, ni.DRY) == (_lib.IMPULSE_LINK_FRAME, _lib.IMPULSE_DRY)
    assert hasattr(pkg.DeviceWorld, "apply_forces") and hasattr(pkg.DeviceWorld, "impulse_response")
    assert hasattr(pkg.Stepper, "apply_impulse")
