"""The applied forces on the GPU (include/snk.h, "The applied forces": snk_apply_impulse; csrc/snk_dyn.hpp: impulse_kernel):
delta = T x M^-1 Q against the independent float64 model of tests/np_impulse.py (validated on the CPU by
tests/test_np_impulse.py), gated by the float32 twin of the kernel's recursion; agreement with the handle's own Jacobians;
the exact structure of what is written and what is not; the substep that follows against the oracle; momentum over 20
substeps; the refusals of both forms; and a captured graph of a push and a substep against the same calls run eagerly.
Five envs, envs 2 and 4 masked off, over the three kernel variants."""
import contextlib
import os

import numpy as np
import pytest

import np_dynamics as nd_
import np_impulse as ni
from conftest import f32_gate, random_state

pytestmark = pytest.mark.gpu

# variant -> (n_modules, SNK_FORCE_STREAMED): Lds<16, true>, Lds<16, false>, Lds<32, false> (snk_seam.hpp: for_variant)
VARIANTS = {"16": (16, False), "16s": (16, True), "32": (32, False)}
E = ni.ENVS
MASK = ni.MASK
ON = [e for e in range(E) if MASK[e]]
OFF = [e for e in range(E) if not MASK[e]]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@contextlib.contextmanager
def stepper(pkg, n_envs, n, streamed=False, **over):
    """A handle; `streamed`: created under SNK_FORCE_STREAMED=1 (read at snk_create), the variable put back after."""
    old = os.environ.get("SNK_FORCE_STREAMED")
    if streamed:
        os.environ["SNK_FORCE_STREAMED"] = "1"
    else:
        os.environ.pop("SNK_FORCE_STREAMED", None)
    try:
        st = pkg.Stepper(n_envs, n_modules=n, **over)
    finally:
        if old is None:
            os.environ.pop("SNK_FORCE_STREAMED", None)
        else:
            os.environ["SNK_FORCE_STREAMED"] = old
    try:
        yield st
    finally:
        st.close()


def vel_slices(n):
    """the velocity floats of snk_get_state: u = [omega, v | qd]"""
    return slice(7, 13), slice(13 + n, 13 + 2 * n)


def state_u(S, n):
    a, b = vel_slices(n)
    return np.concatenate([S[..., a], S[..., b]], axis=-1)


def snapshots_equal_but(before, after, n, envs_velocity_may_differ):
    """every field of two Snapshots byte-equal, but for the velocity floats of `state` in the named envs"""
    for f in before.FIELDS:
        a, b = getattr(before, f), getattr(after, f)
        assert (a is None) == (b is None), f
        if a is None:
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, f
        if f == "state" and len(envs_velocity_may_differ):
            a, b = a.copy(), b.copy()
            for s in vel_slices(n):
                a[envs_velocity_may_differ, s] = 0
                b[envs_velocity_may_differ, s] = 0
        assert a.tobytes() == b.tobytes(), f


FACTOR = 1.5      # conftest.f32_gate's factor, here for both chain lengths


def tensors(world, c):
    t = world.torch
    dev = world.device
    return (t.tensor(c["gen_force"], device=dev), t.tensor(c["rows"], device=dev), t.tensor(c["wrenches"], device=dev),
            t.tensor(MASK, device=dev))


# ----------------------------------------------------------------------------------------------------------------------
# 1. accuracy, and the exact structure of every call along the way
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_delta_matches_the_model_and_only_the_velocity_is_written(pkg, variant):
    """Per frame (world, link) and point count (1, 5, 9: the staging passes of four wrap): the dry call and the writing
    call return the same bits; the dry call leaves every table of the Snapshot byte-equal, the writing call everything but
    the velocity floats of the active envs, which become float32(u) + float32(delta) bit for bit; a masked env's delta is
    zeros.  The error of delta against the float64 model, of the row's largest component, and the conditioning-free M64
    delta - T Q of |T Q|, go through f32_gate with the float32 twin's figure on the same inputs as the yardstick, np_impulse's
    floors (the twin's worst over the gate's cases) and ten times them as the hard caps.  The host form gives the device
    form's bits."""
    n, streamed = VARIANTS[variant]
    ok = True
    with stepper(pkg, E, n, streamed) as st:
        world = pkg.DeviceWorld(stepper=st)
        t = world.torch
        st.reset()
        k = np.arange(st.act_dim)
        for j in range(2):      # (so that the contact cache and the aux floats hold something)
            st.step((-0.9 * np.sin((2 * k[None, :] + 1) * 4.0 + 0.2 * j + 0.37 * np.arange(E)[:, None])).astype(np.float32))
        for frame in ("world", "link"):
            for P in ni.POINT_COUNTS:
                c = ni.gate_case(n, P, frame)
                gf, rows, wr, mask = tensors(world, c)
                st.set_state(c["S"], None)
                before = st.snapshot()
                dry = world.impulse_response(gf, rows, wr, frame=frame, duration=c["T"], active=mask)
                t.cuda.synchronize()
                snapshots_equal_but(before, st.snapshot(), n, [])
                out = t.full((E, n + 6), -7.0, dtype=t.float32, device=world.device)
                assert world.apply_forces(gf, rows, wr, frame=frame, duration=c["T"], active=mask, out=out) is out
                t.cuda.synchronize()
                after = st.snapshot()
                snapshots_equal_but(before, after, n, ON)
                delta = out.cpu().numpy()
                assert same_bits(delta, dry.cpu().numpy()) and np.all(np.isfinite(delta))
                assert np.all(bits(delta[OFF]) == 0) and np.all(np.abs(delta[ON]).max(axis=1) > 0)
                assert same_bits(state_u(after.state, n)[ON], (state_u(before.state, n) + delta)[ON])
                # the host form: the same bits, from the same state
                st.set_state(c["S"], None)
                hd = st.apply_impulse(c["gen_force"], c["rows"], c["wrenches"], flags=ni.LINK_FRAME if frame == "link" else 0,
                                      seconds=c["T"], active=MASK)
                assert same_bits(hd, delta) and same_bits(st.get_state()[0], after.state)
                what = "impulse %s %s frame %d points" % (variant, frame, P)
                ok &= f32_gate(what + ": delta", ni.delta_error(delta, c, ON), ni.delta_error(c["twin"], c, ON),
                               factor=FACTOR, floor=ni.FLOOR_DELTA[n], cap=10 * ni.FLOOR_DELTA[n])
                ok &= f32_gate(what + ": M64 delta - T Q", ni.residual_error(delta, c, ON), ni.residual_error(c["twin"], c, ON),
                               factor=FACTOR, floor=ni.FLOOR_RESIDUAL[n], cap=10 * ni.FLOOR_RESIDUAL[n])
    assert ok


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_wrenches_agree_with_the_handles_own_jacobians(pkg, variant):
    """A call with world wrenches at the links' COMs (snk_link_states' own float32 COMs) against the call with gen_force =
    sum_p J_p^T [f ; tau] formed in torch from snk_jacobians: the two deltas differ by float32 round-off -- the same gate as
    the accuracy -- and gen_force plus wrenches in one call is their sum's delta.  An all-zero Q gives delta == 0 and leaves
    the state equal as values; a link row outside 0 .. 3n + 1 contributes nothing on the device path and is refused on the
    host path."""
    n, streamed = VARIANTS[variant]
    c = ni.gate_case(n, 5, "world")
    with stepper(pkg, E, n, streamed) as st:
        world = pkg.DeviceWorld(stepper=st)
        t = world.torch
        st.set_state(c["S"], None)
        gf, rows, wr, mask = tensors(world, c)
        ls = world.link_states()                                  # [E, 3n + 2, 16]
        wr = wr.clone()
        wr[:, :, 6:9] = ls[:, rows.long(), 0:3]
        J = world.jacobians(rows)                                 # [E, P, 6, nd]
        Q = t.einsum("epkd,epk->ed", J, wr[:, :, 0:6])
        a = world.impulse_response(None, rows, wr, duration=c["T"]).cpu().numpy()
        b = world.impulse_response(Q, duration=c["T"]).cpu().numpy()
        both = world.impulse_response(gf, rows, wr, duration=c["T"]).cpu().numpy()
        summed = world.impulse_response(gf + Q, duration=c["T"]).cpu().numpy()
        for what, x, y in (("wrenches against J^T w", a, b), ("gen_force + wrenches against their sum", both, summed)):
            d = max(float(np.max(np.abs(x[e].astype(np.float64) - y[e])) / np.max(np.abs(y[e]))) for e in range(E))
            f32_gate("impulse %s: %s" % (variant, what), d, ni.delta_error(c["twin"], c), factor=FACTOR,
                     floor=ni.FLOOR_DELTA[n], cap=10 * ni.FLOOR_DELTA[n])
        # nothing applied
        before = st.get_state()[0]
        z = t.full((E, n + 6), -7.0, dtype=t.float32, device=world.device)
        world.apply_forces(t.zeros_like(gf), rows, t.zeros_like(wr), out=z)
        t.cuda.synchronize()
        assert np.all(z.cpu().numpy() == 0) and np.array_equal(st.get_state()[0], before)
        # rows outside the tree
        bad = t.tensor([-1, int(c["rows"][0]), 3 * n + 2], dtype=t.int32, device=world.device)
        w3 = wr[:, :3].contiguous()
        w3[:, 1] = wr[:, 0]
        got = world.impulse_response(None, bad, w3, duration=c["T"]).cpu().numpy()
        want = world.impulse_response(None, rows[:1], wr[:, :1].contiguous(), duration=c["T"]).cpu().numpy()
        assert same_bits(got, want)
        with pytest.raises(RuntimeError, match=r"snk_apply_impulse_host: link_rows\[2\] = %d is outside 0 \.\. %d" % (3 * n + 2, 3 * n + 1)):
            st.apply_impulse(None, [0, 1, 3 * n + 2], np.zeros((E, 3, 9), np.float32))


# ----------------------------------------------------------------------------------------------------------------------
# 2. the next step reads what was written
# ----------------------------------------------------------------------------------------------------------------------
def rel_vel_error(G, ref, n):
    """tests/test_gpu_parity.py's figure: worst |dv| / (1 + |v|) over the base's six and the joints' rates"""
    dv = np.abs(G[13 + n:] - ref[13 + n:]) / (1.0 + np.abs(ref[13 + n:]))
    dw = np.abs(G[7:13] - ref[7:13]) / (1.0 + np.abs(ref[7:13]))
    return max(dv.max(), dw.max())


@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("case", ["air", "ground"])
def test_the_next_substep_reads_what_was_written(pkg, oracle_mod, case, n):
    """apply_forces for dt, then one snk_substep_host, against the float64 oracle stepped from u + delta_ref (the float64
    model's delta) -- tests/test_gpu_parity.py's single-substep yardstick: the relative velocity error per env, its median
    over the envs within 1.5 x the float32 pipeline's on the same inputs (the float32 twin's delta, then the oracle built in
    float32; floor 1e-6), the worst values within 2 x, as there.  ground: snakes lying on the plane, default motors, a 10 N
    sideways push on the head's COM.  air: 1 m up, max_motor_impulse = 0 (motors off: TORQUE_CONTROL), joint torques only.
    16 envs, envs 2 and 4 masked off: they step from u."""
    B = 16
    rng = np.random.default_rng(900 + n + (1 if case == "air" else 0))
    over = dict(residual_threshold=0.0)
    if case == "air":
        over["max_motor_impulse"] = 0.0
    S = np.zeros((B, 13 + 2 * n))
    for i in range(B):
        if case == "air":
            S[i] = random_state(rng, n, z=1.0, qamp=0.5, vamp=0.5)
        else:
            S[i] = random_state(rng, n, z=0.026, qamp=0.3, vamp=0.3, flat=True)
            S[i, 7:10] *= 0.1
    S32 = S.astype(np.float32)
    targets = rng.uniform(-0.5, 0.5, (B, n)).astype(np.float32)
    mask = np.ones(B, np.uint8)
    mask[[2, 4]] = 0
    head = 3 * n + 1
    dt = float(np.float32(1.0 / 240.0))
    gf = W = rows = None
    if case == "air":
        gf = np.zeros((B, n + 6), np.float32)
        gf[:, 6:] = rng.uniform(-0.1, 0.1, (B, n))
    else:
        rows = np.array([head], np.int32)
        W = np.zeros((B, 1, 9), np.float32)
        W[:, 0, 1] = 10.0                                     # LINK_FRAME: 10 N along the head's own y, at its COM
    st = pkg.Stepper(B, n_modules=n, **over)
    try:
        st.set_state(S32, None)
        st.apply_impulse(gf, rows, W, flags=ni.LINK_FRAME, seconds=dt, active=mask)
        info = st.substep(targets, 1)
        G = st.get_state()[0].astype(np.float64)
    finally:
        st.close()
    o64 = oracle_mod.OracleEnv(n_modules=n, **over)
    o32 = oracle_mod.OracleEnv(f32=True, n_modules=n, **over)
    e_gpu, e_f32, q_gpu, q_f32 = [], [], 0.0, 0.0
    for i in range(B):
        s64 = S32[i].astype(np.float64)
        s32 = s64.copy()
        if mask[i]:
            args = (None if gf is None else gf[i], [] if rows is None else rows, [] if W is None else W[i], True)
            Q = ni.gen_force_of(S32[i], n, *args)
            d64 = ni.reference(S32[i], n, Q, dt)[0]
            d32 = ni.twin(S32[i], n, *args, T=dt, dtype=np.float32).astype(np.float64)
            for s, d in ((s64, d64), (s32, d32)):
                s[7:13] += d[0:6]
                s[13 + n:] += d[6:]
        o64.hard_reset()
        o64.set_state(s64)
        o64.substep(targets[i].astype(np.float64))
        ref = o64.get_state()
        assert info[i, 1] == o64.last_num_contacts, (i, info[i], o64.last_num_contacts)
        o32.hard_reset()
        o32.set_state(s32)
        o32.substep(targets[i].astype(np.float64))
        r32 = o32.get_state()
        e_gpu.append(rel_vel_error(G[i], ref, n))
        e_f32.append(rel_vel_error(r32, ref, n))
        q_gpu = max(q_gpu, np.abs(G[i, :7] - ref[:7]).max(), np.abs(G[i, 13:13 + n] - ref[13:13 + n]).max())
        q_f32 = max(q_f32, np.abs(r32[:7] - ref[:7]).max(), np.abs(r32[13:13 + n] - ref[13:13 + n]).max())
    what = "impulse then substep [%s n=%d]" % (case, n)
    print("  %s: worst rel velocity GPU %.3e, float32 pipeline %.3e; worst |dq| GPU %.3e, float32 pipeline %.3e"
          % (what, max(e_gpu), max(e_f32), q_gpu, q_f32))
    ok = f32_gate(what + " rel velocity median of %d" % B, np.median(e_gpu), np.median(e_f32), 1.5, 1e-6)
    # ... and that test's gates on the worst values, with its factor for them
    ok &= f32_gate(what + " worst |dq|", q_gpu, q_f32, 2.0, 1e-6)
    ok &= f32_gate(what + " worst rel velocity", max(e_gpu), max(e_f32), 2.0, 1e-5)
    assert ok


# ----------------------------------------------------------------------------------------------------------------------
# 3. momentum, end to end
# ----------------------------------------------------------------------------------------------------------------------
def momenta(world, n):
    """(linear momentum [E, 3], angular momentum about the world origin [E, 3]) float64 from world.dynamics()' M and the state"""
    M = world.mass_matrix().cpu().numpy().astype(np.float64)
    S = world.stepper.get_state()[0].astype(np.float64)
    u = state_u(S, n)
    lin = np.einsum("eij,ej->ei", M[:, 3:6], u)
    ang = np.einsum("eij,ej->ei", M[:, 0:3], u) + np.cross(S[:, 0:3], lin)
    return lin, ang


@pytest.mark.parametrize("n", [16, 32])
def test_momentum_over_twenty_substeps(pkg, n):
    """No gravity, no damping, motors off, 1 m up: a constant world force at a link's COM before each of 20 single substeps
    makes the linear momentum M[3:6] u grow by k f dt; a pure torque on a link leaves it alone and makes the angular momentum
    about the world origin grow by k tau dt.  Gate: 1.5 x the drift of the same momentum over the same 20 substeps with
    nothing applied, plus 20 x the float32 twin's per-call error in the same units (|M64 twin_delta - dt Q| over the rows
    of that momentum, at the first call's state) -- both measured here and printed.  Measured (MI355X): the free drift is
    the integrator's own -- explicit Euler on a tumbling chain does not conserve momentum: 3e-2 kg m/s over 20 substeps at
    16 links, 2.4e-1 at 32, next to k f dt of 4.2e-2 -- so this gate is loose, and each call is ALSO checked on its own, where
    the integrator has no say (jump_error)."""
    K = 20
    over = dict(gravity_z=0.0, lin_damping=0.0, ang_damping=0.0, joint_damping=0.0, max_motor_impulse=0.0)
    S0 = nd_.gate_states(n)[:E].copy()
    S0[:, 2] = 1.0
    S0[:, 7:13] *= 0.2
    S0[:, 13 + n:] *= 0.2
    row = 3 * (n // 2) + 1                                      # a cylinder link mid-chain
    f, tau = np.array([0.5, -0.3, 0.2]), np.array([0.02, 0.03, -0.01])
    with stepper(pkg, E, n, **over) as st:
        world = pkg.DeviceWorld(stepper=st)
        t = world.torch
        dt = float(np.float32(st.params.dt))
        targets = t.zeros((E, n), dtype=t.float32, device=world.device)
        rows = t.tensor([row], dtype=t.int32, device=world.device)

        jumps = []

        def jump_error(before, after, W9):
            """One call on its own, where the integrator has no say: M (u_after - u_before) over the rows of the momenta (about
            the world origin) against dt x the wrench's force and moment, M from the handle; returned with its bound -- the
            float32 twin's worst residual of the gate's cases (np_impulse.FLOOR_RESIDUAL, of |dt Q|) plus what rounding the
            stored sums u + delta to float32 can move (half an ulp of each, through |M|) -- as (error, bound), worst env."""
            M = world.mass_matrix().cpu().numpy().astype(np.float64)
            worst = (0.0, 0.0)
            for e in range(E):
                du = state_u(after[e], n) - state_u(before[e], n)
                ulp = np.abs(M[e]) @ (np.abs(state_u(after[e], n)) * 2.0 ** -24)
                o0, x, fw, tw = before[e, 0:3], W9[e, 0, 6:9].astype(np.float64), W9[e, 0, 0:3], W9[e, 0, 3:6]
                lin = M[e, 3:6] @ du
                ang = M[e, 0:3] @ du + np.cross(o0, lin)
                err = max(np.abs(lin - dt * fw).max(), np.abs(ang - dt * (tw + np.cross(x, fw))).max())
                Q = ni.gen_force_of(before[e], n, None, [row], W9[e])
                bound = ni.FLOOR_RESIDUAL[n] * dt * np.abs(Q).max() + ulp[0:6].max() * (1.0 + np.abs(o0).sum())
                if err / bound > worst[0] / (worst[1] or 1.0):
                    worst = (err, bound)
            return worst

        def run(wrench):
            """the momenta after each of K (push, substep) pairs, minus the initial ones: [K, E, 3] each"""
            st.set_state(S0, None)
            l0, a0 = momenta(world, n)
            lin, ang = [], []
            W = None
            if wrench is not None:
                W = t.zeros((E, 1, 9), dtype=t.float32, device=world.device)
                W[:, 0, 0:6] = t.tensor(wrench, dtype=t.float32, device=world.device)
            for _ in range(K):
                if W is not None:
                    W[:, 0, 6:9] = world.link_states()[:, row, 0:3]      # the link's COM now
                    before = st.get_state()[0].astype(np.float64)
                    world.apply_forces(None, rows, W)
                    jumps.append(jump_error(before, st.get_state()[0].astype(np.float64), W.cpu().numpy()))
                world.step_simulation(targets, k=1)
                l, a = momenta(world, n)
                lin.append(l - l0)
                ang.append(a - a0)
            return np.array(lin), np.array(ang)

        free_l, free_a = run(None)
        drift_l, drift_a = np.abs(free_l).max(), np.abs(free_a).max()
        # the twin's per-call error, in momentum units, at the first call's state
        tw_l = tw_a = 0.0
        for e in range(E):
            J = nd_._kin64(S0[e], n)[3]
            for wrench, kind in ((np.concatenate([f, np.zeros(3)]), "f"), (np.concatenate([np.zeros(3), tau]), "t")):
                w9 = np.concatenate([wrench, J[row][2]]).astype(np.float32)[None]
                Q = ni.gen_force_of(S0[e], n, None, [row], w9)
                M = ni.reference(S0[e], n, Q, dt)[1]
                r = M @ ni.twin(S0[e], n, None, [row], w9, False, dt, np.float32).astype(np.float64) - dt * Q
                if kind == "f":
                    tw_l = max(tw_l, np.abs(r[3:6]).max())
                else:
                    tw_l, tw_a = max(tw_l, np.abs(r[3:6]).max()), max(tw_a, np.abs(r[0:3]).max())
        print("  impulse momentum n=%d: free drift over %d substeps linear %.3e, angular %.3e kg m/s, kg m^2/s; twin per call linear "
              "%.3e, angular %.3e" % (n, K, drift_l, drift_a, tw_l, tw_a))
        lim_l, lim_a = 1.5 * drift_l + K * tw_l, 1.5 * drift_a + K * tw_a
        ks = np.arange(1, K + 1)[:, None, None]
        push_l, _ = run(np.concatenate([f, np.zeros(3)]))
        err = np.abs(push_l - ks * dt * f).max()
        print("  impulse momentum n=%d: force: linear momentum against k f dt: worst %.3e (limit %.3e; k f dt reaches %.3e)"
              % (n, err, lim_l, K * dt * np.abs(f).max()))
        ok = err < lim_l
        twist_l, twist_a = run(np.concatenate([np.zeros(3), tau]))
        err_l, err_a = np.abs(twist_l).max(), np.abs(twist_a - ks * dt * tau).max()
        print("  impulse momentum n=%d: torque: linear momentum worst %.3e (limit %.3e), angular against k tau dt worst %.3e (limit "
              "%.3e; k tau dt reaches %.3e)" % (n, err_l, lim_l, err_a, lim_a, K * dt * np.abs(tau).max()))
        err_j, bound_j = max(jumps, key=lambda eb: eb[0] / eb[1])
        print("  impulse momentum n=%d: one call alone, M (u_after - u_before) against dt x wrench: worst %.3e of its bound %.3e "
              "(over %d calls)" % (n, err_j, bound_j, len(jumps)))
        assert ok and err_l < lim_l and err_a < lim_a and err_j < bound_j


# ----------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals_of_both_forms(pkg):
    n, nd = 16, 22
    lib = pkg._lib
    with stepper(pkg, E, n) as st:
        world = pkg.DeviceWorld(stepper=st)
        t = world.torch
        dev = world.device
        gf = t.zeros((E, nd), dtype=t.float32, device=dev)
        rows = t.tensor([1, 4], dtype=t.int32, device=dev)
        wr = t.zeros((E, 2, 9), dtype=t.float32, device=dev)
        out = t.zeros((E, nd), dtype=t.float32, device=dev)
        imp = st.apply_impulse_device
        g, r, w, o = gf.data_ptr(), rows.data_ptr(), wr.data_ptr(), out.data_ptr()
        hz = np.zeros((E, nd), np.float32)
        hw = np.zeros((E, 2, 9), np.float32)

        def with_nan(a, idx):
            a = a.copy()
            a[idx] = np.nan
            return a

        for msg, f in (
                ("snk_apply_impulse: flags has bits other than", lambda: imp(0, g, 0, 0, 0, 4, 0.1, o)),
                ("snk_apply_impulse: n_points -1 is outside 0 .. 256", lambda: imp(0, g, r, w, -1, 0, 0.1, o)),
                ("snk_apply_impulse: n_points 257 is outside 0 .. 256", lambda: imp(0, g, r, w, 257, 0, 0.1, o)),
                ("snk_apply_impulse: null link_rows with n_points 2", lambda: imp(0, g, 0, w, 2, 0, 0.1, o)),
                ("snk_apply_impulse: null wrench with n_points 2", lambda: imp(0, g, r, 0, 2, 0, 0.1, o)),
                ("snk_apply_impulse: gen_force is null and n_points is 0", lambda: imp(0, 0, r, w, 0, 0, 0.1, o)),
                ("snk_apply_impulse: null delta with SNK_IMPULSE_DRY", lambda: imp(0, g, 0, 0, 0, lib.IMPULSE_DRY, 0.1, 0)),
                ("snk_apply_impulse: seconds must be finite and not negative", lambda: imp(0, g, 0, 0, 0, 0, -0.1, o)),
                ("snk_apply_impulse: seconds must be finite and not negative", lambda: imp(0, g, 0, 0, 0, 0, float("nan"), o)),
                ("snk_apply_impulse: seconds must be finite and not negative", lambda: imp(0, g, 0, 0, 0, 0, float("inf"), o)),
                ("snk_apply_impulse: gen_force_dev, link_rows_dev, wrench_dev and delta_dev must be 4-byte aligned",
                 lambda: imp(0, g + 2, 0, 0, 0, 0, 0.1, o)),
                ("snk_apply_impulse_host: flags has bits other than", lambda: st.apply_impulse(hz, flags=8)),
                ("snk_apply_impulse_host: n_points 257 is outside 0 .. 256",
                 lambda: st.apply_impulse(None, [1] * 257, np.zeros((E, 257, 9), np.float32))),
                ("snk_apply_impulse_host: gen_force is null and n_points is 0", lambda: st.apply_impulse()),
                ("snk_apply_impulse_host: seconds must be finite and not negative", lambda: st.apply_impulse(hz, seconds=-1.0)),
                (r"snk_apply_impulse_host: link_rows\[1\] = 50 is outside 0 \.\. 49", lambda: st.apply_impulse(None, [0, 50], hw)),
                (r"snk_apply_impulse_host: link_rows\[0\] = -1 is outside 0 \.\. 49", lambda: st.apply_impulse(None, [-1, 0], hw)),
                (r"snk_apply_impulse_host: gen_force\[3\]\[7\] is not finite", lambda: st.apply_impulse(with_nan(hz, (3, 7)))),
                (r"snk_apply_impulse_host: wrench\[1\]\[1\]\[2\] is not finite",
                 lambda: st.apply_impulse(None, [1, 4], with_nan(hw, (1, 1, 2)))),
                (r"snk_apply_impulse_host: wrench\[0\]\[0\]\[8\] is not finite",
                 lambda: st.apply_impulse(None, [1, 4], with_nan(hw, (0, 0, 8))))):
            with pytest.raises(RuntimeError, match=msg):
                f()
        # a masked env's rows are not read: a NaN there is not refused, and nothing of it arrives
        d = st.apply_impulse(with_nan(hz + 1, (2, 7)), active=MASK)
        assert np.all(np.isfinite(d)) and np.all(d[OFF] == 0)
        # null handles; the host form's null delta with DRY
        for msg, rc in (
                ("snk_apply_impulse: null handle", lambda: st.lib.snk_apply_impulse(None, None, g, None, None, 0, 0, 0.1, o, None)),
                ("snk_apply_impulse_host: null handle",
                 lambda: st.lib.snk_apply_impulse_host(None, None, lib.fptr(hz), None, None, 0, 0, 0.1, None)),
                ("snk_apply_impulse_host: null delta with SNK_IMPULSE_DRY",
                 lambda: st.lib.snk_apply_impulse_host(st.h, None, lib.fptr(hz), None, None, 0, lib.IMPULSE_DRY, 0.1, None))):
            assert rc() != 0
            assert msg in lib.last_error(), (msg, lib.last_error())
        # DeviceWorld: shape, dtype and argument mistakes are ValueErrors
        with pytest.raises(ValueError, match="gen_force must have shape"):
            world.apply_forces(t.zeros((E, nd + 1), dtype=t.float32, device=dev))
        with pytest.raises(ValueError, match="gen_force must be torch.float32"):
            world.apply_forces(gf.double())
        with pytest.raises(ValueError, match="wrenches must have shape"):
            world.apply_forces(None, rows, t.zeros((E, 3, 9), dtype=t.float32, device=dev))
        with pytest.raises(ValueError, match="link_rows without wrenches"):
            world.apply_forces(None, rows)
        with pytest.raises(ValueError, match="nothing to apply"):
            world.apply_forces()
        with pytest.raises(ValueError, match="frame must be"):
            world.apply_forces(gf, frame="body")
        with pytest.raises(ValueError, match="0 .. 256 points"):
            world.apply_forces(None, [1] * 257, t.zeros((E, 257, 9), dtype=t.float32, device=dev))
        with pytest.raises(ValueError, match="out must have shape"):
            world.impulse_response(gf, out=t.zeros((E, nd + 1), dtype=t.float32, device=dev))
        with pytest.raises(ValueError, match="active must have shape"):
            world.apply_forces(gf, active=t.zeros(E + 1, dtype=t.uint8, device=dev))
        assert world.apply_forces(gf) is None
        # a poisoned handle: both forms refuse with the scheduler's message; close() still works
        calls = (lambda: imp(0, g, r, w, 2, 0, 0.1, o), lambda: st.apply_impulse(hz))
        for f in calls:
            f()
        t.cuda.synchronize()
        st.debug_raise_alarm()
        for f in calls:
            with pytest.raises(RuntimeError, match="env-step scheduler: a bounded wait ran out"):
                f()
    assert st.h is None


# ----------------------------------------------------------------------------------------------------------------------
# 5. stream order
# ----------------------------------------------------------------------------------------------------------------------
def test_captured_graph_equals_the_eager_calls(pkg):
    """apply_forces + step_simulation(k=1) captured once into a torch.cuda.graph (one stream, no parallel branches; the
    handle warmed up by the same pair before the capture) and replayed three times, against the same three pairs run
    eagerly from the same state: every state float bit for bit."""
    n = 16
    c = ni.gate_case(n, 5, "link")
    with stepper(pkg, E, n) as st:
        world = pkg.DeviceWorld(stepper=st)
        t = world.torch
        gf, rows, wr, mask = tensors(world, c)
        targets = t.tensor(np.random.default_rng(3).uniform(-0.5, 0.5, (E, n)).astype(np.float32), device=world.device)
        S0 = c["S"].copy()
        S0[:, 2] = 1.0

        def pair():
            world.apply_forces(gf, rows, wr, frame="link", active=mask)
            world.step_simulation(targets, k=1)

        st.set_state(S0, None)
        pair()                                                    # warm-up: nothing is allocated under the capture
        t.cuda.synchronize()
        st.set_state(S0, np.zeros((E, n + 2), np.float32))
        start = st.snapshot()
        for _ in range(3):
            pair()
        t.cuda.synchronize()
        eager = st.snapshot()
        graph = t.cuda.CUDAGraph()
        with t.cuda.graph(graph):
            pair()
        t.cuda.synchronize()
        st.restore(start)                                         # (a capture runs nothing; every table is put back anyway)
        for _ in range(3):
            graph.replay()
        t.cuda.synchronize()
        replayed = st.snapshot()
        assert not np.array_equal(eager.state, start.state)
        snapshots_equal_but(eager, replayed, n, [])
