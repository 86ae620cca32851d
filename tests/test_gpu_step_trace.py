"""The traced step (snk_step_traced): test mode's per-substep telemetry (snake.py:275-293, SnakeGymEnv.py:43-44) written
by the fused step kernel itself, one row per physics substep: [observation | link positions | padding].

What is pinned here: a traced step computes what the plain step computes, bit for bit; every row is, bit for bit, what
the single-substep path gives for that substep (set_state / set_manifold, substep(targets, 1), get_obs, link_positions);
rows at and beyond an env's substep count and every row's padding are never written (the buffers start as NaNs); the
in-launch schedule does not show; the rows agree with the reference's own recording within the float32 tolerance; the
Python seams hand out the same infos from the kernel's rows as from the replay."""
import os

import numpy as np
import pytest

from conftest import f32_gate, mismatch_gate

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def gait(pkg, B, j, A):
    import importlib
    syn = importlib.import_module("bullet-envs_amd.synthetic")
    return np.ascontiguousarray(syn.gait_actions(np.arange(B), j, A), dtype=np.float32)


def _family(monkeypatch, streamed, quantum="1"):
    monkeypatch.setenv("SNK_QUANTUM", quantum)
    if streamed:
        monkeypatch.setenv("SNK_FORCE_STREAMED", "1")
    else:
        monkeypatch.delenv("SNK_FORCE_STREAMED", raising=False)


def _payload(n):
    return (3 * n + 8) + 3 * (n + 1)


def _check_shape_of_a_trace(trace, sub, n):
    """rows < sub[i]: payload written (finite), padding NaN; rows >= sub[i]: NaN from end to end"""
    B, R, W = trace.shape
    written = np.arange(R)[None, :] < sub[:, None]
    assert np.isnan(trace[~written]).all()
    assert np.isfinite(trace[written][:, :_payload(n)]).all()
    assert np.isnan(trace[written][:, _payload(n):]).all()


def _targets(a, n, gait_sel, scaling):
    t = np.zeros((len(a), n), dtype=np.float32)
    if gait_sel == 0:
        t[:, 0::2] = a
    elif gait_sel == 1:
        t[:, 1::2] = a
    else:
        t[:, :] = a
    return t * np.float32(scaling)


# ------------------------------------------------------------------------------------------------------------------
# 1. a traced step changes nothing
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,streamed,B", [(16, False, 64), (16, True, 64), (32, False, 32)])
def test_traced_step_changes_nothing(pkg, monkeypatch, n, streamed, B):
    _family(monkeypatch, streamed)
    plain, traced = pkg.Stepper(B, n_modules=n), pkg.Stepper(B, n_modules=n)
    plain.reset(); traced.reset()
    for j in range(3):
        a = gait(pkg, B, j, n // 2) * np.float32(1.2)          # some components get clipped in place
        a2 = a.copy()
        o, r, d, s = plain.step(a)
        o2, r2, d2, s2, tr = traced.step_traced(a2)
        assert tr.shape == (B, 41, 128 if n == 16 else 224) and tr.dtype == np.float32
        assert np.array_equal(o, o2) and np.array_equal(r, r2) and np.array_equal(d, d2) and np.array_equal(s, s2)
        assert np.array_equal(a, a2)
        for x, y in zip(plain.get_state(), traced.get_state()):
            assert np.array_equal(x, y)
        assert np.array_equal(plain.get_manifold(), traced.get_manifold())
        _check_shape_of_a_trace(tr, s2, n)
    assert s.max() > 10
    plain.close(); traced.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. the trace is the replay
# ------------------------------------------------------------------------------------------------------------------
REPLAY_CASES = [
    ("register-resident", 16, False, {}),
    ("streamed-16", 16, True, {}),
    ("links-32", 32, False, {}),
    ("contact_order-2", 16, False, dict(contact_order=2)),
    ("rules", 16, False, dict(noncontact_order=1, contact_erp_rule=1)),
    ("free-box", 16, False, dict(obstacle=2)),
    ("gait-2", 16, False, dict(gait=2)),
]


@pytest.mark.parametrize("name,n,streamed,over", REPLAY_CASES, ids=[c[0] for c in REPLAY_CASES])
def test_trace_is_the_replay(pkg, monkeypatch, name, n, streamed, over):
    _family(monkeypatch, streamed)
    B = 16
    A = n if over.get("gait") == 2 else n // 2
    st = pkg.Stepper(B, n_modules=n, **over)
    sc = pkg.Stepper(B, n_modules=n, **over)               # the existing path: one substep per launch
    st.reset()
    free_box = over.get("obstacle") == 2
    mu = (0.6 + np.arange(B) % 5 / 5.0).astype(np.float32)
    st.set_ground_friction(mu); sc.set_ground_friction(mu)
    no = 3 * n + 8
    compared = 0
    for j in range(2):
        S, X = st.get_state()
        M = st.get_manifold()
        box = st.get_box() if free_box else None
        a = gait(pkg, B, j, A)
        obs, rew, done, sub, tr = st.step_traced(a, vec_mode=True)
        _check_shape_of_a_trace(tr, sub, n)
        sc.set_state(S, X); sc.set_manifold(M)
        if free_box:
            sc.set_box(*box)
        T = _targets(a, n, st.params.gait, st.params.scaling_factor)       # (a: clipped in place by the step)
        for s_ in range(int(sub.max())):
            sc.substep(T, 1)
            o, lp = sc.get_obs(), sc.link_positions()
            live = sub > s_
            assert np.array_equal(tr[live, s_, :no], o[live]), (name, j, s_)
            assert np.array_equal(tr[live, s_, no:no + 3 * (n + 1)], lp[live]), (name, j, s_)
            compared += int(live.sum())
        for i in range(B):
            if sub[i] and not done[i]:
                assert np.array_equal(tr[i, sub[i] - 1, :no], obs[i])
    assert compared > 10 * B
    st.close(); sc.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. edges of the servo loop
# ------------------------------------------------------------------------------------------------------------------
def test_zero_substeps_write_nothing(pkg, monkeypatch):
    _family(monkeypatch, False)
    B = 16
    st = pkg.Stepper(B)
    st.reset()
    obs, rew, done, sub, tr = st.step_traced(np.zeros((B, 8), dtype=np.float32))      # the pose it already has
    assert np.all(sub == 0) and np.isnan(tr).all()
    st.close()


@pytest.mark.parametrize("quantum", ["1", "0"])
def test_capped_servo_loop_fills_every_row_and_no_more(pkg, monkeypatch, quantum):
    """kp = 0.02: the servo never gets there, every env-step runs max_counter + 1 = 41 substeps.  The device form with a
    caller's buffer of 42 rows per env: the 42nd of every env (the next env's first row is right behind it) stays NaN."""
    import torch
    _family(monkeypatch, False, quantum)
    B = 48
    env = pkg.DeviceVecEnv(B, kp=0.02)
    env.reset()
    R, W = env.trace_shape()[1:]
    assert (R, W) == (41, 128)
    t = torch.full((B, R + 1, W), float("nan"), dtype=torch.float32, device="cuda")
    a = torch.tensor(gait(pkg, B, 0, 8)).cuda()
    env.step(a, trace=t)
    torch.cuda.synchronize()
    sub, tr = env.substeps.cpu().numpy(), t.cpu().numpy()
    assert np.all(sub == 41)
    assert np.isfinite(tr[:, :41, :107]).all() and np.isnan(tr[:, :41, 107:]).all()
    assert np.isnan(tr[:, 41]).all()                       # the guard rows
    env.close()


def test_max_counter_beyond_the_queue_classes(pkg, monkeypatch):
    """max_counter = 70 (the step queue has 64 priority classes), kp = 0.02: 71 rows per env, all written, by the scheduled
    and the unscheduled kernel alike."""
    B = 40
    got = []
    for quantum in ("1", "0"):
        _family(monkeypatch, False, quantum)
        st = pkg.Stepper(B, kp=0.02, max_counter=70)
        st.reset()
        assert st.trace_shape() == (B, 71, 128)
        obs, rew, done, sub, tr = st.step_traced(gait(pkg, B, 0, 8))
        live = ~done
        assert sub.max() == 71 and np.array_equal(tr[live, sub[live] - 1, :56], obs[live])
        _check_shape_of_a_trace(tr, sub, 16)
        got.append((sub, tr))
        st.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))


def test_refusals(pkg, monkeypatch):
    import torch
    _family(monkeypatch, False)
    B = 16
    env = pkg.DeviceVecEnv(B)
    env.reset()
    st = env.stepper
    a = torch.tensor(gait(pkg, B, 0, 8)).cuda()
    W = st.trace_shape()[2]
    t = torch.full((B * 42 * W + 64,), float("nan"), dtype=torch.float32, device="cuda")
    args = (a.data_ptr(), env.obs.data_ptr(), env.rew.data_ptr(), env.done.data_ptr(), env.substeps.data_ptr())
    assert t.data_ptr() % 128 == 0
    # too few rows: the message names both numbers
    with pytest.raises(RuntimeError) as ei:
        st.step_traced_device(*args, t.data_ptr(), 40)
    assert "40" in str(ei.value) and "41" in str(ei.value) and "max_counter" in str(ei.value)
    assert "41" in pkg.load().snk_last_error().decode()
    # a pointer that is not at the start of a 128-byte line
    for off in (4, 64):
        with pytest.raises(RuntimeError) as ei:
            st.step_traced_device(*args, t.data_ptr() + off, 41)
        assert "128-byte aligned" in str(ei.value)
    # no substep counts, no trace
    with pytest.raises(RuntimeError) as ei:
        st.step_traced_device(*args[:4], 0, t.data_ptr(), 41)
    assert "substeps_dev is required" in str(ei.value)
    with pytest.raises(RuntimeError):
        st.step_traced_device(*args, 0, 41)
    torch.cuda.synchronize()
    assert bool(torch.isnan(t).all())                       # nothing ran
    # ... and the handle is as good as before
    st.step_traced_device(*args, t.data_ptr(), 41)
    torch.cuda.synchronize()
    assert int(env.substeps[0]) > 0 and bool(torch.isfinite(t[:107]).all()) and bool(torch.isnan(t[107:128]).all())
    env.close()


def test_episode_that_ends_in_the_step(pkg, monkeypatch):
    """The rows of an env whose episode ends hold the step that ended it (pre-reset state: the reference clears its lists
    at the start of the next step, snake.py:276-278).  vec_mode 1 returns the post-reset observation; the last valid row
    is the terminal one: bitwise what the vec_mode 0 twin returns."""
    _family(monkeypatch, False)
    B = 16
    vec, twin = pkg.Stepper(B), pkg.Stepper(B)
    vec.reset(); twin.reset()
    ended = 0
    for j in range(8):
        a = gait(pkg, B, j, 8)               # full-amplitude gait: joint 9's target is beyond the 0.5 rad that ends an episode
        o1, r1, d1, s1, tr = vec.step_traced(a.copy(), vec_mode=True)
        o0, r0, d0, s0 = twin.step(a.copy(), vec_mode=False)
        assert np.array_equal(d1, d0) and np.array_equal(s1, s0)
        _check_shape_of_a_trace(tr, s1, 16)
        for i in np.nonzero(d1 & (s1 > 0))[0]:
            ended += 1
            last = tr[i, s1[i] - 1, :56]
            assert np.array_equal(last, o0[i]) and abs(last[9]) > 0.5
            assert np.all(o1[i, :32] == 0) and np.all(o1[i, 51:55] == [0, 0, 0, 1])     # the worker's reset()
        if ended:
            break
    assert ended > 0
    vec.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. the schedule does not show
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B", [(16, 3000), (32, 1500)])
def test_schedule_does_not_show_in_the_trace(pkg, monkeypatch, n, B):
    """Slices of 1 and 3 substeps (hand-offs between waves on all XCDs) against the unscheduled kernel: the whole trace
    is the same bits -- valid rows, and NaN everywhere else.  A row index lost at a hand-off, or a 128-byte line shared by
    two waves, would show here."""
    def run(quantum):
        _family(monkeypatch, False, str(quantum))
        st = pkg.Stepper(B, n_modules=n)
        st.reset()
        st.set_ground_friction((0.5 + np.arange(B) % 11 / 10.0).astype(np.float32))
        outs = []
        for j in range(2):
            a = gait(pkg, B, j, n // 2) * np.float32(1.2)
            o, r, d, s, tr = st.step_traced(a)
            outs.append((s, tr.view(np.uint32), o))
        st.close()
        return outs

    ref = run(0)
    for s, tr, o in ref:
        _check_shape_of_a_trace(tr.view(np.float32), s, n)
    assert max(s.max() for s, _, _ in ref) > 25 and min(s.min() for s, _, _ in ref) < 20
    for quantum in (1, 3):
        for (s, tr, o), (S, TR, O) in zip(run(quantum), ref):
            assert np.array_equal(s, S) and np.array_equal(o, O)
            assert np.array_equal(tr, TR)


# ------------------------------------------------------------------------------------------------------------------
# 5. against the reference's own recording
# ------------------------------------------------------------------------------------------------------------------
def test_rows_against_the_reference_recording(pkg, oracle_mod, monkeypatch):
    """tests/golden/env_logic_vectors.npz holds info['internal_observations'] / ['link_positions'] of four test-mode
    env-steps, recorded by running the reference's own Python.  Every row of a traced step from the recorded pre-step
    state against them; the yardstick is the float32 build of the oracle replayed from the same state."""
    _family(monkeypatch, False)
    N = 16
    d = np.load(os.path.join(HERE, "golden", "env_logic_vectors.npz"))
    v = {k: d[k] for k in d.files}
    assert len(v["telemetry_rows"]) >= 3
    gpu = dict(q=0.0, lp=0.0, qd=[])
    cal = dict(q=0.0, lp=0.0, qd=[])
    mism = mism32 = 0
    for t, i in enumerate(v["telemetry_rows"]):
        over = dict(gait=int(v["gait"][i]))
        assert over["gait"] == 1 and not np.isfinite(v["max_motor_impulse"][i])
        k_ref = int(v["substeps"][i])
        st = pkg.Stepper(1, **over)
        st.reset()
        st.set_state(v["state"][i:i + 1], v["aux"][i:i + 1])
        st.set_manifold(v["manifold"][i:i + 1])
        a = np.ascontiguousarray(v["action_in"][i:i + 1, :8], dtype=np.float32)
        obs, rew, done, sub, tr = st.step_traced(a, vec_mode=bool(v["vec_mode"][i]))
        st.close()
        mism += int(sub[0]) != k_ref
        # the float32 oracle, substep by substep from the same state (tests/test_env_logic_golden.py does this in float64)
        e = oracle_mod.OracleEnv(f32=True, **over)
        e.hard_reset()
        e.sync(v["state"][i], v["aux"][i], v["manifold"][i])
        targets = np.zeros(N)
        targets[1::2] = v["action_out"][i, :8] * e.params.scaling_factor
        k32 = e.env_step(v["action_in"][i, :8].copy(), vec_mode=bool(v["vec_mode"][i]))[3]
        mism32 += k32 != k_ref
        e.hard_reset()
        e.sync(v["state"][i], v["aux"][i], v["manifold"][i])
        for s in range(k_ref):
            o_ref, l_ref = v["internal_observations"][t, s], v["link_positions"][t, s]
            e.substep(targets)
            for fig, o, l in ((cal, e.get_obs(), e.link_com_world()[1::3][:N + 1].T.reshape(-1)),
                              (gpu, tr[0, s, :56].astype(np.float64), tr[0, s, 56:107].astype(np.float64))):
                if fig is gpu and s >= sub[0]:
                    continue
                fig["q"] = max(fig["q"], np.abs(o[:N] - o_ref[:N]).max(), np.abs(o[3 * N:3 * N + 7] - o_ref[3 * N:3 * N + 7]).max())
                fig["lp"] = max(fig["lp"], np.abs(l - l_ref).max())
                fig["qd"].append((np.abs(o[N:2 * N] - o_ref[N:2 * N]) / (1 + np.abs(o_ref[N:2 * N]))).max())
    # counts: the GPU's mismatches against the float32 oracle's, by conftest's one rule
    mismatch_gate("telemetry rows: substep counts of %d env-steps" % len(v["telemetry_rows"]), mism, mism32)
    # Four env-steps, i.e. fewer than 30 samples: factor 2.0 (DESIGN.md 3's table).  Floors and caps: those of the env-step
    # gates on the same vectors (tests/test_env_logic_golden.py); the float32 oracle's own figures on these rows are
    # worst q / pose 5.4e-3, worst link position 5.2e-3, 90th percentile of the relative velocity error 7.3e-2, so the
    # floors sit at or below what float32 itself does here and the limits are 2 x the float32 oracle's figures.
    f32_gate("telemetry rows: worst q / pose of %d rows" % len(gpu["qd"]), gpu["q"], cal["q"], 2.0, 5e-3, 2.5e-2)
    f32_gate("telemetry rows: worst link position", gpu["lp"], cal["lp"], 2.0, 5e-3, 2.5e-2)
    f32_gate("telemetry rows: rel qd p90", np.percentile(gpu["qd"], 90), np.percentile(cal["qd"], 90), 2.0, 5e-2, 0.25)


# ------------------------------------------------------------------------------------------------------------------
# 6. the seams
# ------------------------------------------------------------------------------------------------------------------
def _same_infos(a, b):
    assert type(a) is type(b) and sorted(a) == sorted(b) == ['frames', 'internal_observations', 'link_positions']
    assert a['frames'] == [] and b['frames'] == []
    for key in ('internal_observations', 'link_positions'):
        assert type(a[key]) is list and type(b[key]) is list and len(a[key]) == len(b[key])
        for x, y in zip(a[key], b[key]):
            assert type(x) is type(y) and x.dtype == y.dtype == np.float64 and x.shape == y.shape
            assert np.array_equal(x, y)


def test_vec_env_seam(pkg, monkeypatch):
    _family(monkeypatch, False)
    B = 8
    kern = pkg.SnakeVecEnv(B, mode='test', telemetry='kernel')
    repl = pkg.SnakeVecEnv(B, mode='test', telemetry='replay')
    assert pkg.SnakeVecEnv.__init__.__defaults__ is not None and repl.telemetry == 'replay'
    kern.reset(); repl.reset()
    rows = 0
    for j in range(3):
        a = gait(pkg, B, j, 8)
        ok, rk, dk, ik = kern.step(a)
        orr, rr, dr, ir = repl.step(a)
        assert np.array_equal(ok, orr) and np.array_equal(rk, rr) and np.array_equal(dk, dr)
        assert isinstance(ik, tuple) and len(ik) == len(ir) == B
        for x, y, k in zip(ik, ir, kern.last_substeps):
            _same_infos(x, y)
            assert len(x['internal_observations']) == k
            rows += k
    assert rows > 100
    assert kern._scratch is None and repl._scratch is not None          # no second handle behind the kernel's rows
    kern.close(); repl.close()
    with pytest.raises(ValueError):
        pkg.SnakeVecEnv(2, mode='test', telemetry='host')


def test_single_env_seam(pkg, monkeypatch):
    _family(monkeypatch, False)

    class Args:
        alpha, beta, gamma = 1.0, 0.01, 0.1
        gaitSelection, scaling_factor, mode = 1, 6.0, 'test'
        motorVelocityLimit, motorTorqueLimit = np.inf, np.inf

    kern = pkg.SnakeGymEnv(pkg.Snake(None, "snake/snake.urdf", Args(), telemetry='kernel'), Args())
    repl = pkg.SnakeGymEnv(pkg.Snake(None, "snake/snake.urdf", Args()), Args())
    assert kern.telemetry == 'kernel' and repl.telemetry == 'replay'
    kern.reset(); repl.reset()
    for j in range(3):
        a = gait(pkg, 1, j, 8)[0].astype(np.float64) * 0.9
        ok, rk, dk, ik = kern.step(a.copy())
        orr, rr, dr, ir = repl.step(a.copy())
        assert np.array_equal(ok, orr) and rk == rr and dk == dr
        _same_infos(ik, ir)
        assert len(ik['internal_observations']) == kern.robot.counter > 0
        assert ik['internal_observations'] is kern.robot.step_internal_observations
    assert getattr(kern, "_scratch", None) is None and repl._scratch is not None
    kern.close(); repl.close()
    # thunks built with telemetry='kernel' carry it into the vector env
    envs = pkg.SubprocVecEnv([lambda: pkg.SnakeGymEnv(None, Args(), telemetry='kernel') for _ in range(2)])
    assert envs.mode == 'test' and envs.telemetry == 'kernel'
    envs.reset()
    infos = envs.step(gait(pkg, 2, 0, 8))[3]
    assert len(infos[0]['internal_observations']) == envs.last_substeps[0] and envs._scratch is None
    envs.close()


def test_device_vec_env_trace(pkg, monkeypatch):
    import torch
    _family(monkeypatch, False)
    B = 32
    env = pkg.DeviceVecEnv(B)
    st = pkg.Stepper(B)
    env.reset(); st.reset()
    assert env.trace_shape() == (B, 41, 128) == st.trace_shape()
    t = torch.empty(env.trace_shape(), dtype=torch.float32, device="cuda")
    for j in range(2):
        a = gait(pkg, B, j, 8)
        t.fill_(float("nan"))
        o, r, d = env.step(torch.tensor(a).cuda(), trace=t)
        torch.cuda.synchronize()
        O, R, D, S, T = st.step_traced(a)
        assert np.array_equal(o.cpu().numpy(), O) and np.array_equal(env.substeps.cpu().numpy(), S)
        got = t.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(T))              # the same rows written, the rest as it was
        assert np.array_equal(got.view(np.uint32)[~np.isnan(T)], T.view(np.uint32)[~np.isnan(T)])
        _check_shape_of_a_trace(got, S, 16)
    a = torch.tensor(gait(pkg, B, 2, 8)).cuda()
    bad = [torch.empty((B, 41, 127), dtype=torch.float32, device="cuda"),          # row length
           torch.empty((B, 40, 128), dtype=torch.float32, device="cuda"),          # too few rows
           torch.empty((B - 1, 41, 128), dtype=torch.float32, device="cuda"),      # envs
           torch.empty((B, 41, 128), dtype=torch.float64, device="cuda"),          # dtype
           torch.empty((B, 41, 128), dtype=torch.float32),                         # device
           torch.empty((B, 41, 256), dtype=torch.float32, device="cuda")[:, :, ::2]]   # not contiguous
    for x in bad:
        with pytest.raises(ValueError):
            env.step(a, trace=x)
    env.close(); st.close()


# ------------------------------------------------------------------------------------------------------------------
# 7. a poisoned handle
# ------------------------------------------------------------------------------------------------------------------
def test_alarm_refuses_the_traced_step(pkg, monkeypatch):
    import torch
    _family(monkeypatch, False)
    B = 16
    st = pkg.Stepper(B)
    st.reset()
    a = gait(pkg, B, 0, 8)
    st.step_traced(a.copy())
    st.debug_raise_alarm()
    msg = "env-step scheduler: a bounded wait ran out"
    with pytest.raises(RuntimeError) as ei:
        st.step_traced(a.copy())
    assert msg in str(ei.value)
    with pytest.raises(RuntimeError) as ei2:
        st.step(a.copy())
    assert msg in str(ei2.value)
    t_a = torch.tensor(a).cuda()
    t_o = torch.zeros((B, 56), device="cuda")
    t_r = torch.zeros((B,), device="cuda")
    t_d = torch.zeros((B,), dtype=torch.uint8, device="cuda")
    t_s = torch.zeros((B,), dtype=torch.int32, device="cuda")
    t_t = torch.full(st.trace_shape(), float("nan"), device="cuda")
    with pytest.raises(RuntimeError) as ei:
        st.step_traced_device(t_a.data_ptr(), t_o.data_ptr(), t_r.data_ptr(), t_d.data_ptr(), t_s.data_ptr(), t_t.data_ptr(), 41)
    assert msg in str(ei.value)
    torch.cuda.synchronize()
    assert float(t_o.abs().sum()) == 0.0 and bool(torch.isnan(t_t).all())          # nothing ran
    st.close()
