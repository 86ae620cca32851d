"""The tensor seam on the GPU (include/snk.h: snk_substep, snk_observe, snk_link_states, snk_copy_envs; device_env.py:
DeviceWorld): link states against the independent numpy model, the masked substep against the host substep bit for bit,
a torch env over the seam against the fused step kernel bit for bit, the env fork, and the entry contract."""
import importlib

import numpy as np
import pytest

import np_link_states as nls
from conftest import f32_gate, random_state      # noqa: E402

pytestmark = pytest.mark.gpu


def gait(ids, j, A=8):
    k = np.arange(A)
    return (-np.sin((2 * k[None, :] + 1) * 4.0 + 0.2 * j + 0.37 * np.asarray(ids)[:, None])).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def snap_equal(a, b, rows_a, rows_b, fields):
    return [k for k in fields if getattr(a, k) is not None and not same_bits(getattr(a, k)[rows_a], getattr(b, k)[rows_b])]


STATE_FIELDS = ("state", "aux", "ground_friction", "manifold", "box_state", "box_manifold")


# ----------------------------------------------------------------------------------------------------------------------
# 1. link states against the independent model
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def link_cases(pkg):
    """Per chain length: 24 random states (tumbled base, joints across their range, non-zero twists) on a handle, what
    the GPU says of them, and the float64 reference and float32 twin of tests/np_link_states.py -- computed once."""
    out = {}
    for n in (16, 32):
        rng = np.random.default_rng(1400 + n)
        S = np.stack([random_state(rng, n, z=0.3, qamp=1.5, vamp=1.0) for _ in range(24)]).astype(np.float32)
        st = pkg.Stepper(24, n_modules=n)
        st.set_state(S, None)
        got = st.link_states()
        S2, _ = st.get_state()
        lp = st.link_positions()
        st.close()
        ref = np.stack([nls.reference(s, n) for s in S])
        tw = np.stack([nls.twin(s, n) for s in S])
        out[n] = dict(S=S, S2=S2, got=got, lp=lp, ref=ref, twin=tw)
    return out


@pytest.mark.parametrize("n", [16, 32])
def test_link_states_match_the_independent_model(link_cases, n):
    """COM, orientation, link-frame origin, COM velocity and angular velocity of all 3n + 2 links against np_model's
    ow + Rw c, Rw, ow, Jv gvel, Jw gvel in float64 on the float32 state, gated by the same formulas evaluated in float32
    (the twin: the yardstick, not the kernel).  Factor 3: the kernel composes n + 1 composite-body frames plus one fixed
    offset, the twin the 3n + 2-link tree, so the two round differently.  Floors: the project's figure for chain
    round-off, 17 x 6e-8 x 1.1 m ~ 1e-6 m (1e-6 in 1 - |q . q'|, 1e-6 x the largest twist component); hard caps 1e-4 m,
    1e-4, 1e-3 relative.  The GATE lines of a run are profiles/r14_link_state_accuracy.txt."""
    c = link_cases[n]
    S, got, ref, tw = c["S"], c["got"], c["ref"], c["twin"]
    assert got.shape == (24, 3 * n + 2, 16) and got.dtype == np.float32 and np.all(np.isfinite(got))
    assert same_bits(c["S2"], S)
    # row 0 is the record itself: bitwise what get_state returns
    root = np.concatenate([S[:, 0:7], S[:, 0:3], S[:, 10:13], S[:, 7:10]], axis=1)
    assert same_bits(got[:, 0, :], root)
    # quaternions: unit to float32 round-off and signed w >= 0 (row 0 is the caller's own quaternion: as given)
    assert np.all(got[:, 1:, 6] >= 0)
    assert np.max(np.abs(np.linalg.norm(got[:, 1:, 3:7].astype(np.float64), axis=2) - 1.0)) < 3e-7
    worst = {k: [0.0, 0.0] for k in ("com", "origin", "quat", "vel", "omega")}
    for e in range(24):
        gvel = nls.split_state(S[e].astype(np.float64), n)[2]
        r = ref[e].copy()
        r[0, 3:7] *= np.sign(np.sum(r[0, 3:7] * got[e, 0, 3:7]))      # (the root's sign is the caller's)
        eg, et = nls.errors(got[e], r, gvel), nls.errors(tw[e], ref[e], gvel)
        for k in worst:
            worst[k] = [max(worst[k][0], eg[k]), max(worst[k][1], et[k])]
    caps = dict(com=1e-4, origin=1e-4, quat=1e-4, vel=1e-3, omega=1e-3)
    for k in ("com", "origin", "quat", "vel", "omega"):
        f32_gate("link states n=%d: %s (worst of 24 states x %d links)" % (n, k, 3 * n + 2), worst[k][0], worst[k][1],
                 factor=3.0, floor=1e-6, cap=caps[k])
    # rows 1 + 3k are getLinkPositions' links 0, 3, .., 3n: the same points by another route (obs_kernel's)
    lp = c["lp"].reshape(24, 3, n + 1).transpose(0, 2, 1)
    d = np.max(np.abs(got[:, 1::3, 0:3].astype(np.float64) - lp))
    print("  link states n=%d: rows 1 + 3k against link_positions: %.3e m" % (n, d))
    assert got[:, 1::3].shape[1] == n + 1 and d < 1e-6


def test_link_states_env_ids_on_the_device(pkg):
    """env_ids permuted and repeated; an id outside the handle gives rows of zeros; bytes beyond n_rows are left alone."""
    torch = pytest.importorskip("torch")
    n, E = 16, 5
    rng = np.random.default_rng(77)
    S = np.stack([random_state(rng, n, z=0.3, qamp=1.0) for _ in range(E)]).astype(np.float32)
    st = pkg.Stepper(E, n_modules=n)
    st.set_state(S, None)
    full = st.link_states()
    assert same_bits(st.link_states([3, 0, 3]), full[[3, 0, 3]])
    world = pkg.DeviceWorld(stepper=st)
    ids = [4, 1, 1, E, 0, -1, 2]
    dev = world.link_states(ids)
    assert tuple(dev.shape) == (len(ids), 3 * n + 2, 16)
    buf = torch.full((len(ids) + 1, 3 * n + 2, 16), -7.0, dtype=torch.float32, device=world.device)
    idt = torch.tensor(ids, dtype=torch.int32, device=world.device)
    st.link_states_device(idt.data_ptr(), len(ids), buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dev, buf = dev.cpu().numpy(), buf.cpu().numpy()
    for k, e in enumerate(ids):
        want = full[e] if 0 <= e < E else np.zeros_like(full[0])
        assert same_bits(dev[k], want) and same_bits(buf[k], want), (k, e)
    assert np.all(buf[len(ids)] == -7.0)
    # without ids: envs 0 .. n_rows - 1; and into a caller's tensor
    out = torch.empty((E, 3 * n + 2, 16), dtype=torch.float32, device=world.device)
    assert world.link_states(out=out) is out
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), full)
    # the host form refuses what the device form cannot
    with pytest.raises(RuntimeError, match=r"env_ids\[1\] = 5 is outside 0 \.\. 4"):
        st.link_states([0, E])
    with pytest.raises(ValueError, match="shape"):
        world.link_states(out=torch.empty((E, 3 * n + 2, 15), dtype=torch.float32, device=world.device))
    st.close()


def test_snake_link_orientations_and_base_velocity(pkg):
    """Snake.getLinkOrientations (snake.py:148-156): [x.., y.., z.., w..] over links 0, 3, .., 3n, from the same rows."""
    env = pkg.SnakeGymEnv(None, None)
    env.reset()
    for j in range(2):
        env.step(gait([1], j)[0] * 0.9)
    robot, st, n = env.robot, env._stepper, 16
    rows = st.link_states()[0]
    o = robot.getLinkOrientations()
    assert o.shape == (4 * (n + 1),) and o.dtype == np.float64
    assert np.array_equal(o.reshape(4, n + 1).T, rows[1::3, 3:7].astype(np.float64))
    assert np.allclose(np.linalg.norm(o.reshape(4, n + 1), axis=0), 1.0, atol=1e-6)
    # and next to getLinkPositions, link by link
    assert np.max(np.abs(robot.getLinkPositions().reshape(3, n + 1).T - rows[1::3, 0:3])) < 1e-6
    v, w = robot.getBaseVelocity()
    S, _ = st.get_state()
    assert np.array_equal(np.float32(v), S[0, 10:13]) and np.array_equal(np.float32(w), S[0, 7:10])
    env.close()


# ----------------------------------------------------------------------------------------------------------------------
# 2. the masked substep
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 32])
def test_masked_substep_is_the_host_substep_on_the_active_envs(pkg, n):
    torch = pytest.importorskip("torch")
    E, A = 6, n // 2
    a, b = pkg.Stepper(E, n_modules=n), pkg.Stepper(E, n_modules=n)
    a.reset()
    for j in range(3):
        a.step(gait(range(E), j, A) * 0.9)
    snap = a.snapshot()
    b.restore(snap)
    assert snap.manifold is not None and snap.manifold[:, :, 0].sum() > 0          # non-trivial: contacts in the cache
    tg = np.zeros((E, n), np.float32)
    tg[:, 1::2] = gait(range(E), 3, A) * np.float32(np.pi / 6)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    t_tg = torch.tensor(tg, device=dev)
    mask = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    on, off = np.nonzero(mask)[0], np.nonzero(mask == 0)[0]
    t_mask = torch.tensor(mask, device=dev)
    t_info = torch.full((E, 2), -77, dtype=torch.int32, device=dev)
    a.substep_device(t_tg.data_ptr(), 3, t_mask.data_ptr(), t_info.data_ptr(), stream)
    torch.cuda.synchronize()
    info_b = b.substep(tg, 3)
    sa, sb = a.snapshot(), b.snapshot()
    info_a = t_info.cpu().numpy()
    assert snap_equal(sa, sb, on, on, STATE_FIELDS) == []
    assert np.array_equal(info_a[on], info_b[on]) and np.all(info_b[on, 0] > 0)
    assert snap_equal(sa, snap, off, off, STATE_FIELDS) == [] and np.all(info_a[off] == -77)
    assert not same_bits(sa.state[on], snap.state[on])                              # (the active ones did move)
    # NULL mask: every env, bit for bit the host call -- and through DeviceWorld, with a bool mask of ones
    a.restore(snap)
    b.restore(snap)
    a.substep_device(t_tg.data_ptr(), 2, 0, t_info.data_ptr(), stream)
    torch.cuda.synchronize()
    info_b = b.substep(tg, 2)
    assert snap_equal(a.snapshot(), b.snapshot(), slice(None), slice(None), STATE_FIELDS) == []
    assert np.array_equal(t_info.cpu().numpy(), info_b)
    world = pkg.DeviceWorld(stepper=a)
    world.step_simulation(t_tg, 2, active=torch.ones(E, dtype=torch.bool, device=dev))
    b.substep(tg, 2)
    assert snap_equal(a.snapshot(), b.snapshot(), slice(None), slice(None), STATE_FIELDS) == []
    with pytest.raises(ValueError, match="targets must have shape"):
        world.step_simulation(t_tg[:, :-1].contiguous())
    with pytest.raises(ValueError, match="active must be"):
        world.step_simulation(t_tg, active=torch.ones(E, dtype=torch.int32, device=dev))
    a.close()
    b.close()


# ----------------------------------------------------------------------------------------------------------------------
# 3. a torch env on the seam reproduces the fused kernel
# ----------------------------------------------------------------------------------------------------------------------
def test_torch_servo_loop_over_the_seam_is_the_fused_step(pkg):
    """Snake.step's loop (snake.py:283-304) written in torch over DeviceWorld -- feedback norm in float64 from the float32
    observation (as snake_env.Snake has it), `active` = the envs still inside their loop, the height exit through
    mean_height, the counter cap -- ends every env-step with the fused kernel's substep count and, bit for bit, its
    observation.  Nothing but the final comparison touches the host."""
    torch = pytest.importorskip("torch")
    E, n, A, steps = 8, 16, 8, 5
    world = pkg.DeviceWorld(E)
    P = world.params
    dev = world.device
    acts = np.stack([gait(range(E), j, A) * np.float32(0.9) for j in range(steps)])      # (|q9| stays below 0.5)
    t_acts = torch.tensor(acts, device=dev)
    obs = world.reset()
    height = torch.empty(E, dtype=torch.float32, device=dev)
    all_obs = torch.zeros((steps, E, world.obs_dim), dtype=torch.float32, device=dev)
    all_cnt = torch.zeros((steps, E), dtype=torch.int32, device=dev)
    scaling = float(np.float32(P.scaling_factor))
    for j in range(steps):
        targets = torch.zeros((E, n), dtype=torch.float32, device=dev)
        targets[:, 1::2] = t_acts[j] * scaling                                        # createAction, gait 1 (snake.py:247-269)
        t64 = targets.double()
        counter = torch.zeros(E, dtype=torch.int32, device=dev)
        world.observation(out=obs)
        active = (t64 - obs[:, :n].double()).norm(dim=1) > P.servo_tol                 # checkFeedback (snake.py:228-235)
        for _ in range(P.max_counter + 1):
            world.step_simulation(targets, 1, active=active)                          # stepSimulation (snake.py:286)
            world.observation(out=obs)
            world.mean_height(out=height)
            counter += active.to(torch.int32)
            too_high = height > P.height_threshold                                    # checkSnakeHeight (snake.py:295-297)
            capped = counter > P.max_counter                                          # snake.py:303
            wants = (t64 - obs[:, :n].double()).norm(dim=1) > P.servo_tol
            active = active & wants & ~too_high & ~capped
        all_obs[j] = obs
        all_cnt[j] = counter
    torch.cuda.synchronize()
    all_obs, all_cnt = all_obs.cpu().numpy(), all_cnt.cpu().numpy()
    world.close()
    twin = pkg.Stepper(E)
    twin.reset()
    for j in range(steps):
        o, r, d, sub = twin.step(acts[j].copy(), vec_mode=False)
        assert not d.any(), (j, d)
        assert np.array_equal(sub, all_cnt[j]), (j, sub, all_cnt[j])
        assert same_bits(o, all_obs[j]), (j, np.nonzero(bits(o) != bits(all_obs[j])))
    assert all_cnt.min() > 0 and len(np.unique(all_cnt)) > 1                          # (a loop that ran, env by env)
    twin.close()


# ----------------------------------------------------------------------------------------------------------------------
# 4. fork
# ----------------------------------------------------------------------------------------------------------------------
def _pose_rows(E, n, rng):
    pose = np.zeros((E, 7 + n), np.float32)
    pose[:, 0:2] = rng.uniform(-0.2, 0.2, (E, 2))
    pose[:, 6] = 1.0
    pose[:, 7:] = rng.uniform(-0.3, 0.3, (E, n))
    return pose


@pytest.mark.parametrize("obstacle", [0, 2])
def test_fork_copies_the_simulator_state(pkg, obstacle):
    E, n, A = 8, 16, 8
    rng = np.random.default_rng(40 + obstacle)
    st = pkg.Stepper(E, n_modules=n, obstacle=obstacle, contact_model=1)
    st.reset()
    st.set_ground_friction((0.6 + 0.1 * np.arange(E)).astype(np.float32))
    if obstacle == 2:
        bs, _ = st.get_box()
        bs[:, 1] = 0.05 * np.arange(E)                   # every env's box somewhere else
        st.set_box(bs, None)
    pose = _pose_rows(E, n, rng)
    st.set_reset_pose(pose)
    for j in range(3):
        st.step(gait(range(E), j, A) * 0.9)
    before = st.snapshot()
    assert before.manifold[:, :, 0].sum() > 0 and (obstacle == 2) == (before.box_state is not None)
    world = pkg.DeviceWorld(stepper=st)
    src, dst, rest = [0, 1, 2], [5, 6, 7], [0, 1, 2, 3, 4]
    world.fork(src, dst)
    after = st.snapshot()
    assert snap_equal(after, before, dst, src, STATE_FIELDS) == []
    assert snap_equal(after, before, rest, rest, STATE_FIELDS) == []
    assert not same_bits(before.state[dst], before.state[src])
    assert same_bits(after.reset_pose, pose)                                          # without the flag: not copied
    if obstacle == 2:
        assert same_bits(after.box_state[dst], before.box_state[src]) and not same_bits(before.box_state[dst], before.box_state[src])
    # two env-steps in which each dst gets its src's action: the pairs stay on the same bits
    st.set_reset_pose(np.broadcast_to(pose[0], pose.shape).copy())                    # (a reset would land both alike)
    for j in range(3, 5):
        a = gait(range(E), j, A) * np.float32(0.9)
        a[dst] = a[src]
        o, r, d, sub = st.step(a)
        assert same_bits(o[dst], o[src]) and same_bits(r[dst], r[src])
        assert np.array_equal(d[dst], d[src]) and np.array_equal(sub[dst], sub[src]) and sub[src].min() > 0
    end = st.snapshot()
    assert snap_equal(end, end, dst, src, STATE_FIELDS) == []
    assert not same_bits(end.state[[3]], end.state[[4]])
    # reset_pose=True copies the rows of the reset-pose table too; CUDA id tensors pass through as they are
    torch = world.torch
    st.set_reset_pose(pose)
    world.fork(torch.tensor([3], dtype=torch.int32, device=world.device),
               torch.tensor([4], dtype=torch.int32, device=world.device), reset_pose=True)
    got = st.get_reset_pose()
    want = pose.copy()
    want[4] = pose[3]
    assert same_bits(got, want)
    fin = st.snapshot()
    assert snap_equal(fin, end, [4], [3], STATE_FIELDS) == [] and snap_equal(fin, end, rest[:4] + dst, rest[:4] + dst, STATE_FIELDS) == []
    st.close()


def test_fork_host_form_refuses_by_index(pkg):
    E = 8
    st = pkg.Stepper(E)
    st.reset()
    for j in range(2):
        st.step(gait(range(E), j) * 0.9)
    before = st.snapshot()
    for src, dst, msg in (([0, 1, 2], [5, 6, 5], r"dst_ids\[2\] = 5 repeats dst_ids\[0\]"),
                          ([0, 1], [5, 0], r"dst_ids\[1\] = 0 is also src_ids\[0\]"),
                          ([0, E], [5, 6], r"src_ids\[1\] = 8 is outside 0 \.\. 7"),
                          ([0, 1], [5, -1], r"dst_ids\[1\] = -1 is outside 0 \.\. 7")):
        with pytest.raises(RuntimeError, match=msg):
            st.copy_envs(src, dst)
        assert snap_equal(st.snapshot(), before, slice(None), slice(None), STATE_FIELDS + ("reset_pose",)) == []
    world = pkg.DeviceWorld(stepper=st)
    with pytest.raises(ValueError, match=r"dst\[2\] = 5 repeats dst\[0\]"):
        world.fork([0, 1, 2], [5, 6, 5])
    assert snap_equal(st.snapshot(), before, slice(None), slice(None), STATE_FIELDS) == []
    # on the device path an id outside the handle makes its pair a no-op, the other pairs go through
    torch = world.torch
    world.fork(torch.tensor([0, E, 1], dtype=torch.int32, device=world.device),
               torch.tensor([5, 6, -3], dtype=torch.int32, device=world.device))
    after = st.snapshot()
    assert snap_equal(after, before, [5], [0], STATE_FIELDS) == []
    assert snap_equal(after, before, [0, 1, 2, 3, 4, 6, 7], [0, 1, 2, 3, 4, 6, 7], STATE_FIELDS) == []
    st.copy_envs([1], [6])                                                             # and the host form copies
    assert snap_equal(st.snapshot(), before, [6], [1], STATE_FIELDS) == []
    st.close()


# ----------------------------------------------------------------------------------------------------------------------
# 5. contract
# ----------------------------------------------------------------------------------------------------------------------
def test_seam_calls_refuse_a_poisoned_handle_and_null_outputs(pkg):
    torch = pytest.importorskip("torch")
    E, n = 4, 16
    st = pkg.Stepper(E)
    dev = torch.device("cuda", 0)
    tg = torch.zeros((E, n), dtype=torch.float32, device=dev)
    obs = torch.zeros((E, st.obs_dim), dtype=torch.float32, device=dev)
    rows = torch.zeros((E, 3 * n + 2, 16), dtype=torch.float32, device=dev)
    ids = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    ids2 = torch.tensor([2, 3], dtype=torch.int32, device=dev)
    assert st.link_rows == 3 * n + 2
    with pytest.raises(RuntimeError, match="snk_observe: obs_dev, height_dev and linkpos_dev are all null"):
        st.observe_device()
    with pytest.raises(RuntimeError, match="n_rows must be at least 1"):
        st.link_states_device(0, 0, rows.data_ptr())
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        st.link_states_device(0, 1, rows.data_ptr() + 4)
    with pytest.raises(RuntimeError, match="unknown bits in flags"):
        pkg._lib.check(st.lib.snk_copy_envs(st.h, ids.data_ptr(), ids2.data_ptr(), 2, 2, None), "snk_copy_envs")
    calls = (lambda: st.substep_device(tg.data_ptr(), 1),
             lambda: st.observe_device(obs_ptr=obs.data_ptr()),
             lambda: st.link_states_device(0, E, rows.data_ptr()),
             lambda: st.copy_envs_device(ids.data_ptr(), ids2.data_ptr(), 2),
             lambda: st.link_states(),
             lambda: st.copy_envs([0], [1]))
    for f in calls:
        f()                                              # alive: every one goes through
    torch.cuda.synchronize()
    st.debug_raise_alarm()
    for f in calls:
        with pytest.raises(RuntimeError, match="env-step scheduler: a bounded wait ran out"):
            f()
    assert st.link_rows == 3 * n + 2                     # (a dimension getter: still answers)
    st.close()
    assert st.h is None


def test_a_step_enqueued_behind_a_substep_sees_its_result(pkg):
    """snk_substep is asynchronous on the stream and ordered with what follows there: substeps, then a fused env-step
    and a link-state read-out, with no synchronisation in between, against the synchronous host path."""
    torch = pytest.importorskip("torch")
    E, n = 6, 16
    env = pkg.DeviceVecEnv(E)
    env.reset()
    world = env.world
    assert world.stepper is env.stepper and env.world is world
    tg = np.zeros((E, n), np.float32)
    tg[:, 1::2] = gait(range(E), 0) * np.float32(0.4)
    act = gait(range(E), 1) * np.float32(0.9)
    world.step_simulation(torch.tensor(tg, device=env.device), 3)
    obs, rew, done = env.step(torch.tensor(act, device=env.device), vec_mode=False)
    rows = world.link_states()
    torch.cuda.synchronize()
    twin = pkg.Stepper(E)
    twin.reset()
    twin.substep(tg, 3)
    o, r, d, _ = twin.step(act.copy(), vec_mode=False)
    assert same_bits(obs.cpu().numpy(), o) and same_bits(rew.cpu().numpy(), r) and np.array_equal(done.cpu().numpy() != 0, d)
    assert same_bits(rows.cpu().numpy(), twin.link_states())
    twin.close()
    env.close()
