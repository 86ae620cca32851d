"""Episodes that start from a caller-given pose (snk_set_reset_pose; the reference's Snake.initPosition / initOrientation /
initState, snake.py:22-24, 119-127), against vectors produced by EXECUTING the reference's own Python with those
attributes set (tests/golden/make_reset_pose_vectors.py: two poses x (SnakeGymEnv.step | the SubprocVecEnv worker)).

CPU (`-m "not gpu"`): the recipe the GPU tests use as their yardstick -- the oracle's env-step and, where an episode ends,
its soft reset with the pose written over position, orientation and joint angles and prev_x set as the reference's
`_observation` ends up -- on ONE free-running oracle env per scenario reproduces the recorded run: every pre-step state
bit for bit, observations and rewards to 1e-9, counts and dones exactly, the worker's post-reset observation and prev_x
after each kind of reset included."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
VEC = os.path.join(HERE, "golden", "reset_pose_vectors.npz")
N = 16


@pytest.fixture(scope="module")
def vec():
    d = np.load(VEC)
    return {k: d[k] for k in d.files}


def apply_pose(e, pose, prev_x=None):
    """The soft reset's writes on an oracle env that orc_reset (or the auto-reset of orc_env_step) has just put on the
    zero pose with zero twist and joint rates: position, orientation, joint angles <- pose; with prev_x also the reward's
    previous x (torques and the joint-0 force stay)."""
    n = e.n
    s = e.get_state()
    s[0:3], s[3:7], s[13:13 + n] = pose[0:3], pose[3:7], pose[7:7 + n]
    e.set_state(s)
    if prev_x is not None:
        tau, fz, _ = e.get_aux()
        e.set_aux(tau, fz, float(prev_x))


def reset_to_pose(e, pose):
    """SnakeGymEnv.reset() with the pose set (SnakeGymEnv.py:28-31): returns the reset observation."""
    e.reset()
    apply_pose(e, pose, prev_x=pose[0])
    return e.get_obs()


def env_step_with_pose(e, action, vec_mode, pose):
    """orc_env_step, then -- where the episode ended -- the pose over the zero pose its soft reset wrote.  vec_mode 1 (the
    worker): the returned observation is the pose's and prev_x its x (multiprocessing_env.py:13-15 -> SnakeGymEnv.py:30);
    vec_mode 0: the terminal observation, prev_x stays its x (SnakeGymEnv.py:41-42)."""
    o, r, d, k, a = e.env_step(action, vec_mode=vec_mode)
    if d:
        apply_pose(e, pose, prev_x=pose[0] if vec_mode else None)
        if vec_mode:
            o = e.get_obs()
    return o, r, d, k, a


def scenarios(v):
    return [np.nonzero(v["scenario"] == s)[0] for s in np.unique(v["scenario"])]


def test_vectors_cover_both_poses_and_both_seams(vec):
    v = vec
    seen = set()
    for rows in scenarios(v):
        assert len(rows) >= 25 and v["done"][rows].sum() >= 2            # at least two episode ends per scenario
        pose = v["pose"][rows[0]]
        assert np.all(v["pose"][rows] == pose) and np.all(np.isfinite(pose))
        assert abs(np.linalg.norm(pose[3:7]) - 1) < 1e-12 and pose[5] != 0      # yawed
        assert np.abs(pose[:2]).min() > 0 and pose[2] == 0                       # a planar offset
        seen.add((int(v["vec_mode"][rows[0]]), bool(np.all(pose[7::2] == 0))))
        # the run starts ON the pose: the soft reset before the first step
        assert np.array_equal(v["state"][rows[0], 0:7], pose[0:7]) and np.array_equal(v["state"][rows[0], 13:13 + N], pose[7:])
        assert v["aux"][rows[0], N + 1] == pose[0]
    # (seam, "even joints at zero"): pose A leaves the even slots at zero, pose B bends every joint
    assert seen == {(0, True), (1, True), (0, False), (1, False)}
    assert np.abs(v["pose"][:, 7:]).max() <= 0.25 + 1e-12                        # inside the joint limits


def test_recipe_on_one_free_running_oracle_env_reproduces_the_reference(vec, oracle_mod):
    v = vec
    for rows in scenarios(v):
        i0 = rows[0]
        pose, vec_mode = v["pose"][i0], bool(v["vec_mode"][i0])
        e = oracle_mod.OracleEnv()
        e.hard_reset()
        e.sync(v["state"][i0], v["aux"][i0], v["manifold"][i0])
        for i in rows:
            # the state, caches and prev_x this step starts from are the reference's, bit for bit, with no
            # re-synchronisation since the scenario's first step: every reset in between went through the recipe
            tau, fz, px = e.get_aux()
            assert np.array_equal(e.get_state(), v["state"][i]), (i, np.abs(e.get_state() - v["state"][i]).max())
            assert np.array_equal(np.concatenate([tau, [fz, px]]), v["aux"][i]), i
            assert np.array_equal(e.get_manifold(), v["manifold"][i]), i
            o, r, d, k, a = env_step_with_pose(e, v["action_in"][i].copy(), vec_mode, pose)
            assert np.array_equal(a, v["action_out"][i]), i
            assert k == v["substeps"][i] and d == bool(v["done"][i]), (i, k, v["substeps"][i], d)
            assert abs(r - v["reward"][i]) < 1e-9, (i, r, v["reward"][i])
            assert np.abs(o - v["obs"][i]).max() < 1e-9, i
            # what the step left behind: the post-reset state of a done env, and prev_x after each kind of reset
            tau, fz, px = e.get_aux()
            assert np.array_equal(e.get_state(), v["post_state"][i]), i
            assert np.array_equal(np.concatenate([tau, [fz, px]]), v["post_aux"][i]), i
            if d:
                s = v["post_state"][i]
                assert np.array_equal(s[0:7], pose[0:7]) and np.all(s[7:13] == 0)
                assert np.array_equal(s[13:13 + N], pose[7:]) and np.all(s[13 + N:] == 0)
                assert px == (pose[0] if vec_mode else v["obs"][i][3 * N])
                if vec_mode:        # the worker's post-reset observation: the pose, zero rates, the persisted caches
                    assert np.array_equal(o[:N], pose[7:]) and np.all(o[N:2 * N] == 0)
                    assert np.array_equal(o[3 * N:3 * N + 7], pose[0:7])
                    assert np.array_equal(o[2 * N:3 * N], tau) and o[3 * N + 7] == fz


def test_explicit_reset_to_the_pose(vec, oracle_mod):
    """SnakeGymEnv.reset() with the attributes set: the first row of every scenario is the state right after it."""
    v = vec
    for rows in scenarios(v):
        i0 = rows[0]
        e = oracle_mod.OracleEnv()
        e.hard_reset()
        o = reset_to_pose(e, v["pose"][i0])
        assert np.array_equal(e.get_state(), v["state"][i0])
        tau, fz, px = e.get_aux()
        assert np.array_equal(np.concatenate([tau, [fz, px]]), v["aux"][i0])
        assert np.array_equal(o[3 * N:3 * N + 7], v["pose"][i0][:7]) and np.array_equal(o[:N], v["pose"][i0][7:])
