"""Generates tests/golden/reset_pose_vectors.npz by RUNNING the reference's own env-logic code with the three attributes
its Snake reads at every soft reset set to something other than their defaults:

    robot.initPosition, robot.initOrientation   snake.py:23-24, read by resetPositionOrientation (snake.py:126-127)
    robot.initState                             snake.py:22,    read by resetPose (snake.py:119-124)

The machinery is make_env_logic_vectors.py's, imported as it is: the reference's snake.py / SnakeGymEnv.py /
ppo/multiprocessing_env.py::worker behind the injected client that the CPU oracle answers (its
resetBasePositionAndOrientation and resetJointState take whatever pose the reference hands them).  Every line of the
reference that decides WHEN a reset happens, what it writes and which observation becomes `_observation` afterwards is
executed, not restated.

Two poses:
  A  the base at (0.3, -0.2, 0), yawed by 0.4 rad, +-0.25 rad on the joints the default gait drives (odd slots), zero elsewhere
  B  the base at (-0.1, 0.25, 0), yawed by -0.7 rad, +-0.15 rad on EVERY joint: inside the limits, but not planar
Four scenarios (pose A, B) x (SnakeGymEnv.step called directly | the SubprocVecEnv worker's reset-on-done), 26 env-steps
of the bench's serpenoid gait each, every one with at least two episode ends (asserted below).

Stored per env-step, in the layout tests/test_env_logic_golden.py's vectors have (arrays only, no reference text): the
state the step started from (state, aux with prev_x = the reference's `_observation[48]`, contact cache), the action, the
returned observation / reward / done / substep count, the servo errors -- and, new here, the env's reset pose, the state and
aux right AFTER the step (post-reset for a done env) and the `_observation[48]` the reference holds after it.

Run where the reference is:  python tests/golden/make_reset_pose_vectors.py
"""
import importlib.util
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_env_logic_vectors", os.path.join(HERE, "make_env_logic_vectors.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

N = 16
STEPS = 26


def yaw_quat(yaw):
    return [0.0, 0.0, float(np.sin(yaw / 2)), float(np.cos(yaw / 2))]


def pose_a():
    q = np.zeros(N)
    q[1::2] = 0.25 * np.array([1, -1] * (N // 4))        # the joints gait 1 drives (snake.py:247-269)
    return [0.3, -0.2, 0.0], yaw_quat(0.4), q.tolist()


def pose_b():
    q = 0.15 * np.array([1, -1] * (N // 2), dtype=np.float64)
    return [-0.1, 0.25, 0.0], yaw_quat(-0.7), q.tolist()


def pose_row(robot):
    return np.concatenate([np.asarray(robot.initPosition, dtype=np.float64), np.asarray(robot.initOrientation, dtype=np.float64),
                           np.asarray(robot.initState, dtype=np.float64)])


def set_pose(pose):
    """The `setup` hook of the existing generator's scenarios: the attributes on the reference's Snake, then the
    reference's own soft reset (SnakeGymEnv.reset -> Snake.reset(False) -> resetPositionOrientation, resetPose)."""
    def setup(client, env):
        env.robot.initPosition, env.robot.initOrientation, env.robot.initState = pose
        env.reset()
    return setup


def post(client, env):
    e = client.e
    tau, fz, _ = e.get_aux()
    return dict(state=e.get_state(), aux=np.concatenate([tau, [fz, float(env._observation[3 * e.n])]]), manifold=e.get_manifold())


def run_single(rows, scen, actions, pose):
    client, robot, env = base.new_env()
    env.reset()
    set_pose(pose)(client, env)
    rec = base.Recorder()
    for a in actions:
        a = np.array(a, dtype=np.float64)
        pre = rec.pre(client, env)
        a_in = a.copy()
        client.servo_err = []
        obs, rew, done, info = env.step(a)
        assert info == {}
        rows.append(dict(scen=scen, vec=0, pre=pre, post=post(client, env), a_in=a_in, a_out=a.copy(), obs=np.array(obs, dtype=np.float64),
                         rew=float(rew), done=bool(done), k=int(robot.counter), err=list(client.servo_err), pose=pose_row(robot)))


def run_worker(rows, scen, actions, pose):
    client, robot, env = base.new_env()
    env.reset()
    set_pose(pose)(client, env)
    rec = base.Recorder()
    pres, a_ins, posts, counters, errs = [], [], [], [], []

    def on_step(a):
        if pres:
            posts.append(post(client, env))      # the worker has finished the step before (its reset-on-done included)
        pres.append(rec.pre(client, env))
        a_ins.append(np.array(a, dtype=np.float64).copy())

    acts = [np.array(a, dtype=np.float64) for a in actions]
    cmds = [("step", a) for a in acts] + [("get_spaces", None), ("close", None)]
    remote = base.FakeRemote(cmds, on_step)
    real_step = env.step

    def step_and_count(a):
        client.servo_err = []
        out = real_step(a)
        counters.append(robot.counter)
        errs.append(list(client.servo_err))
        return out
    env.step = step_and_count
    base.ref_mp.worker(remote, base.FakeRemote([], None), types.SimpleNamespace(x=lambda: env))
    posts.append(post(client, env))
    outs = remote.sent[:-1]
    assert len(outs) == len(acts) == len(counters) == len(posts)
    for a, a_in, pre, po, (obs, rew, done, info), k, er in zip(acts, a_ins, pres, posts, outs, counters, errs):
        assert info == {}
        rows.append(dict(scen=scen, vec=1, pre=pre, post=po, a_in=a_in, a_out=a.copy(), obs=np.array(obs, dtype=np.float64),
                         rew=float(rew), done=bool(done), k=int(k), err=er, pose=pose_row(robot)))


def main():
    rows = []
    # the bench's serpenoid gait; the amplitude is raised (and clipped by checkBound, SnakeGymEnv.py:82-88) until obs[9]
    # ends at least two episodes in every scenario
    amp = {0: 1.0, 1: 1.0, 2: 1.0, 3: 1.0}
    scen = 0
    for pose in (pose_a(), pose_b()):
        for runner, phi in ((run_single, 0.4), (run_worker, 1.3)):
            while True:
                mine = []
                runner(mine, scen, [amp[scen] * base.gait_action(j, phi) for j in range(STEPS)], pose)
                if sum(r["done"] for r in mine) >= 2:
                    break
                amp[scen] += 0.25
                assert amp[scen] <= 3.0, "scenario %d: no two episode ends" % scen
            rows += mine
            scen += 1
    R = rows
    d = {
        "scenario": np.array([r["scen"] for r in R], dtype=np.int32),
        "vec_mode": np.array([r["vec"] for r in R], dtype=np.int32),
        "pose": np.stack([r["pose"] for r in R]),
        "state": np.stack([r["pre"]["state"] for r in R]),
        "aux": np.stack([r["pre"]["aux"] for r in R]),
        "manifold": np.stack([r["pre"]["manifold"] for r in R]),
        "post_state": np.stack([r["post"]["state"] for r in R]),
        "post_aux": np.stack([r["post"]["aux"] for r in R]),
        "action_in": np.stack([r["a_in"] for r in R]),
        "action_out": np.stack([r["a_out"] for r in R]),
        "obs": np.stack([r["obs"] for r in R]),
        "reward": np.array([r["rew"] for r in R]),
        "done": np.array([r["done"] for r in R], dtype=np.bool_),
        "substeps": np.array([r["k"] for r in R], dtype=np.int32),
        "servo_err": np.stack([np.pad(np.array(r["err"], dtype=np.float64), (0, 41 - len(r["err"]))) for r in R]),
        "gait_amplitude": np.array([amp[s] for s in range(scen)]),
    }
    out = os.path.join(HERE, "reset_pose_vectors.npz")
    np.savez_compressed(out, **d)
    print("wrote", out, os.path.getsize(out), "bytes:", len(R), "env-steps; done per scenario",
          [int(d["done"][d["scenario"] == s].sum()) for s in range(scen)], "gait amplitudes", d["gait_amplitude"].tolist())


if __name__ == "__main__":
    main()
