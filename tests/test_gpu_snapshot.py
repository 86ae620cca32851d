"""Snapshot on the kernels: a fresh handle restored from a snapshot continues bit for bit, in any slot order, on every
handle kind, reset-pose table included; and a test-mode replay starts from the snapshot of the step's own handle, so
friction that reached that handle behind the environment's back is replayed too.  (What Snapshot itself does is pinned
without a GPU by tests/test_snapshot_host.py; tests/test_gpu_step_trace.py::test_trace_is_the_replay and the oracle tests
stay on the explicit getters as the independent check.)"""
import numpy as np
import pytest

from conftest import ROUND1
from test_gpu_reset_pose import _family, default_rows, gait, random_poses

pytestmark = pytest.mark.gpu

KINDS = [(16, False, {}), (16, True, {}), (32, False, {}), (16, False, dict(obstacle=2, obstacle_pos=[0.12, 0.0, 0.1])),
         (16, False, dict(warm_start=1)), (16, False, ROUND1)]
KIND_IDS = ["register-resident", "streamed-16", "links-32", "free-box", "warm-start", "contact-model-0"]


def friction(B):
    return (0.5 + np.arange(B) % 11 / 10.0).astype(np.float32)


@pytest.mark.parametrize("n,streamed,over", KINDS, ids=KIND_IDS)
def test_restore_continues_bit_for_bit(pkg, monkeypatch, n, streamed, over):
    _family(monkeypatch, streamed)
    B, A = 8, n // 2
    fr = friction(B)
    # envs 2 and 5 start their episodes from poses of their own (tests/test_gpu_reset_pose.py's); env 5's is lifted to
    # z = 0.5, so the height exit ends its episode in every env-step and the kernel reads its row of the table
    own = np.array([2, 5])
    P = default_rows(B, n)
    P[own] = random_poses(B, n, 31, qamp=0.3 if n == 16 else 0.08)[own]
    P[5, 2] = 0.5
    acts = [gait(pkg, B, j, A, 1.2) for j in range(4)]

    def make():
        return pkg.Stepper(B, n_modules=n, **over)

    def run(st, p):
        outs = [st.step(a[p].copy()) for a in acts[2:]]
        return outs, st.get_state()

    def check(got, ref, p):
        (outs, state), (routs, rstate) = got, ref
        for j, (x, y) in enumerate(zip(outs, routs)):
            for name, u, v in zip(("obs", "rew", "done", "sub"), x, y):
                assert np.array_equal(u, v[p]), (j, name)
        assert np.array_equal(state[0], rstate[0][p]) and np.array_equal(state[1], rstate[1][p])

    a_ = make()
    a_.set_ground_friction(fr)
    a_.set_reset_pose(P, np.isin(np.arange(B), own))
    a_.reset()
    for a in acts[:2]:
        a_.step(a.copy())
    snap = a_.snapshot()
    assert np.array_equal(snap.ground_friction, fr) and np.array_equal(snap.reset_pose, P)
    assert (snap.manifold is None) == (over.get("contact_model") == 0)
    assert (snap.box_state is None) == (snap.box_manifold is None) == (over.get("obstacle") != 2)
    ident = np.arange(B)
    ref = run(a_, ident)
    # not vacuous: an env with a pose of its own ended an episode in the compared steps and landed on ITS row
    ends = [j for j, out in enumerate(ref[0]) if out[2][5]]
    assert ends, "env 5 ended no episode in the compared steps"
    assert np.array_equal(ref[0][ends[-1]][0][5, 3 * n:3 * n + 7], P[5, :7])
    a_.close()

    b_ = make()
    b_.restore(snap)
    check(run(b_, ident), ref, ident)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    b_.restore(snap[perm])
    assert np.array_equal(b_.get_reset_pose(), P[perm]) and np.array_equal(b_.get_ground_friction(), fr[perm])
    check(run(b_, perm), ref, perm)
    b_.close()


def same_infos(x, y):
    assert len(x) == len(y)
    for i, (ix, iy) in enumerate(zip(x, y)):
        assert sorted(ix) == sorted(iy) == ['frames', 'internal_observations', 'link_positions']
        for key in ix:
            assert len(ix[key]) == len(iy[key]), (i, key)
            for s_, (u, v) in enumerate(zip(ix[key], iy[key])):
                assert u.dtype == v.dtype and np.array_equal(u, v), (i, key, s_)


@pytest.mark.parametrize("route", ["setter", "checkpoint"])
def test_replay_sees_friction_set_behind_the_env(pkg, tmp_path, route):
    """Friction that reaches the handle without SnakeVecEnv.set_ground_friction -- the stepper's own setter, or a
    checkpoint loaded into the env -- once left the replay's scratch handle on stale values: SystemError("test-mode replay
    diverged ...") for envs that went on, silently wrong telemetry for envs that finished.  The replay now starts from
    the step handle's own snapshot; the kernel's rows (telemetry='kernel') are the independent witness."""
    B = 4
    mu = np.array([0.5, 0.8, 1.2, 1.5], dtype=np.float32)
    repl = pkg.SnakeVecEnv(B, mode='test', telemetry='replay')
    kern = pkg.SnakeVecEnv(B, mode='test', telemetry='kernel')
    outs = []
    for j in range(3):
        a = gait(pkg, B, j, 8, 1.2)
        r, k = repl.step(a), kern.step(a)
        for u, v in zip(r[:3], k[:3]):
            assert np.array_equal(u, v), j
        same_infos(r[3], k[3])
        outs.append(r)
        if j == 0:
            assert repl._scratch is not None and kern._scratch is None       # the scratch handle exists: with ones
            if route == "setter":
                for env in (repl, kern):
                    env._stepper.set_ground_friction(mu)
            else:
                third = pkg.Stepper(B)
                third.set_ground_friction(mu)
                third.step(gait(pkg, B, 5, 8, 1.2))
                pkg.save_state(third, str(tmp_path / "third.npz"))
                third.close()
                for env in (repl, kern):
                    pkg.load_state(env, str(tmp_path / "third.npz"))
            for env in (repl, kern):
                assert np.array_equal(env._stepper.get_ground_friction(), mu)
    assert sum(len(info['internal_observations']) for r in outs[1:] for info in r[3]) > 0
    repl.close(); kern.close()
