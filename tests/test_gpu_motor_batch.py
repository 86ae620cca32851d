"""With at most 48 contacts the register-resident substep builds its sixteen motor rows in lanes 48..63 of the normals'
batch instead of in a batch of their own (snk_pgs_v2.hpp: build_batch_v2, KIND 5).  Every lane does there what it did
before, so nothing may change: SNK_MOTORS_APART=1 (read by snk_create) keeps the old sequence at every contact count, and
both sequences must give the same bits -- in the fused kernel and in the single-substep API, on both sides of the
48 | 49 cut and of every other gate of the setup phases.  States, pitches and bins are test_gpu_setup_gates.py's; an empty
bin fails the test.  A second case runs four gait env-steps of 1000 environments either way."""
import importlib

import numpy as np
import pytest

from test_gpu_setup_gates import BINS, N, PITCH, gait_states

pytestmark = pytest.mark.gpu


def test_motor_rows_in_the_normals_batch_bitwise_per_contact_bin(pkg, monkeypatch):
    syn = importlib.import_module("bullet-envs_amd.synthetic")
    monkeypatch.delenv("SNK_FORCE_STREAMED", raising=False)
    monkeypatch.delenv("SNK_MOTORS_APART", raising=False)
    monkeypatch.setenv("SNK_QUANTUM", "1")
    B0 = 384
    S0, M0 = gait_states(pkg, B0, 8)
    S = np.concatenate([S0] * len(PITCH)).astype(np.float32)
    Mf = np.concatenate([M0] * len(PITCH)).astype(np.float32)
    for i, ang in enumerate(PITCH):
        # q <- (rotation by ang about the world's y axis) x q, quaternions as [x, y, z, w]: the chain turns about the base
        blk = S[i * B0:(i + 1) * B0]
        x, y, z, w = (blk[:, 3 + j].astype(np.float64) for j in range(4))
        sy, cw = np.sin(ang / 2), np.cos(ang / 2)
        blk[:, 3:7] = np.stack([cw * x + sy * z, cw * y + sy * w, cw * z - sy * x, cw * w - sy * y], axis=1).astype(np.float32)
    B = len(S)
    act = np.zeros((B, N), np.float32)
    act[:, 1::2] = np.concatenate([syn.gait_actions(np.arange(B0), 8, N // 2)] * len(PITCH)).astype(np.float32)
    over = dict(n_modules=N, gait=2, max_counter=0)      # max_counter 0: a fused env-step is exactly one substep

    def both(apart):
        if apart:
            monkeypatch.setenv("SNK_MOTORS_APART", "1")
        else:
            monkeypatch.delenv("SNK_MOTORS_APART", raising=False)
        st = pkg.Stepper(B, **over)
        st.set_state(S)
        st.set_manifold(Mf)
        obs, rew, done, sub = st.step(act.copy(), vec_mode=False)
        assert np.all(sub == 1)
        fused = (st.get_state(), st.get_manifold(), done, obs, rew)
        st.set_state(S, np.zeros((B, N + 2), np.float32))
        st.set_manifold(Mf)
        info = st.substep(act * np.float32(st.params.scaling_factor), 1)
        api = (st.get_state(), st.get_manifold(), info)
        st.close()
        return fused, api

    (f0, a0), (f1, a1) = both(False), both(True)
    nc = a1[2][:, 1]
    assert np.array_equal(nc, a0[2][:, 1]) and np.array_equal(a0[2][:, 0], a1[2][:, 0])
    counts = [int(np.sum((nc >= lo) & (nc <= hi))) for lo, hi in BINS]
    print("contact counts per bin %s: %s" % (["%d-%d" % b for b in BINS], counts))
    assert all(c > 0 for c in counts), ("a contact-count bin is empty", BINS, counts)
    for lo, hi in BINS:
        sel = (nc >= lo) & (nc <= hi)
        what = "for %d..%d contacts" % (lo, hi)
        for name, (x0, x1) in (("fused", (f0, f1)), ("substep API", (a0, a1))):
            (s0, t0), m0 = x0[0], x0[1]
            (s1, t1), m1 = x1[0], x1[1]
            assert np.array_equal(s0[sel], s1[sel]), "%s: states differ %s" % (name, what)
            assert np.array_equal(t0[sel][:, :N], t1[sel][:, :N]), "%s: motor torques differ %s" % (name, what)
            assert np.array_equal(m0[sel], m1[sel]), "%s: contact caches differ %s" % (name, what)
        assert np.array_equal(f0[2][sel], f1[2][sel]), "done flags differ %s" % what
        assert np.array_equal(f0[3][sel], f1[3][sel]) and np.array_equal(f0[4][sel], f1[4][sel]), "outputs differ %s" % what


def test_motor_rows_in_the_normals_batch_bitwise_over_gait_steps(pkg, monkeypatch):
    syn = importlib.import_module("bullet-envs_amd.synthetic")
    monkeypatch.delenv("SNK_FORCE_STREAMED", raising=False)
    B = 1000

    def run(apart):
        if apart:
            monkeypatch.setenv("SNK_MOTORS_APART", "1")
        else:
            monkeypatch.delenv("SNK_MOTORS_APART", raising=False)
        st = pkg.Stepper(B, n_modules=N)
        st.reset()
        st.set_ground_friction((0.5 + np.arange(B) % 11 / 10.0).astype(np.float32))
        outs = [st.step(syn.gait_actions(np.arange(B), j, N // 2).astype(np.float32)) for j in range(4)]
        S, X = st.get_state()
        Mf = st.get_manifold()
        st.close()
        return outs, S, X, Mf

    o0, S0, X0, M0 = run(False)
    o1, S1, X1, M1 = run(True)
    for j, (a, b) in enumerate(zip(o0, o1)):
        for name, x, y in zip(("obs", "reward", "done", "substeps"), a, b):
            assert np.array_equal(x, y), "env-step %d: %s differ" % (j, name)
    assert np.array_equal(S0, S1) and np.array_equal(X0, X1) and np.array_equal(M0, M1)
