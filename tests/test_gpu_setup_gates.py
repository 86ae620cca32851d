"""The setup phases of the register-resident substep branch on the contact count (wave-uniform gates around the second
friction batch and the groups of coupling scalars: snk_pgs_v2.hpp, substep_v2).  Each of the instantiations that contain
the substep -- the scheduled fused kernel, the unscheduled fused kernel (SNK_QUANTUM=0), the single-substep API -- is
compiled on its own, so a gate that leaves a row register in another state in ONE of them shows only in a cross-check
over contact counts on BOTH sides of every gate.  Same method as test_three_kernels_one_substep, but from the states
the bench's gait produces (persistent manifolds filled, real contact sets) instead of random flat poses, and with the
contact count of every compared state put into the bins the gates cut:  <= 8, 9-16, 17-32, 33-40, 41-48, > 48.

Under the gait 99 % of the substeps have 32 contacts or more (profiles/r04_contact_histogram.txt), so the low bins are
filled from the same gait states pitched about the base by a few milliradians, either way: the far end of the chain
leaves the reach of the breaking threshold and the manifolds there drop their points, link by link (the method of
test_partial_contact_sets).  An empty bin fails the test."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BINS = ((0, 8), (9, 16), (17, 32), (33, 40), (41, 48), (49, 64))
PITCH = (0.0, 0.001, -0.001, 0.002, -0.002, 0.004, -0.004, 0.008, -0.008, 0.016, -0.016, 0.03, -0.03)
N = 16


def gait_states(pkg, B, steps):
    """(state, contact cache) of B environments after `steps` env-steps of the bench's gait."""
    syn = importlib.import_module("bullet-envs_amd.synthetic")
    st = pkg.Stepper(B, n_modules=N)
    st.reset()
    for j in range(steps):
        st.step(syn.gait_actions(np.arange(B), j, N // 2).astype(np.float32))
    S, _ = st.get_state()
    Mf = st.get_manifold()
    st.close()
    return S, Mf


@pytest.mark.parametrize("streamed", [False, True])
def test_one_substep_bitwise_across_contact_count_bins(pkg, monkeypatch, streamed):
    syn = importlib.import_module("bullet-envs_amd.synthetic")
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
    # gait 2: one action per joint; the yaw joints get the gait's next command, the pitch joints stay at zero
    act = np.zeros((B, N), np.float32)
    act[:, 1::2] = np.concatenate([syn.gait_actions(np.arange(B0), 8, N // 2)] * len(PITCH)).astype(np.float32)
    over = dict(n_modules=N, gait=2, max_counter=0)      # max_counter 0: a fused env-step is exactly one substep

    def fused(quantum):
        monkeypatch.setenv("SNK_QUANTUM", quantum)
        st = pkg.Stepper(B, **over)
        st.set_state(S)
        st.set_manifold(Mf)
        obs, rew, done, sub = st.step(act.copy(), vec_mode=False)
        assert np.all(sub == 1)
        out = (st.get_state(), st.get_manifold(), done)
        st.close()
        return out

    # the contact counts come from the register-resident substep API (the bins are its gates'), whichever family is compared
    monkeypatch.delenv("SNK_FORCE_STREAMED", raising=False)
    monkeypatch.setenv("SNK_QUANTUM", "1")
    st = pkg.Stepper(B, **over)
    st.set_state(S)
    st.set_manifold(Mf)
    scale = np.float32(st.params.scaling_factor)
    nc = st.substep(act * scale, 1)[:, 1].copy()
    api = (st.get_state(), st.get_manifold())
    st.close()
    if streamed:
        monkeypatch.setenv("SNK_FORCE_STREAMED", "1")
        st = pkg.Stepper(B, **over)
        st.set_state(S)
        st.set_manifold(Mf)
        st.substep(act * scale, 1)
        api = (st.get_state(), st.get_manifold())
        st.close()
    (s0, x0), m0, done0 = fused("1")
    (s1, x1), m1, done1 = fused("0")
    # an env-step that ends in a termination resets the environment in the fused kernels, which the substep API does not do
    keep = ~done0 & ~done1
    counts = [int(np.sum(keep & (nc >= lo) & (nc <= hi))) for lo, hi in BINS]
    print("streamed %s: %d of %d states compared; contact counts per bin %s: %s" % (
        streamed, int(keep.sum()), B, ["%d-%d" % b for b in BINS], counts))
    assert all(c > 0 for c in counts), ("a contact-count bin is empty", BINS, counts)
    for (sa, xa), ma in (((s1, x1), m1), api):
        for lo, hi in BINS:
            sel = keep & (nc >= lo) & (nc <= hi)
            assert np.array_equal(s0[sel], sa[sel]), "states differ for %d..%d contacts" % (lo, hi)
            assert np.array_equal(x0[sel][:, :N], xa[sel][:, :N]), "motor torques differ for %d..%d contacts" % (lo, hi)
            assert np.array_equal(m0[sel], ma[sel]), "contact caches differ for %d..%d contacts" % (lo, hi)
