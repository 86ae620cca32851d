"""GPU tests of the two solver rules the kernels take since ABI 7: snk_params::noncontact_order 1 (the limit
and motor rows in the order of Bullet's quickSort on equal island ids: the motors first, then the violated limits, both in
one fixed permutation, swept alternately backwards / forwards) and snk_params::contact_erp_rule 1 (a contact row takes
limit_erp unless it is deeper than the split-impulse threshold).  Every switch set runs on the three kernel families --
16 links register-resident, 16 links streamed rows (SNK_FORCE_STREAMED), 32 links -- against the float64 oracle under
the same switches, with the float32 oracle as the yardstick."""
import numpy as np
import pytest

from conftest import f32_gate, mismatch_gate
from test_gpu_accuracy_distribution import _check
from test_gpu_contact_models import _same_manifold

pytestmark = pytest.mark.gpu

SETS = {
    "nco": dict(noncontact_order=1),
    "erp": dict(contact_erp_rule=1),
    "both-qsorts": dict(noncontact_order=1, contact_order=2),
    "as-read": dict(noncontact_order=1, contact_order=2, contact_erp_rule=1),
}
FAMILIES = [(16, False), (16, True), (32, False)]          # (n, SNK_FORCE_STREAMED)


def _family(monkeypatch, streamed):
    if streamed:
        monkeypatch.setenv("SNK_FORCE_STREAMED", "1")
    else:
        monkeypatch.delenv("SNK_FORCE_STREAMED", raising=False)


def _gait_states(pkg, n, B, over):
    """States and contact caches the gait produces under `over` (two env-steps from the reset pose), and the next
    env-step's joint targets."""
    import bench
    st = pkg.Stepper(B, residual_threshold=0.0, **over)
    st.reset()
    ids = np.arange(B)
    for j in range(2):
        st.step(bench.gait_actions(ids, j, n // 2).astype(np.float32), vec_mode=False)
    S, X = st.get_state()
    Mf = st.get_manifold()
    T = np.zeros((B, n), np.float32)
    T[:, 1::2] = (bench.gait_actions(ids, 2, n // 2) * (np.pi / 6)).astype(np.float32)
    return st, S, Mf, T


def _oracle(oracle_mod, S, Mf, f32=False, **over):
    e = oracle_mod.OracleEnv(residual_threshold=0.0, max_contacts=0, f32=f32, **over)
    e.set_state(S.astype(np.float64))
    e.set_manifold(Mf.astype(np.float64))
    return e


@pytest.mark.parametrize("n,streamed", FAMILIES)
@pytest.mark.parametrize("name", list(SETS))
def test_substep_parity_from_gait_states(pkg, oracle_mod, monkeypatch, name, n, streamed):
    """K substeps from states the gait produces: state, contact cache, motor torques and the joint-0 force sensor against
    the float64 oracle under the same switches (cache flips gated by the float32 oracle's own); then the switch is shown
    to be honoured: after one substep the GPU is far closer to the oracle WITH the switch than to the oracle without it
    (median over the environments; sized on the CPU: the switches move a gait state 30x (contact_erp_rule) to 2000x
    (noncontact_order) farther than float32 round-off after one substep)."""
    _family(monkeypatch, streamed)
    B, K = (16, 3) if n == 16 else (8, 3)
    over = dict(n_modules=n, self_collision=0, **SETS[name])
    st, S, Mf, T = _gait_states(pkg, n, B, over)
    assert Mf[:, :, 0].sum() > B * n // 2
    refs = [_oracle(oracle_mod, S[i], Mf[i], **over) for i in range(B)]
    refs32 = [_oracle(oracle_mod, S[i], Mf[i], f32=True, **over) for i in range(B)]
    worst = dict(p=0.0, v=0.0, tau=0.0, f=0.0)
    cal = dict(p=0.0, v=0.0, tau=0.0, f=0.0)
    bad = bad32 = 0
    alive, alive32 = np.ones(B, bool), np.ones(B, bool)
    first = None
    for k in range(K):
        info = st.substep(T, 1)
        G, GX = st.get_state()
        M = st.get_manifold()
        if k == 0:
            first = G.copy()
        for i in range(B):
            e, e32 = refs[i], refs32[i]
            e.substep(T[i].astype(np.float64))
            e32.substep(T[i].astype(np.float64))
            if not alive[i]:
                continue
            r = e.get_state()
            ta, fa, _ = e.get_aux()
            if e32.last_num_contacts == e.last_num_contacts:
                r32 = e32.get_state()
                tb, fb, _ = e32.get_aux()
                cal["p"] = max(cal["p"], np.abs(r32[:7] - r[:7]).max(), np.abs(r32[13:13 + n] - r[13:13 + n]).max())
                cal["v"] = max(cal["v"], (np.abs(r32[13 + n:] - r[13 + n:]) / (1 + np.abs(r[13 + n:]))).max())
                cal["tau"] = max(cal["tau"], np.abs(tb - ta).max() / (1 + np.abs(ta).max()))
                cal["f"] = max(cal["f"], abs(fb - fa))
            if alive32[i] and not (e32.last_num_contacts == e.last_num_contacts
                                   and _same_manifold(e32.get_manifold(), e.get_manifold(), n)):
                alive32[i] = False
                bad32 += 1
            if not (e.last_num_contacts == info[i, 1] and _same_manifold(M[i], e.get_manifold(), n)):
                alive[i] = False
                bad += 1
                continue
            worst["p"] = max(worst["p"], np.abs(G[i, :7] - r[:7]).max(), np.abs(G[i, 13:13 + n] - r[13:13 + n]).max())
            worst["v"] = max(worst["v"], (np.abs(G[i, 13 + n:] - r[13 + n:]) / (1 + np.abs(r[13 + n:]))).max())
            worst["tau"] = max(worst["tau"], np.abs(GX[i, :n] - ta).max() / (1 + np.abs(ta).max()))
            worst["f"] = max(worst["f"], abs(float(GX[i, n]) - fa))
    what = "%s n = %d%s" % (name, n, " streamed" if streamed else "")
    print(what, "worst", worst, "| float32 oracle", cal, "| cache flips", bad, "(float32 oracle:", bad32, ")")
    mismatch_gate("%s: cache flips" % what, bad, bad32, 1.5, 2)
    assert bad <= B // 2
    f32_gate("%s: worst pos" % what, worst["p"], cal["p"], 2.0, 1e-4, 5e-3)
    f32_gate("%s: worst rel qd" % what, worst["v"], cal["v"], 2.0, 1e-2, 1.0)
    f32_gate("%s: motor torques" % what, worst["tau"], cal["tau"], 2.0, 1e-2, 1.0)
    f32_gate("%s: sensor force" % what, worst["f"], cal["f"], 2.0, 0.02, 0.5)
    # the switch is honoured: one substep, oracle with the switches against oracle without them (contact_order kept)
    base = {k: v for k, v in over.items() if k not in ("noncontact_order", "contact_erp_rule")}
    moved, near = [], []
    for i in range(B):
        w = _oracle(oracle_mod, S[i], Mf[i], **over)
        wo = _oracle(oracle_mod, S[i], Mf[i], **base)
        w.substep(T[i].astype(np.float64))
        wo.substep(T[i].astype(np.float64))
        a, b = w.get_state(), wo.get_state()
        rel = lambda x: (np.abs(x[13 + n:] - a[13 + n:]) / (1 + np.abs(a[13 + n:]))).max()      # noqa: E731
        moved.append(rel(b))
        near.append(rel(first[i].astype(np.float64)))
    print("  %s: oracle with / without the switch after one substep: rel qd %.3e (median); GPU from the oracle with it: %.3e"
          % (what, np.median(moved), np.median(near)))
    assert np.median(moved) > 8 * np.median(near), (np.median(moved), np.median(near))
    st.close()


@pytest.mark.parametrize("n,streamed", FAMILIES)
def test_violated_limits(pkg, oracle_mod, monkeypatch, n, streamed):
    """Joint angles up to 1.7 rad (past the 1.57 limits): limit rows enter the permuted list and are swept both ways; the
    distribution gate on joint velocities, motor torques and the joint-0 sensor (which sums the rows in list order)."""
    _family(monkeypatch, streamed)
    # (the 32-link chain folded sits near the p90 gate under the DEFAULT rules too -- 1.99 x the float32 oracle's at K = 3
    #  over 1024 states -- so it takes the 1024 states of the other 32-link distribution tests: over 256, p90 is noise)
    _check("%d links%s folded, noncontact_order 1 + contact_erp_rule 1" % (n, " streamed" if streamed else ""), pkg,
           oracle_mod, n, 1024 if n == 32 else 256, 4340 + n + streamed, dict(noncontact_order=1, contact_erp_rule=1),
           qamp=1.7)


@pytest.mark.parametrize("n", [16, 32])
def test_distribution_under_the_as_read_set(pkg, oracle_mod, n):
    """>= 512 random ground states per chain under the full as-read set, as test_another_sweep_order_of_the_manifolds."""
    _check("%d links, as-read rules" % n, pkg, oracle_mod, n, 512, 4350 + n, dict(SETS["as-read"]))


@pytest.mark.parametrize("n", [16, 32])
def test_env_step_parity_under_the_as_read_set(pkg, oracle_mod, n):
    """Env-steps of the gait: substep counts, rewards and done flags against the float64 oracle started from the GPU's
    state every step (count / done mismatches gated by the float32 oracle's)."""
    import bench
    over = dict(n_modules=n, **SETS["as-read"])
    B, A = 16, n // 2
    st = pkg.Stepper(B, **over)
    st.reset()
    ids = np.arange(B)
    mis = mis32 = compared = 0
    worst_r = cal_r = 0.0
    for j in range(4):
        a = bench.gait_actions(ids, j, A).astype(np.float32)
        S, X = st.get_state()
        Mf = st.get_manifold()
        o, r, d, s = st.step(a, vec_mode=False)
        for i in range(B):
            res = []
            for f32 in (False, True):
                e = oracle_mod.OracleEnv(f32=f32, **over)
                e.sync(S[i].astype(np.float64), X[i].astype(np.float64), Mf[i].astype(np.float64))
                res.append(e.env_step(a[i].astype(np.float64), vec_mode=False))
            (ro, rr, rd, rk, _), (qo, qr, qd, qk, _) = res
            if rk != qk or rd != qd:
                mis32 += 1
            if rk != int(s[i]) or rd != bool(d[i]):
                mis += 1
                continue
            compared += 1
            worst_r = max(worst_r, abs(float(r[i]) - rr))
            if qk == rk and qd == rd:
                cal_r = max(cal_r, abs(qr - rr))
    print("env-steps n = %d: compared %d, mismatches %d (float32 oracle %d), worst reward %.3e (float32 oracle %.3e)"
          % (n, compared, mis, mis32, worst_r, cal_r))
    mismatch_gate("as-read env-steps n = %d: count / done" % n, mis, mis32, 1.5, 4)
    assert compared >= B
    f32_gate("as-read env-steps n = %d: worst reward" % n, worst_r, cal_r, 2.0, 1e-3, 5e-2)
    st.close()


def test_schedule_and_checkpoint_under_the_switches(pkg, monkeypatch, tmp_path):
    """With the switches on, results do not depend on the in-launch schedule (SNK_QUANTUM 0 = unscheduled, 1, 3), and a
    checkpoint (which carries both fields by name) resumes bit for bit."""
    import bench
    B = 3000
    ids = np.arange(B)
    over = dict(SETS["as-read"])

    def run(quantum, ckpt=None):
        monkeypatch.setenv("SNK_QUANTUM", str(quantum))
        st = pkg.Stepper(B, **over)
        st.reset()
        outs = []
        for j in range(4):
            if ckpt is not None and j == 2:
                pkg.save_state(st, ckpt)
            o, r, d, s = st.step((bench.gait_actions(ids, j) * 1.1).astype(np.float32))
            outs.append((o.copy(), r.copy(), d.copy(), s.copy()))
        S, X = st.get_state()
        M = st.get_manifold()
        st.close()
        return outs, S, X, M

    path = str(tmp_path / "rules.npz")
    ref, S0, X0, M0 = run(0, ckpt=path)
    for quantum in (1, 3):
        got, S, X, M = run(quantum)
        for g, w in zip(got, ref):
            for x, y in zip(g, w):
                assert np.array_equal(x, y)
        assert np.array_equal(S, S0) and np.array_equal(X, X0) and np.array_equal(M, M0)
    monkeypatch.setenv("SNK_QUANTUM", "1")
    st = pkg.Stepper(B, **over)
    pkg.load_state(st, path)
    for j in (2, 3):
        o, r, d, s = st.step((bench.gait_actions(ids, j) * 1.1).astype(np.float32))
        assert np.array_equal(o, ref[j][0]) and np.array_equal(r, ref[j][1]) and np.array_equal(s, ref[j][3])
    st.close()
    # ... and a handle with the defaults refuses it
    st = pkg.Stepper(4)
    with pytest.raises(ValueError):
        pkg.load_state(st, path)
    st.close()


def test_rules_off_are_the_default_bits(pkg, monkeypatch):
    """contact_erp_rule 0 on the kernels compiled for noncontact_order 1 reads the same ERP at any depth; and the default
    kernels are untouched: a handle with both fields 0 given explicitly is the default handle, bit for bit."""
    import bench
    B = 64
    ids = np.arange(B)
    outs = []
    for over in (dict(), dict(noncontact_order=0, contact_erp_rule=0)):
        st = pkg.Stepper(B, **over)
        st.reset()
        o = [st.step(bench.gait_actions(ids, j).astype(np.float32)) for j in range(3)]
        outs.append([x.copy() for t in o for x in t])
        st.close()
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("cls", ["SnakeVecEnv", "DeviceVecEnv", "SubprocVecEnv", "test-mode"])
def test_the_switches_travel_through_every_seam(pkg, cls):
    over = dict(SETS["as-read"])
    if cls == "SnakeVecEnv":
        env = pkg.SnakeVecEnv(4, **over)
        ps = [env._stepper.params]
    elif cls == "DeviceVecEnv":
        env = pkg.DeviceVecEnv(4, **over)
        ps = [env.stepper.params]
    elif cls == "SubprocVecEnv":
        env = pkg.SubprocVecEnv([lambda: pkg.SnakeGymEnv(**over) for _ in range(3)])
        ps = [pkg.checkpoint._stepper(env).params]
    else:
        import argparse
        args = argparse.Namespace(alpha=1.0, beta=0.01, gamma=0.1, mode="test", gaitSelection=1, scaling_factor=6,
                                  motorVelocityLimit=np.inf, motorTorqueLimit=np.inf)
        env = pkg.SnakeGymEnv(args=args, **over)
        env.reset()
        env.step(np.zeros(env._stepper.act_dim, np.float32))
        assert getattr(env, "_scratch", None) is not None          # the replay handle of test mode
        ps = [env.params, env._stepper.params, env._scratch.params]
    for p in ps:
        for k, v in over.items():
            assert getattr(p, k) == v, (cls, k)
    env.close()
