"""The device / host entry-point pairs (include/snk.h: snk_render, snk_link_states, snk_contacts, snk_copy_envs, snk_reset,
snk_step, snk_step_traced, snk_substep, snk_observe and their host forms) against each other: a host form is its device
form behind an upload and a download, so the two give the same bytes on handles in the same state; the staging arena the
host forms share, grown and reused without changing an answer; and the host forms' refusals word for word
(tests/golden/host_form_refusals.json, written on the commits before the host forms shared their scaffolding)."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_host_form_refusals", os.path.join(GOLDEN, "make_host_form_refusals.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

VARIANTS = ("16 register-resident", "16 streamed, free box", "32")
IDS = ([3, 0, 0], None)             # an id repeated and out of order; every env
W = H = 8


@pytest.fixture(scope="module")
def handles(pkg):
    """One handle per kernel variant, gen.N_ENVS envs after two gait steps."""
    pytest.importorskip("torch")
    out = {}
    for name, kw in zip(VARIANTS, gen.HANDLES):
        st = pkg.Stepper(gen.N_ENVS, **kw)
        st.reset()
        k = np.arange(st.act_dim)
        for j in range(2):
            st.step((-0.9 * np.sin((2 * k[None, :] + 1) * 4.0 + 0.2 * j + 0.37 * np.arange(gen.N_ENVS)[:, None])).astype(np.float32))
        out[name] = (st, pkg.DeviceWorld(stepper=st))
    yield out
    for st, _ in out.values():
        st.close()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("ids", IDS, ids=["ids_3_0_0", "all"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_render_host_and_device_forms_agree(pkg, handles, variant, ids):
    st, world = handles[variant]
    t, lib = world.torch, pkg._lib
    k = gen.N_ENVS if ids is None else len(ids)
    view, proj = lib.default_camera(W, H)
    host = st.render(view, proj, W, H, env_ids=ids, shadow=True)
    cams, shared = lib.camera_block(view, proj, k)
    d_cams = t.as_tensor(cams, device=world.device)
    d_ids = None if ids is None else t.tensor(ids, dtype=t.int32, device=world.device)
    dev = (t.zeros((k, H, W, 4), dtype=t.uint8, device=world.device), t.zeros((k, H, W), dtype=t.float32, device=world.device),
           t.zeros((k, H, W), dtype=t.int32, device=world.device))
    st.render_device(0 if ids is None else d_ids.data_ptr(), k, d_cams.data_ptr(), shared, W, H, lib.RENDER_SHADOW,
                     dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), t.cuda.current_stream(world.device).cuda_stream)
    t.cuda.synchronize()
    assert host[0].any()
    for name, a, b in zip(("rgba", "depth", "seg"), host, dev):
        assert same_bytes(a, b.cpu().numpy()), name


@pytest.mark.parametrize("ids", IDS, ids=["ids_3_0_0", "all"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_link_states_host_and_device_forms_agree(handles, variant, ids):
    st, world = handles[variant]
    host = st.link_states(ids)
    assert np.all(np.isfinite(host)) and host.any()
    assert same_bytes(host, world.link_states(ids).cpu().numpy())


@pytest.mark.parametrize("ids", IDS, ids=["ids_3_0_0", "all"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_contacts_host_and_device_forms_agree(handles, variant, ids):
    st, world = handles[variant]
    host = st.contacts(ids)
    assert host[2].sum() > 0 and host[0].shape[1] == 8 * st.n + (4 if variant == VARIANTS[1] else 0)
    for name, a, b in zip(("points", "force", "count"), host, world.contacts(ids)):
        assert same_bytes(a, b.cpu().numpy()), name


@pytest.mark.parametrize("reset_pose", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_copy_envs_host_and_device_forms_agree(pkg, handles, variant, reset_pose):
    st, world = handles[variant]
    t = world.torch
    src, dst = [3, 0], [1, 2]
    before = st.snapshot()
    pose = before.reset_pose.copy()
    pose[:, 0] = 0.1 * np.arange(gen.N_ENVS)                            # (every env's row of the reset-pose table its own)
    st.set_reset_pose(pose)
    before = st.snapshot()
    after = []
    for form in ("host", "device"):
        if form == "host":
            st.copy_envs(src, dst, reset_pose)
        else:
            world.fork(t.tensor(src, dtype=t.int32, device=world.device), t.tensor(dst, dtype=t.int32, device=world.device),
                       reset_pose)
            t.cuda.synchronize()
        after.append(st.snapshot())
        st.restore(before)
    fields = [f for f in pkg._lib.Snapshot.FIELDS if getattr(before, f) is not None]
    assert {"state", "aux", "ground_friction", "manifold", "reset_pose"} <= set(fields)
    assert ("box_state" in fields) == (variant == VARIANTS[1])
    for f in fields:
        assert same_bytes(getattr(after[0], f), getattr(after[1], f)), f
    assert same_bytes(after[0].state[dst], before.state[src]) and not same_bytes(before.state[dst], before.state[src])
    assert same_bytes(after[0].reset_pose[dst], before.reset_pose[src if reset_pose else dst])
    assert same_bytes(st.snapshot().state, before.state)               # (the handle is left as the other tests expect it)


@pytest.mark.parametrize("variant", VARIANTS)
def test_host_forms_refuse_in_the_recorded_words(pkg, handles, variant):
    """Every recorded refusal of the host forms, string for string."""
    with open(os.path.join(GOLDEN, "host_form_refusals.json")) as f:
        want = json.load(f)
    assert want["n_envs"] == gen.N_ENVS and len(want["refusals"]) == 31
    st, _ = handles[variant]
    before = st.snapshot()
    got = gen.refusals(pkg, st)
    assert sorted(got) == sorted(want["refusals"])
    for case in sorted(got):
        print("  %-44s %s" % (case, got[case]))
        assert got[case] == want["refusals"][case], case
    after = st.snapshot()                                               # a refused call writes nothing
    for f in pkg._lib.Snapshot.FIELDS:
        assert (getattr(before, f) is None) == (getattr(after, f) is None)
        assert getattr(before, f) is None or same_bytes(getattr(before, f), getattr(after, f)), f


def gait(st, j):
    k = np.arange(st.act_dim)
    return (-0.9 * np.sin((2 * k[None, :] + 1) * 4.0 + 0.2 * j + 0.37 * np.arange(st.n_envs)[:, None])).astype(np.float32)


@pytest.fixture(scope="module")
def twins(pkg, handles):
    """Per variant: a handle for the host forms, a DeviceVecEnv (a handle of its own) for the device forms, and the
    Snapshot -- the shared handle's, two gait steps in -- that both are restored to before every form."""
    out = {}
    for name, kw in zip(VARIANTS, gen.HANDLES):
        snap = handles[name][0].snapshot()
        host = pkg.Stepper(gen.N_ENVS, **kw)
        out[name] = (host, pkg.DeviceVecEnv(gen.N_ENVS, params=host.params), snap)
    yield out
    for host, env, _ in out.values():
        host.close()
        env.close()


def all_ones(t, shape, device):
    """a float32 tensor with every bit set: what snk_step_traced_host makes of its trace before the launch"""
    return t.full(shape, -1, dtype=t.int32, device=device).view(t.float32)


@pytest.mark.parametrize("variant", VARIANTS)
def test_moved_host_forms_and_device_forms_agree(pkg, twins, variant):
    """Reset with and without a mask, step, traced step, substep with k = 1 and k = 3 and the three read-outs: every
    output of the host form and the Snapshot behind it have the bytes of the device form's on a twin handle."""
    host, env, snap = twins[variant]
    world, t, lib, E = env.world, env.torch, pkg._lib, gen.N_ENVS
    mask = np.array([1, 0, 1, 0], np.uint8)
    actions = 1.7 * gait(host, 2)                                          # (beyond [-1, 1]: the clipping shows)
    assert np.abs(actions).max() > 1.0
    targets = (0.3 * np.sin(0.5 * np.arange(host.n)[None, :] + np.arange(E)[:, None])).astype(np.float32)

    def dev(x):
        return t.as_tensor(x, device=env.device)

    def step_dev(trace):
        a = dev(actions.copy())
        obs, rew, done = env.step(a, trace=trace)
        return (a, obs, rew, done, env.substeps) + (() if trace is None else (trace,))

    def step_host():
        a = actions.copy()
        obs, rew, done, sub = host.step(a)
        return a, obs, rew, done.astype(np.uint8), sub

    def traced_host():
        a = actions.copy()
        obs, rew = np.empty((E, host.obs_dim), np.float32), np.empty(E, np.float32)
        done, sub = np.empty(E, np.uint8), np.empty(E, np.int32)
        trace = np.full(host.trace_shape(), 7.0, np.float32)             # (a caller's buffer that held something else)
        lib.check(host.lib.snk_step_traced_host(host.h, lib.fptr(a), lib.fptr(obs), lib.fptr(rew),
                                                done.ctypes.data_as(lib._U8), sub.ctypes.data_as(lib._I32), lib.fptr(trace),
                                                trace.shape[1], 1), "snk_step_traced_host")
        rows = np.arange(trace.shape[1])[None, :] >= sub[:, None]
        assert sub.min() >= 1 and rows.any() and np.isnan(trace[rows]).all()      # at and beyond an env's count: NaN
        assert np.isfinite(trace[~rows][:, :host.obs_dim + 3 * (host.n + 1)]).all()
        return a, obs, rew, done, sub, trace

    def reset_host(m):
        """snk_reset_host on an obs buffer that holds something: rows of unmasked envs come back as they went"""
        obs = np.full((E, host.obs_dim), 3.5, np.float32)
        lib.check(host.lib.snk_reset_host(host.h, None if m is None else m.ctypes.data_as(lib._U8), lib.fptr(obs)),
                  "snk_reset_host")
        assert m is None or ((obs[m == 0] == 3.5).all() and (obs[m != 0] != 3.5).any(axis=1).all())
        return (obs,)

    def reset_dev(m):
        out = t.full((E, host.obs_dim), 3.5, dtype=t.float32, device=env.device)
        return (world.reset(None if m is None else dev(m), out=out),)

    def substep_dev(k):
        info = t.zeros((E, 2), dtype=t.int32, device=env.device)
        world.step_simulation(dev(targets), k, info=info)
        return (info,)

    forms = {
        "reset": (lambda: reset_host(None), lambda: reset_dev(None)),
        "reset, masked": (lambda: reset_host(mask), lambda: reset_dev(mask)),
        "step": (step_host, lambda: step_dev(None)),
        "step_traced": (traced_host, lambda: step_dev(all_ones(t, host.trace_shape(), env.device))),
        "substep k=1": (lambda: (host.substep(targets, 1),), lambda: substep_dev(1)),
        "substep k=3": (lambda: (host.substep(targets, 3),), lambda: substep_dev(3)),
        "get_obs": (lambda: (host.get_obs(),), lambda: (world.observation(),)),
        "mean_height": (lambda: (host.mean_height(),), lambda: (world.mean_height(),)),
        "link_positions": (lambda: (host.link_positions(),), lambda: (world.link_positions(),)),
    }
    fields = [f for f in lib.Snapshot.FIELDS if getattr(snap, f) is not None]
    for name, (host_form, device_form) in forms.items():
        host.restore(snap)
        env.stepper.restore(snap)
        a = host_form()
        b = device_form()
        t.cuda.synchronize()
        assert len(a) == len(b) and any(np.asarray(x).any() for x in a), name
        for i, (x, y) in enumerate(zip(a, b)):
            assert same_bytes(x, y.cpu().numpy()), (name, i)
        after = host.snapshot(), env.stepper.snapshot()
        for f in fields:
            assert same_bytes(getattr(after[0], f), getattr(after[1], f)), (name, f)
        moved = not same_bytes(after[0].state, snap.state)
        assert moved == (name not in ("get_obs", "mean_height", "link_positions")), name


@pytest.mark.parametrize("variant", VARIANTS)
def test_staging_arena_grows_without_changing_an_answer(pkg, handles, variant):
    """The read-only host forms on ONE handle, from the few bytes of the read-outs up to a 32 x 32 render of every env
    (the arena is replaced on the way up) and down again (it is reused, larger than needed): every pair of results has
    the same bytes, and they are those of a fresh handle, whose arena starts at the largest size."""
    snap = handles[variant][0].snapshot()
    view = {w: pkg._lib.default_camera(w, w) for w in (8, 32)}

    def calls(st):
        return [lambda: (st.get_obs(),), lambda: (st.mean_height(),), lambda: (st.link_positions(),),
                lambda: (st.link_states(),), st.contacts, st.dynamics,
                lambda: (st.jacobians(np.arange(3 * st.n + 2)),),
                lambda: st.render(*view[8], 8, 8), lambda: st.render(*view[32], 32, 32)]

    results = []
    for order in ("up and down", "down"):
        st = pkg.Stepper(gen.N_ENVS, **gen.HANDLES[VARIANTS.index(variant)])
        try:
            st.restore(snap)
            cs = calls(st)
            if order == "up and down":
                results.append([c() for c in cs])
            results.append([c() for c in cs[::-1]][::-1])
        finally:
            st.close()
    for i, parts in enumerate(results[0]):
        assert any(np.asarray(x).any() for x in parts), i
        for other in results[1:]:
            assert len(other[i]) == len(parts)
            for x, y in zip(parts, other[i]):
                assert same_bytes(x, y), i
