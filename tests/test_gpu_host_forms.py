"""The four device / host entry-point pairs (include/snk.h: snk_render, snk_link_states, snk_contacts, snk_copy_envs and
their _host forms) against each other: a host form is its device form behind an upload and a download, so the two give
the same bytes on the same handle in the same state; and the host forms' id and count refusals word for word
(tests/golden/host_form_refusals.json, written on the commit before the host forms shared their scaffolding)."""
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
    """Every id and count refusal of the four host forms, string for string."""
    with open(os.path.join(GOLDEN, "host_form_refusals.json")) as f:
        want = json.load(f)
    assert want["n_envs"] == gen.N_ENVS and len(want["refusals"]) == 15
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
