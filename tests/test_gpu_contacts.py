"""The reported contacts on the GPU (include/snk.h, "The reported contacts": snk_contacts; csrc/snk_world.hpp:
contacts_kernel) against tests/np_contacts.py, the numpy model written from the header: synthetic caches on both chain
lengths and with the free box, the read-out behind real physics bit for bit, the weight a resting snake and box put on
their contact points, the rules of the tensor seam, and BulletClient.getContactPoints on the kernels.

Handles hold at most 24 envs.  Tolerances (test 1 and 2):
  exact    live flags, cylinder and slot indices, count, ground points, normals, the impulse; dead slots are zero WORDS;
  points   world point and distance through conftest.f32_gate against the float32 twin of the model: factor 3, floor
           1e-6 m, cap 1e-4 m -- the link-state gate's figures (tests/test_gpu_world.py) for the same reason: the kernel
           composes n + 1 composite-body frames plus one fixed offset, the twin the 3n + 2-link tree;
  force    impulse / dt is one correctly rounded float32 division: within 2^-22 relative of float64(impulse) /
           float64(float32(dt)) (2^-24 would be half an ulp; two ulps leave room for a reciprocal-multiply form);
  sums     a cylinder's force adds at most four such terms in float32: within 2^-21 x sum |f|.
A run's GATE lines are profiles/r16_contacts_accuracy.txt."""
import numpy as np
import pytest

import np_contacts as npc
from conftest import f32_gate, random_state      # noqa: E402
from test_gpu_world import STATE_FIELDS, bits, gait, same_bits, snap_equal

pytestmark = pytest.mark.gpu

E = 24


def model_params(st):
    """np_contacts' params of a handle: dt as the kernels hold it (float32), cyl_zoff from snk_params_derived."""
    import ctypes as C
    out = (C.c_double * 6)()
    assert st.lib.snk_params_derived(C.byref(st.params), out) == 0
    return dict(n=st.n, dt=float(np.float32(st.params.dt)), cyl_zoff=out[3])


def synthetic_cache(rng, n, envs):
    """[envs, 2n, 29] float32: counts 0 .. 4 per cylinder (env 0: every count 0; env 1: every count 4), link-frame points
    across the collider, ground points around the origin, impulses; the slots beyond a count are filled too -- the cache
    keeps stale points there (snk_set_manifold stores them), the read-out must not show them."""
    M = np.zeros((envs, 2 * n, 29), np.float32)
    M[:, :, 0] = rng.integers(0, 5, (envs, 2 * n))
    M[0, :, 0], M[1, :, 0] = 0, 4
    pts = M[:, :, 1:].reshape(envs, 2 * n, 4, 7)
    pts[..., 0:3] = rng.uniform(-0.03, 0.03, pts[..., 0:3].shape)
    pts[..., 3:5] = rng.uniform(-1.5, 1.5, pts[..., 3:5].shape)
    pts[..., 6] = rng.uniform(0.0, 0.5, pts[..., 6].shape)
    return M


def synthetic_box(rng, envs):
    """(state [envs, 13], manifold [envs, 29]) float32: a tumbled box somewhere, counts 0 .. 4 (env 0: 0, env 1: 4)."""
    bs = np.zeros((envs, 13), np.float32)
    bs[:, 0:3] = rng.uniform(-1.0, 1.0, (envs, 3))
    q = rng.normal(size=(envs, 4))
    bs[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    bm = np.zeros((envs, 29), np.float32)
    bm[:, 0] = rng.integers(0, 5, envs)
    bm[0, 0], bm[1, 0] = 0, 4
    pts = bm[:, 1:].reshape(envs, 4, 7)
    pts[..., 0:3] = rng.uniform(-0.4, 0.4, pts[..., 0:3].shape)
    pts[..., 3:5] = rng.uniform(-1.5, 1.5, pts[..., 3:5].shape)
    pts[..., 6] = rng.uniform(0.0, 9.0, pts[..., 6].shape)
    return bs, bm


def read_on_device(torch, st, ids, rows, slots, canary=-7.0):
    """snk_contacts into canary-filled tensors one row longer than asked for: (points, force, count) as numpy, whole."""
    dev = torch.device("cuda", 0)
    pts = torch.full((rows + 1, slots, 16), canary, dtype=torch.float32, device=dev)
    frc = torch.full((rows + 1, 2 * st.n + 1), canary, dtype=torch.float32, device=dev)
    cnt = torch.full((rows + 1,), -77, dtype=torch.int32, device=dev)
    idt = None if ids is None else torch.tensor(ids, dtype=torch.int32, device=dev)
    st.contacts_device(idt.data_ptr() if idt is not None else 0, rows, pts.data_ptr(), frc.data_ptr(), cnt.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return pts.cpu().numpy(), frc.cpu().numpy(), cnt.cpu().numpy()


def check_against_the_model(what, got, S, M, box, params):
    """The exact part asserted, the float32 part gated; `got` = (points [envs, slots, 16], force, count)."""
    pts, frc, cnt = got
    n = params["n"]
    envs = len(S)
    dt64 = float(params["dt"])
    worst = dict(point=[0.0, 0.0], dist=[0.0, 0.0])
    live_total = 0
    for e in range(envs):
        bx = None if box is None else (box[0][e], box[1][e])
        ref, rforce, rcount = npc.reference(S[e], M[e], bx, params)
        tw, _, _ = npc.twin(S[e], M[e], bx, params)
        assert pts[e].shape == ref.shape
        live = ref[:, 14] == 1.0
        live_total += int(live.sum())
        assert cnt[e] == rcount == live.sum(), (what, e, cnt[e], rcount)
        assert not bits(pts[e][~live]).any(), (what, e, "a dead slot is not sixteen zero words")
        g = pts[e][live]
        r = ref[live]
        for cols in ((3, 6), (6, 9), (11, 16)):                       # ground point, normal, impulse, c, j, live, 0
            assert np.array_equal(g[:, cols[0]:cols[1]].astype(np.float64), r[:, cols[0]:cols[1]]), (what, e, cols)
        if live.any():
            t = tw[live].astype(np.float64)
            g64 = g.astype(np.float64)
            worst["point"] = [max(worst["point"][0], np.linalg.norm(g64[:, 0:3] - r[:, 0:3], axis=1).max()),
                              max(worst["point"][1], np.linalg.norm(t[:, 0:3] - r[:, 0:3], axis=1).max())]
            worst["dist"] = [max(worst["dist"][0], np.abs(g64[:, 9] - r[:, 9]).max()),
                             max(worst["dist"][1], np.abs(t[:, 9] - r[:, 9]).max())]
            f64 = r[:, 11] / dt64
            assert np.all(np.abs(g64[:, 10] - f64) <= 2.0 ** -22 * np.abs(f64)), (what, e, "force")
        # per unit: the sum of its live slots' forces
        units = 2 * n + (1 if box is not None else 0)
        for c in range(units):
            f = ref[4 * c:4 * c + 4, 11] / dt64 * ref[4 * c:4 * c + 4, 14]
            assert abs(float(frc[e, c]) - f.sum()) <= 2.0 ** -21 * np.abs(f).sum(), (what, e, c, frc[e, c], f.sum())
        if box is None:
            assert frc[e, 2 * n] == 0.0 and not bits(frc[e, 2 * n:2 * n + 1]).any()
    for k in ("point", "dist"):
        f32_gate("contacts %s: %s (worst of %d live slots)" % (what, k, live_total), worst[k][0], worst[k][1], factor=3.0,
                 floor=1e-6, cap=1e-4)
    return live_total


# ----------------------------------------------------------------------------------------------------------------------
# 1. synthetic caches, both chain lengths
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 32])
def test_synthetic_caches_match_the_independent_model(pkg, n):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1600 + n)
    S = np.stack([random_state(rng, n, z=0.3, qamp=1.5, vamp=1.0) for _ in range(E)]).astype(np.float32)
    M = synthetic_cache(rng, n, E)
    st = pkg.Stepper(E, n_modules=n)
    assert st.contact_slots == 8 * n
    st.set_state(S, None)
    st.set_manifold(M)
    params = model_params(st)
    host = st.contacts()
    dev = read_on_device(torch, st, None, E, 8 * n)
    st.close()
    assert host[0].shape == (E, 8 * n, 16) and host[1].shape == (E, 2 * n + 1) and host[2].shape == (E,)
    # the two forms are one kernel; the row beyond the request keeps its canaries
    assert same_bits(host[0], dev[0][:E]) and same_bits(host[1], dev[1][:E]) and np.array_equal(host[2], dev[2][:E])
    assert np.all(dev[0][E] == -7.0) and np.all(dev[1][E] == -7.0) and dev[2][E] == -77
    live = check_against_the_model("n=%d" % n, (dev[0][:E], dev[1][:E], dev[2][:E]), S, M, None, params)
    assert dev[2][0] == 0 and dev[2][1] == 8 * n and live > 8 * n      # the empty env, the full env (all 8n slots live)


def test_model_params_of_a_handle_are_the_headers(pkg):
    """dt and cyl_zoff as the tests above spell them are what the handle reports (snk_params_derived gives float64 of the
    URDF constant; the kernels hold its float32)."""
    st = pkg.Stepper(1)
    p = model_params(st)
    st.close()
    assert p["dt"] == float(np.float32(1.0 / 240.0)) and abs(p["cyl_zoff"] - 0.0183) < 1e-9


# ----------------------------------------------------------------------------------------------------------------------
# 2. obstacle 2: the free box's four slots
# ----------------------------------------------------------------------------------------------------------------------
def test_free_box_slots_match_the_independent_model(pkg):
    torch = pytest.importorskip("torch")
    n = 16
    rng = np.random.default_rng(1602)
    S = np.stack([random_state(rng, n, z=0.3, qamp=1.5, vamp=1.0) for _ in range(E)]).astype(np.float32)
    M = synthetic_cache(rng, n, E)
    bs, bm = synthetic_box(rng, E)
    st = pkg.Stepper(E, n_modules=n, obstacle=2)
    assert st.contact_slots == 8 * n + 4
    st.set_state(S, None)
    st.set_manifold(M)
    st.set_box(bs, bm)
    params = model_params(st)
    host = st.contacts()
    dev = read_on_device(torch, st, None, E, 8 * n + 4)
    st.close()
    assert same_bits(host[0], dev[0][:E]) and same_bits(host[1], dev[1][:E]) and np.array_equal(host[2], dev[2][:E])
    assert np.all(dev[0][E] == -7.0) and np.all(dev[1][E] == -7.0) and dev[2][E] == -77
    check_against_the_model("n=16 + box", (dev[0][:E], dev[1][:E], dev[2][:E]), S, M, (bs, bm), params)
    box_rows = dev[0][:E, 8 * n:]
    assert np.all(box_rows[box_rows[:, :, 14] == 1.0][:, 12] == 2 * n)
    assert np.array_equal((box_rows[:, :, 14] == 1.0).sum(axis=1), bm[:, 0].astype(int))
    assert dev[1][1, 2 * n] > 0 and dev[1][0, 2 * n] == 0


# ----------------------------------------------------------------------------------------------------------------------
# 3. behind real physics, on one stream
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,streamed", [(16, False), (16, True), (32, False)])
def test_contacts_behind_a_substep_on_one_stream(pkg, monkeypatch, n, streamed):
    """snk_substep, then snk_contacts on the same stream with no synchronisation between: bit for bit the contacts of a
    second handle loaded with the downloaded post-substep state and cache."""
    torch = pytest.importorskip("torch")
    if streamed:
        monkeypatch.setenv("SNK_FORCE_STREAMED", "1")
    else:
        monkeypatch.delenv("SNK_FORCE_STREAMED", raising=False)
    B, A = 6, n // 2
    a, b = pkg.Stepper(B, n_modules=n), pkg.Stepper(B, n_modules=n)
    a.reset()
    for j in range(2):
        a.step(gait(range(B), j, A) * 0.9)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    tg = np.zeros((B, n), np.float32)
    tg[:, 1::2] = gait(range(B), 2, A) * np.float32(np.pi / 6)
    t_tg = torch.tensor(tg, device=dev)
    slots = a.contact_slots
    pts = torch.zeros((B, slots, 16), dtype=torch.float32, device=dev)
    frc = torch.zeros((B, 2 * n + 1), dtype=torch.float32, device=dev)
    cnt = torch.zeros((B,), dtype=torch.int32, device=dev)
    a.substep_device(t_tg.data_ptr(), 3, 0, 0, stream)
    a.contacts_device(0, B, pts.data_ptr(), frc.data_ptr(), cnt.data_ptr(), stream)
    torch.cuda.synchronize()
    snap = a.snapshot()
    b.restore(snap)
    want = b.contacts()
    assert same_bits(pts.cpu().numpy(), want[0]) and same_bits(frc.cpu().numpy(), want[1])
    assert np.array_equal(cnt.cpu().numpy(), want[2])
    # and it is the cache that was read: count = the cache's counts, impulses = the cache's, forces not all zero
    assert np.array_equal(want[2], snap.manifold[:, :, 0].sum(axis=1).astype(np.int32)) and want[2].min() > 0
    lam = snap.manifold[:, :, 1:].reshape(B, 2 * n, 4, 7)[..., 6].reshape(B, 8 * n)
    assert same_bits(want[0][:, :, 11], lam) and want[1].max() > 0
    a.close()
    b.close()


# ----------------------------------------------------------------------------------------------------------------------
# 4. physics: the project's own rest invariant (tests/test_oracle_physics.py: test_rest_on_plane_supports_weight)
# ----------------------------------------------------------------------------------------------------------------------
def test_resting_snake_and_box_put_their_weight_on_the_contacts(pkg):
    st = pkg.Stepper(1)
    st.reset()
    zero = np.zeros((1, 16), np.float32)
    st.substep(zero, 420)
    totals = []
    for k in range(420, 480):
        st.substep(zero, 1)
        pts, force, count = st.contacts()
        totals.append(float(force.astype(np.float64).sum()))
    st.close()
    totals = np.array(totals)
    print("  resting snake: force.sum() mean %.3f N, worst deviation %.3f N (weight %.3f N), %d live slots"
          % (totals.mean(), np.abs(totals - 21.296 * 9.8).max(), 21.296 * 9.8, count[0]))
    assert abs(totals.mean() - 21.296 * 9.8) < 0.5
    assert np.abs(totals - 21.296 * 9.8).max() < 2.0
    assert force[0, 32] == 0.0
    # the free box two metres away, at rest on its four corners (tests/test_obstacle.py: 0.5 N after 240 substeps)
    st = pkg.Stepper(1, obstacle=2, obstacle_pos=[2.0, 0.0, 0.1])
    st.reset()
    st.substep(zero, 240)
    pts, force, count = st.contacts()
    st.close()
    print("  resting box: %.3f N on %d points (weight %.1f N)" % (force[0, 32], int(pts[0, 128:, 14].sum()), 200 * 9.8))
    assert pts[0, 128:, 14].sum() == 4 and abs(float(force[0, 32]) - 200.0 * 9.8) < 0.5


# ----------------------------------------------------------------------------------------------------------------------
# 5. the rules of the seam
# ----------------------------------------------------------------------------------------------------------------------
def test_env_ids_canaries_and_null_outputs_on_the_device(pkg):
    torch = pytest.importorskip("torch")
    n, B = 16, 5
    st = pkg.Stepper(B, n_modules=n)
    st.reset()
    for j in range(3):
        st.step(gait(range(B), j) * 0.9)
    before = st.snapshot()
    full = st.contacts()
    assert full[2].min() > 0
    assert all(same_bits(x, y[[3, 0, 3]]) if x.dtype == np.float32 else np.array_equal(x, y[[3, 0, 3]])
               for x, y in zip(st.contacts([3, 0, 3]), full))
    ids = [4, 1, 1, B, 0, -1, 2]
    dev = read_on_device(torch, st, ids, len(ids), 8 * n)
    for k, e in enumerate(ids):
        known = 0 <= e < B
        for got, want in zip(dev, full):
            w = want[e] if known else np.zeros_like(want[0])
            assert (same_bits(got[k], w) if w.dtype == np.float32 else got[k] == w), (k, e)
    assert np.all(dev[0][len(ids)] == -7.0) and np.all(dev[1][len(ids)] == -7.0) and dev[2][len(ids)] == -77
    # each combination of NULL outputs: what is asked for is written, the same bits as with all three
    d = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    for want_p, want_f, want_c in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        p = torch.full((B + 1, 8 * n, 16), -7.0, dtype=torch.float32, device=d)
        f = torch.full((B + 1, 2 * n + 1), -7.0, dtype=torch.float32, device=d)
        c = torch.full((B + 1,), -77, dtype=torch.int32, device=d)
        st.contacts_device(0, B, p.data_ptr() if want_p else 0, f.data_ptr() if want_f else 0,
                           c.data_ptr() if want_c else 0, stream)
        torch.cuda.synchronize()
        p, f, c = p.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy()
        assert same_bits(p[:B], full[0]) if want_p else np.all(p == -7.0)
        assert same_bits(f[:B], full[1]) if want_f else np.all(f == -7.0)
        assert np.array_equal(c[:B], full[2]) if want_c else np.all(c == -77)
        assert np.all(p[B] == -7.0) and np.all(f[B] == -7.0) and c[B] == -77
    # through DeviceWorld: tensors on the world's stream, into a caller's tensors, and the forces alone
    world = pkg.DeviceWorld(stepper=st)
    wp, wf, wc = world.contacts([2, 2, 0])
    out = tuple(torch.empty_like(x) for x in world.contacts())
    assert all(x is y for x, y in zip(world.contacts(out=out), out))
    cf = world.contact_forces()
    torch.cuda.synchronize()
    assert same_bits(wp.cpu().numpy(), full[0][[2, 2, 0]]) and same_bits(wf.cpu().numpy(), full[1][[2, 2, 0]])
    assert np.array_equal(wc.cpu().numpy(), full[2][[2, 2, 0]]) and wc.dtype == torch.int32
    assert same_bits(out[0].cpu().numpy(), full[0]) and same_bits(cf.cpu().numpy(), full[1]) and tuple(cf.shape) == (B, 2 * n + 1)
    with pytest.raises(ValueError, match="shape"):
        world.contacts(out=(torch.empty((B, 8 * n, 15), dtype=torch.float32, device=d), None, None))
    # nothing of the handle's state was written
    assert snap_equal(st.snapshot(), before, slice(None), slice(None), STATE_FIELDS + ("reset_pose",)) == []
    st.close()
    # the free box's record stays too
    st = pkg.Stepper(3, obstacle=2)
    st.reset()
    st.substep(np.zeros((3, 16), np.float32), 20)
    before = st.snapshot()
    assert st.contacts()[0].shape == (3, 8 * n + 4, 16)
    assert snap_equal(st.snapshot(), before, slice(None), slice(None), STATE_FIELDS) == [] and before.box_manifold[:, 0].min() > 0
    st.close()


def test_contact_calls_refuse_what_the_header_says(pkg):
    torch = pytest.importorskip("torch")
    n, B = 16, 4
    st = pkg.Stepper(B)
    d = torch.device("cuda", 0)
    p = torch.zeros((B, 8 * n, 16), dtype=torch.float32, device=d)
    f = torch.zeros((B, 2 * n + 1), dtype=torch.float32, device=d)
    c = torch.zeros((B,), dtype=torch.int32, device=d)
    with pytest.raises(RuntimeError, match="snk_contacts: points_dev, force_dev and count_dev are all null"):
        st.contacts_device(0, B)
    with pytest.raises(RuntimeError, match="snk_contacts: points_dev must be 16-byte aligned"):
        st.contacts_device(0, 1, p.data_ptr() + 4)
    with pytest.raises(RuntimeError, match="snk_contacts: n_rows must be at least 1"):
        st.contacts_device(0, 0, p.data_ptr())
    # the host form refuses by index what the device form cannot
    with pytest.raises(RuntimeError, match=r"snk_contacts_host: env_ids\[1\] = 4 is outside 0 \.\. 3"):
        st.contacts([0, B])
    with pytest.raises(RuntimeError, match=r"snk_contacts_host: env_ids\[0\] = -1 is outside 0 \.\. 3"):
        st.contacts([-1])
    import ctypes as C
    buf = np.zeros((B + 1, 8 * n, 16), np.float32)
    rc = st.lib.snk_contacts_host(st.h, None, B + 1, buf.ctypes.data_as(C.POINTER(C.c_float)), None, None)
    assert rc != 0 and "n_rows 5 without env_ids is more than the handle's 4 envs" in pkg._lib.last_error()
    assert st.lib.snk_contacts_host(st.h, None, B, None, None, None) != 0
    assert "snk_contacts_host: points, force and count are all null" in pkg._lib.last_error()
    # a contact_model 0 handle has no cache: no slots, and the calls refuse
    from conftest import ROUND1
    old = pkg.Stepper(2, **ROUND1)
    assert old.lib.snk_contact_slots(old.h) == 0 and "contact_model 0" in pkg._lib.last_error()
    with pytest.raises(RuntimeError, match="snk_contacts: this handle has contact_model 0"):
        old.contacts_device(0, 2, p.data_ptr())
    with pytest.raises(RuntimeError, match="contact_model 0"):
        old.contacts()
    old.close()
    # alive: every call goes through; poisoned: every one refuses, the slot count answers 0
    calls = (lambda: st.contacts_device(0, B, p.data_ptr(), f.data_ptr(), c.data_ptr()),
             lambda: st.contacts(),
             lambda: st.contacts([1]))
    for fn in calls:
        fn()
    torch.cuda.synchronize()
    assert st.contact_slots == 8 * n
    st.debug_raise_alarm()
    for fn in calls:
        with pytest.raises(RuntimeError, match="env-step scheduler: a bounded wait ran out"):
            fn()
    assert st.lib.snk_contact_slots(st.h) == 0 and "a bounded wait ran out" in pkg._lib.last_error()
    assert np.array_equal(st.contact_links(), pkg._lib.contact_links(n))      # (host arithmetic: still answers)
    st.close()


# ----------------------------------------------------------------------------------------------------------------------
# 6. BulletClient.getContactPoints on the kernels
# ----------------------------------------------------------------------------------------------------------------------
def test_client_contact_points_are_the_handles_slot_table(pkg):
    from test_pybullet_client import SeamLogic
    p = pkg.BulletClient()
    logic = SeamLogic(p, f32_targets=True)
    for vec_mode in (True, False):
        for j in range(3):
            logic.env_step((gait([3], j)[0] * np.float32(0.9)).astype(np.float32), vec_mode)
    st = p._stepper()
    pts = st.contacts()[0][0]
    links = st.contact_links()
    live = [r for r in pts if r[14] == 1.0]
    cps = p.getContactPoints(logic.body, 0)
    assert len(cps) == len(live) > 0
    for t, r in zip(cps, live):
        assert t[:5] == (0, logic.body, 0, int(links[int(r[12])]), -1)
        assert t[5] == tuple(float(v) for v in r[0:3]) and t[6] == tuple(float(v) for v in r[3:6])
        assert t[7] == (0.0, 0.0, 1.0) and t[8] == float(r[9]) and t[9] == float(r[10])
        assert t[10:] == (0.0, (0.0, 0.0, 0.0), 0.0, (0.0, 0.0, 0.0))
    assert p.getContactPoints(0, logic.body) == cps
    one = cps[len(cps) // 2][3]
    assert p.getContactPoints(logic.body, 0, linkIndexA=one) == [t for t in cps if t[3] == one]
    with pytest.raises(NotImplementedError):
        p.getContactPoints(logic.body, logic.body)
    with pytest.raises(NotImplementedError):
        p.getContactPoints(logic.body)
    p.close()
