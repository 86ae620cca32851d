"""The dynamics queries on the GPU (include/snk.h, "The dynamics queries": snk_dynamics, snk_jacobians; csrc/snk_dyn.hpp):
mass matrix, bias forces and link Jacobians against the independent float64 model of tests/np_dynamics.py (validated on
the CPU by tests/test_np_dynamics.py), gated by its float32 twin; the exact properties the contract states; ids and bytes;
the refusals of both forms; a block taking a second row; and that nothing of the handle's state is written."""
import contextlib
import os

import numpy as np
import pytest

import np_dynamics as nd_
import np_model as npm
from conftest import f32_gate
from np_link_states import split_state

pytestmark = pytest.mark.gpu

# variant -> (n_modules, SNK_FORCE_STREAMED): Lds<16, true>, Lds<16, false>, Lds<32, false> (snk_seam.hpp: for_variant)
VARIANTS = {"16": (16, False), "16s": (16, True), "32": (32, False)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@contextlib.contextmanager
def stepper(pkg, n_envs, n, streamed=False, **over):
    """A handle; `streamed`: created under SNK_FORCE_STREAMED=1 (read at snk_create), the variable put back after."""
    old = os.environ.get("SNK_FORCE_STREAMED")
    if streamed:
        os.environ["SNK_FORCE_STREAMED"] = "1"
    else:
        os.environ.pop("SNK_FORCE_STREAMED", None)
    try:
        st = pkg.Stepper(n_envs, n_modules=n, **over)
    finally:
        if old is None:
            os.environ.pop("SNK_FORCE_STREAMED", None)
        else:
            os.environ["SNK_FORCE_STREAMED"] = old
    try:
        yield st
    finally:
        st.close()


def link_body(r):
    """the composite body of link row r: rows 0 .. 3 are body 0, rows 3b + 1 .. 3b + 3 body b"""
    return 0 if r <= 3 else (r - 1) // 3


@pytest.fixture(scope="module")
def cases(pkg):
    """Per kernel variant: the gate's 24 states on a handle and everything the GPU says of them, all rows in one call
    each -- M and h (flags 3), h alone (flags 1, 2), J of the gate's points, the link states -- computed once."""
    out = {}
    for v, (n, streamed) in VARIANTS.items():
        ref = nd_.references(n)
        S = ref["S"]
        rows, local = nd_.points_arrays(ref["points"])
        with stepper(pkg, len(S), n, streamed) as st:
            st.set_state(S, None)
            assert st.dyn_dofs == n + 6
            M, h3 = st.dynamics()
            H = {1: st.dynamics(flags=1, mass=False)[1], 2: st.dynamics(flags=2, mass=False)[1], 3: h3}
            J = st.jacobians(rows, local)
            Jcom = st.jacobians(rows)
            ls = st.link_states()
            S2, _ = st.get_state()
        assert same_bits(S2, S)
        out[v] = dict(n=n, S=S, M=M, H=H, J=J, Jcom=Jcom, ls=ls, rows=rows, ref=ref)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# 1. accuracy
# ----------------------------------------------------------------------------------------------------------------------
# Floors: the float32 twin's own worst figures on these states (tests/test_np_dynamics.py,
# test_twin_is_ten_times_inside_the_caps_on_the_gate_states prints them): M 2.43e-6 normalised (32 links, joint block); h
# 5.2e-7 of its block's largest component (32 links, flags 2, joints: 1.144e-4 of 219); J 4.7e-7 (32 links).  Below them a
# figure is the round-off of float32 arithmetic over this tree, whoever does it.
FLOOR_M, FLOOR_H_REL, FLOOR_J = 2.5e-6, 5.5e-7, 5e-7


def gate_factor(n):
    """the project's factor (conftest.f32_gate): worst values over >= 30 samples of the 16-link chain 1.5, the 32-link
    chain 2.0 -- every figure here is a worst over 24 states times hundreds of entries"""
    return 1.5 if n == 16 else 2.0


@pytest.mark.parametrize("n", [16, 32])
def test_dynamics_match_the_independent_model(cases, n):
    """M per entry normalised by sqrt(M_ii M_jj) over the base block, the base-joint block and the joint block; h per block
    (base moment, base force, joints) for flags 1, 2 and 3; J of the 2n cylinder links' COMs and of a point 0.05 m off the
    head's COM, linear and angular rows: each the worst over 24 states against float64, gated by the float32 twin's figure on
    the same states.  Hard caps: 1e-4 for M, 1e-3 of the block's largest component for h and J.  The GATE lines of a run
    are profiles/r22_dynamics_accuracy.txt."""
    c = cases[str(n)]
    ref, tw = c["ref"], c["ref"]["twin"]
    assert c["M"].shape == (24, n + 6, n + 6) and c["J"].shape == (24, 2 * n + 1, 6, n + 6)
    assert all(np.all(np.isfinite(a)) for a in (c["M"], c["J"], c["H"][1], c["H"][2], c["H"][3]))
    got = nd_.figures(n, c["S"], c["M"], c["H"], c["J"], ref)
    twf = nd_.figures(n, c["S"], tw["M"], tw["H"], tw["J"], ref)
    ok = True
    for k in sorted(got):
        err, big = got[k]
        if big is None:
            floor, cap = FLOOR_M, 1e-4
        elif k.startswith("J"):
            floor, cap = FLOOR_J, 1e-3 * big
        else:
            floor, cap = FLOOR_H_REL * big, 1e-3 * big
        ok &= f32_gate("dynamics n=%d: %s (worst of 24 states)" % (n, k), err, twf[k][0], factor=gate_factor(n), floor=floor, cap=cap)
    assert ok


# ----------------------------------------------------------------------------------------------------------------------
# 2. exact properties
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_exact_properties(cases, variant):
    """M equals its transpose bit for bit; the columns of J for joints beyond the link's body are exact zeros, those of
    v the identity and zeros, those of omega the identity in the angular rows; J u at the COM is the link's twist of
    snk_link_states on the same handle; 1/2 u^T M u is np_model's kinetic energy.  flags 3 is computed in ONE pass and is
    not required to be the sum of flags 1 and 2 (include/snk.h says so): the distance is printed, the accuracy gate holds
    each of the three."""
    c = cases[variant]
    n, S, M, J, Jcom, rows = c["n"], c["S"], c["M"], c["J"], c["Jcom"], c["rows"]
    assert same_bits(M, np.ascontiguousarray(M.transpose(0, 2, 1)))
    assert np.all(np.diagonal(M, axis1=1, axis2=2) > 0)
    for p, r in enumerate(rows):
        b = link_body(int(r))
        for A in (J, Jcom):
            assert np.all(bits(A[:, p, :, 6 + b:]) == 0), (p, r)
            if b:      # the joints that do move it: unit axes in the angular rows
                assert np.max(np.abs(np.linalg.norm(A[:, p, 3:6, 6:6 + b].astype(np.float64), axis=1) - 1.0)) < 1e-5
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), J[:, :, 0:3, 3:6].shape)
    for A in (J, Jcom):
        assert same_bits(A[:, :, 0:3, 3:6], eye) and np.all(bits(A[:, :, 3:6, 3:6]) == 0)
        assert same_bits(A[:, :, 3:6, 0:3], eye)
    # the same points with and without a local list where the local point is the COM
    assert same_bits(J[:, :-1], Jcom[:, :-1]) and not same_bits(J[:, -1], Jcom[:, -1])
    worst_tw, worst_ke, worst_ke_twin = 0.0, 0.0, 0.0
    links = npm.build_tree(n)
    for e in range(len(S)):
        pos, quat, u, q = split_state(S[e].astype(np.float64), n)
        tw = c["ls"][e][rows].astype(np.float64)                       # [P, 16]: floats 10-12 v(COM), 13-15 omega
        Ju = Jcom[e].astype(np.float64) @ u                            # [P, 6]
        worst_tw = max(worst_tw, np.max(np.abs(Ju - tw[:, 10:16])) / np.max(np.abs(c["ls"][e][:, 10:16])))
        K = npm.momentum(links, pos, quat, q, u)[2]
        worst_ke = max(worst_ke, abs(0.5 * u @ M[e].astype(np.float64) @ u - K) / K)
        worst_ke_twin = max(worst_ke_twin, abs(0.5 * u @ c["ref"]["twin"]["M"][e].astype(np.float64) @ u - K) / K)
    print("  dynamics %s: J u against snk_link_states' twists: %.3e of the largest twist component" % (variant, worst_tw))
    assert worst_tw < 1e-5
    f32_gate("dynamics %s: kinetic energy 1/2 u^T M u (worst of 24 states)" % variant, worst_ke, worst_ke_twin,
             factor=gate_factor(n), floor=FLOOR_M, cap=1e-4)
    d = np.max(np.abs(c["H"][3].astype(np.float64) - (c["H"][1].astype(np.float64) + c["H"][2])))
    print("  dynamics %s: h(flags 3) against h(1) + h(2): %.3e (largest component %.3e)" % (variant, d, np.max(np.abs(c["H"][3]))))


def test_streamed_variant_gives_the_register_variants_bits(cases):
    """The 16-link kernels on the streamed-row LDS image (SNK_FORCE_STREAMED=1 at create) run the same arithmetic on the
    same record: the same bits."""
    a, b = cases["16"], cases["16s"]
    assert same_bits(a["M"], b["M"]) and same_bits(a["J"], b["J"]) and all(same_bits(a["H"][f], b["H"][f]) for f in (1, 2, 3))


# ----------------------------------------------------------------------------------------------------------------------
# 3. ids and bytes
# ----------------------------------------------------------------------------------------------------------------------
E = 5
IDS = [3, 0, 3, 7, 1]                  # a repeat, and 7: outside a 5-env handle


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_ids_and_bytes(pkg, variant):
    torch = pytest.importorskip("torch")
    n, streamed = VARIANTS[variant]
    nd = n + 6
    S = nd_.gate_states(n)[:E]
    pts = [(3 * n + 1, (0.03, -0.04, 0.0)), (2, None), (0, None), (3 * (n // 2), (0.0, 0.01, 0.0))]
    rows, local = nd_.points_arrays(pts)
    P = len(rows)
    with stepper(pkg, E, n, streamed) as st:
        st.set_state(S, None)
        world = pkg.DeviceWorld(stepper=st)
        dev, stream = world.device, torch.cuda.current_stream().cuda_stream
        Mf, hf = st.dynamics()
        Jf = st.jacobians(rows, local)
        assert np.all(Mf[:, 0, 0] > 0) and np.all(np.abs(Jf).max(axis=(1, 2, 3)) > 0)
        # the host form with ids that repeat
        Mh, hh = st.dynamics([3, 0, 3])
        assert same_bits(Mh, Mf[[3, 0, 3]]) and same_bits(hh, hf[[3, 0, 3]]) and same_bits(st.jacobians(rows, local, [3, 0, 3]), Jf[[3, 0, 3]])
        # the device form: ids with a repeat and an unknown id, a row beyond n_rows pre-filled
        k = len(IDS)
        idt = torch.tensor(IDS, dtype=torch.int32, device=dev)
        Mb = torch.full((k + 1, nd, nd), -7.0, dtype=torch.float32, device=dev)
        hb = torch.full((k + 1, nd), -7.0, dtype=torch.float32, device=dev)
        Jb = torch.full((k + 1, P, 6, nd), -7.0, dtype=torch.float32, device=dev)
        rt, lt = torch.tensor(rows, device=dev), torch.tensor(local, device=dev)
        st.dynamics_device(idt.data_ptr(), k, 3, Mb.data_ptr(), hb.data_ptr(), stream)
        st.jacobians_device(idt.data_ptr(), k, rt.data_ptr(), lt.data_ptr(), P, Jb.data_ptr(), stream)
        Mw, hw = world.dynamics(IDS)
        Jw = world.jacobians(rows.tolist(), local.tolist(), IDS)
        torch.cuda.synchronize()
        Mb, hb, Jb, Mw, hw, Jw = (x.cpu().numpy() for x in (Mb, hb, Jb, Mw, hw, Jw))
        for i, e in enumerate(IDS):
            for got, got2, full in ((Mb, Mw, Mf), (hb, hw, hf), (Jb, Jw, Jf)):
                want = full[e] if 0 <= e < E else np.zeros_like(full[0])
                assert same_bits(got[i], want) and same_bits(got2[i], want), (i, e)
        assert np.all(Mb[k] == -7.0) and np.all(hb[k] == -7.0) and np.all(Jb[k] == -7.0)
        # without ids, into a caller's tensors; each output omitted in turn
        Mo = torch.empty((E, nd, nd), dtype=torch.float32, device=dev)
        ho = torch.empty((E, nd), dtype=torch.float32, device=dev)
        Jo = torch.empty((E, P, 6, nd), dtype=torch.float32, device=dev)
        r = world.dynamics(out=(Mo, ho))
        assert r[0] is Mo and r[1] is ho and world.jacobians(rt, lt, out=Jo) is Jo
        M1, h1 = world.mass_matrix(), world.bias_forces()
        hg, hv = world.bias_forces(velocity=False), world.bias_forces(gravity=False)
        M2 = torch.full((E, nd, nd), -7.0, dtype=torch.float32, device=dev)
        h2 = torch.full((E, nd), -7.0, dtype=torch.float32, device=dev)
        assert world.mass_matrix(out=M2) is M2 and world.bias_forces(out=h2) is h2
        torch.cuda.synchronize()
        for got, full in ((Mo, Mf), (ho, hf), (Jo, Jf), (M1, Mf), (h1, hf), (M2, Mf), (h2, hf)):
            assert same_bits(got.cpu().numpy(), full)
        assert same_bits(hg.cpu().numpy(), st.dynamics(flags=2, mass=False)[1])
        assert same_bits(hv.cpu().numpy(), st.dynamics(flags=1, mass=False)[1])
        assert st.dynamics(mass=False)[0] is None and st.dynamics(bias=False)[1] is None
        assert same_bits(st.dynamics(bias=False)[0], Mf)
        # the COMs without a local list
        assert same_bits(world.jacobians(rows[1:3]).cpu().numpy(), Jf[:, 1:3])
        # a link row outside the tree on the device path: a zero Jacobian, its neighbours untouched by it
        Jz = world.jacobians([-1, int(rows[0]), 3 * n + 2], [[0.0, 0.0, 0.0], list(local[0]), [0.0, 0.0, 0.0]]).cpu().numpy()
        assert np.all(bits(Jz[:, 0]) == 0) and np.all(bits(Jz[:, 2]) == 0) and same_bits(Jz[:, 1], Jf[:, 0])


# ----------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals_of_both_forms(pkg):
    torch = pytest.importorskip("torch")
    n, nd = 16, 22
    lib = pkg._lib
    with stepper(pkg, E, n) as st:
        world = pkg.DeviceWorld(stepper=st)
        dev = world.device
        M = torch.zeros((E, nd, nd), dtype=torch.float32, device=dev)
        h = torch.zeros((E, nd), dtype=torch.float32, device=dev)
        J = torch.zeros((E, 2, 6, nd), dtype=torch.float32, device=dev)
        rows = torch.tensor([1, 4], dtype=torch.int32, device=dev)
        loc = torch.zeros((2, 3), dtype=torch.float32, device=dev)
        dyn, jac = st.dynamics_device, st.jacobians_device
        for msg, f in (
                ("snk_dynamics: n_rows must be at least 1", lambda: dyn(0, 0, 3, M.data_ptr(), h.data_ptr())),
                ("snk_dynamics: flags must be SNK_BIAS_VELOCITY, SNK_BIAS_GRAVITY or both", lambda: dyn(0, E, 0, M.data_ptr(), h.data_ptr())),
                ("snk_dynamics: flags must be SNK_BIAS_VELOCITY, SNK_BIAS_GRAVITY or both", lambda: dyn(0, E, 4, M.data_ptr(), h.data_ptr())),
                ("snk_dynamics: mass and bias are both null", lambda: dyn(0, E, 3)),
                ("snk_dynamics: mass_dev must be 16-byte aligned", lambda: dyn(0, E, 3, M.data_ptr() + 4, h.data_ptr())),
                ("snk_jacobians: n_rows must be at least 1", lambda: jac(0, 0, rows.data_ptr(), 0, 2, J.data_ptr())),
                ("snk_jacobians: n_points 0 is outside 1 .. 256", lambda: jac(0, E, rows.data_ptr(), 0, 0, J.data_ptr())),
                ("snk_jacobians: n_points 257 is outside 1 .. 256", lambda: jac(0, E, rows.data_ptr(), 0, 257, J.data_ptr())),
                ("snk_jacobians: null link_rows", lambda: jac(0, E, 0, loc.data_ptr(), 2, J.data_ptr())),
                ("snk_jacobians: null jac", lambda: jac(0, E, rows.data_ptr(), loc.data_ptr(), 2, 0)),
                ("snk_jacobians: jac_dev must be 16-byte aligned", lambda: jac(0, E, rows.data_ptr(), loc.data_ptr(), 2, J.data_ptr() + 4)),
                ("snk_dynamics_host: n_rows must be at least 1", lambda: st.dynamics([])),
                ("snk_dynamics_host: flags must be SNK_BIAS_VELOCITY, SNK_BIAS_GRAVITY or both", lambda: st.dynamics(flags=0)),
                ("snk_dynamics_host: flags must be SNK_BIAS_VELOCITY, SNK_BIAS_GRAVITY or both", lambda: st.dynamics(flags=8)),
                ("snk_dynamics_host: mass and bias are both null", lambda: st.dynamics(mass=False, bias=False)),
                (r"snk_dynamics_host: env_ids\[1\] = 5 is outside 0 \.\. 4", lambda: st.dynamics([0, E])),
                (r"snk_dynamics_host: env_ids\[0\] = -1 is outside 0 \.\. 4", lambda: st.dynamics([-1])),
                (r"snk_jacobians_host: env_ids\[2\] = 9 is outside 0 \.\. 4", lambda: st.jacobians([1], None, [0, 1, 9])),
                ("snk_jacobians_host: n_rows must be at least 1", lambda: st.jacobians([1], None, [])),
                ("snk_jacobians_host: n_points 0 is outside 1 .. 256", lambda: st.jacobians([])),
                ("snk_jacobians_host: n_points 257 is outside 1 .. 256", lambda: st.jacobians([1] * 257)),
                (r"snk_jacobians_host: link_rows\[1\] = 50 is outside 0 \.\. 49", lambda: st.jacobians([0, 3 * n + 2])),
                (r"snk_jacobians_host: link_rows\[0\] = -1 is outside 0 \.\. 49", lambda: st.jacobians([-1])),
                (r"snk_jacobians_host: local\[1\]\[2\] is not finite", lambda: st.jacobians([1, 2], [[0, 0, 0], [0, 0, np.inf]])),
                (r"snk_jacobians_host: local\[0\]\[0\] is not finite", lambda: st.jacobians([1], [[np.nan, 0, 0]]))):
            with pytest.raises(RuntimeError, match=msg):
                f()
        # n_rows above n_envs without ids; null handles; null host outputs
        Mh, Jh = np.zeros((E + 1, nd, nd), np.float32), np.zeros((E + 1, 1, 6, nd), np.float32)
        one = np.array([1], np.int32)
        I32 = lib._I32
        for msg, rc in (
                ("snk_dynamics_host: n_rows 6 without env_ids is more than the handle's 5 envs",
                 lambda: st.lib.snk_dynamics_host(st.h, None, E + 1, 3, lib.fptr(Mh), None)),
                ("snk_jacobians_host: n_rows 6 without env_ids is more than the handle's 5 envs",
                 lambda: st.lib.snk_jacobians_host(st.h, None, E + 1, one.ctypes.data_as(I32), None, 1, lib.fptr(Jh))),
                ("snk_jacobians_host: null link_rows", lambda: st.lib.snk_jacobians_host(st.h, None, E, None, None, 1, lib.fptr(Jh))),
                ("snk_jacobians_host: null jac", lambda: st.lib.snk_jacobians_host(st.h, None, E, one.ctypes.data_as(I32), None, 1, None)),
                ("snk_dynamics: null handle", lambda: st.lib.snk_dynamics(None, None, E, 3, M.data_ptr(), None, None)),
                ("snk_dynamics_host: null handle", lambda: st.lib.snk_dynamics_host(None, None, E, 3, lib.fptr(Mh), None)),
                ("snk_jacobians: null handle", lambda: st.lib.snk_jacobians(None, None, E, rows.data_ptr(), None, 2, J.data_ptr(), None)),
                ("snk_jacobians_host: null handle",
                 lambda: st.lib.snk_jacobians_host(None, None, E, one.ctypes.data_as(I32), None, 1, lib.fptr(Jh)))):
            assert rc() != 0
            assert msg in lib.last_error(), (msg, lib.last_error())
        assert st.lib.snk_dyn_dofs(None) == 0 and "snk_dyn_dofs: null handle" in lib.last_error()
        # DeviceWorld: shape and dtype mistakes are ValueErrors
        with pytest.raises(ValueError, match="shape"):
            world.mass_matrix(out=torch.empty((E, nd, nd + 1), dtype=torch.float32, device=dev))
        with pytest.raises(ValueError, match="shape"):
            world.dynamics(out=(M, torch.empty((E, nd + 1), dtype=torch.float32, device=dev)))
        with pytest.raises(ValueError, match="must be torch.float32"):
            world.bias_forces(out=torch.empty((E, nd), dtype=torch.float64, device=dev))
        with pytest.raises(ValueError, match="shape"):
            world.jacobians([1, 4], out=torch.empty((E, 3, 6, nd), dtype=torch.float32, device=dev))
        with pytest.raises(ValueError, match="local must have shape"):
            world.jacobians([1, 4], [[0.0, 0.0, 0.0]])
        with pytest.raises(ValueError, match="local must be torch.float32"):
            world.jacobians([1, 4], torch.zeros((2, 3), dtype=torch.float64, device=dev))
        with pytest.raises(ValueError, match="1 .. 256 points"):
            world.jacobians([])
        with pytest.raises(ValueError, match="gravity, velocity or both"):
            world.bias_forces(gravity=False, velocity=False)
        # BulletClient is not extended
        assert not hasattr(pkg.BulletClient, "calculateMassMatrix") and not hasattr(pkg.BulletClient, "applyExternalForce")
        # a poisoned handle: all four calls and the dimension refuse with the scheduler's message; close() still works
        calls = (lambda: dyn(0, E, 3, M.data_ptr(), h.data_ptr()),
                 lambda: jac(0, E, rows.data_ptr(), loc.data_ptr(), 2, J.data_ptr()),
                 lambda: st.dynamics(),
                 lambda: st.jacobians([1, 4]),
                 lambda: st.dyn_dofs)
        for f in calls:
            f()                                              # alive: every one goes through
        torch.cuda.synchronize()
        st.debug_raise_alarm()
        for f in calls:
            with pytest.raises(RuntimeError, match="env-step scheduler: a bounded wait ran out"):
                f()
    assert st.h is None


# ----------------------------------------------------------------------------------------------------------------------
# 5. more rows than blocks
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_a_block_taking_a_second_row_gives_the_bits_of_the_first(pkg, variant):
    """The grid of a wave-per-row kernel is capped at 65536 blocks (snk_seam.hpp: grid_for); with 65536 + 3 rows, blocks 0
    to 2 take a second row, and the row loop's trailing barrier is all that keeps the next row's record load from the
    lanes still reading this row's.  The ids cycle over the five envs, so row r must be, bit for bit, row r - 5: checked
    on the device over every row.  The cheap outputs only: h, and a one-point Jacobian."""
    torch = pytest.importorskip("torch")
    n, streamed = VARIANTS[variant]
    nd = n + 6
    rows = 65536 + 3
    dev = torch.device("cuda", 0)
    ids = torch.as_tensor(np.arange(rows, dtype=np.int32) % E, device=dev)

    def cyclic(what, t):
        raw = t.reshape(rows, -1).view(torch.int32)
        assert bool(raw[:E].any()), (what, "the first rows hold nothing")
        assert torch.equal(raw[E:], raw[:-E]), (what, "a row differs from the earlier row of the same env")

    with stepper(pkg, E, n, streamed) as st:
        st.set_state(nd_.gate_states(n)[:E], None)
        h = torch.full((rows, nd), -7.0, dtype=torch.float32, device=dev)
        st.dynamics_device(ids.data_ptr(), rows, 3, 0, h.data_ptr())
        cyclic("snk_dynamics bias", h)
        J = torch.full((rows, 1, 6, nd), -7.0, dtype=torch.float32, device=dev)
        lr = torch.tensor([3 * n + 1], dtype=torch.int32, device=dev)
        loc = torch.tensor([[0.03, -0.04, 0.0]], dtype=torch.float32, device=dev)
        st.jacobians_device(ids.data_ptr(), rows, lr.data_ptr(), loc.data_ptr(), 1, J.data_ptr())
        cyclic("snk_jacobians", J)
        torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# 6. nothing of the state is written
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_state_is_not_written(pkg, variant):
    """A Snapshot of the handle before and after the calls -- after two env-steps, so that the contact cache holds
    something -- has every field bit-identical."""
    n, streamed = VARIANTS[variant]
    with stepper(pkg, E, n, streamed) as st:
        st.reset()
        k = np.arange(st.act_dim)
        for j in range(2):
            st.step((-0.9 * np.sin((2 * k[None, :] + 1) * 4.0 + 0.2 * j + 0.37 * np.arange(E)[:, None])).astype(np.float32))
        before = st.snapshot()
        world = pkg.DeviceWorld(stepper=st)
        st.dynamics()
        st.dynamics([4, 4, 0], flags=1)
        st.jacobians([0, 5, 3 * n + 1], [[0.0, 0.0, 0.0], [0.01, 0.0, 0.0], [0.0, 0.0, 0.05]])
        world.dynamics(IDS)
        world.jacobians([3 * n + 1], env_ids=IDS)
        world.torch.cuda.synchronize()
        after = st.snapshot()
        for f in before.FIELDS:
            a, b = getattr(before, f), getattr(after, f)
            assert (a is None) == (b is None), f
            if a is not None:
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f
