"""The free box (obstacle 2) on the HIP kernels against tests/np_substep.py, the float64 numpy model written from the rules:
its free motion (gyroscopic term, k + k|.| damping, the clamp), its block of M^-1 J^T and the sign of its part of a link-box
row, its friction coefficients, its exponential-map integration, inertia_from_file 1, and a box light enough for the snake
to move.  tests/test_np_substep.py holds the float64 oracle to the same model on the same kinds of states.

One substep through set_state / set_manifold / set_box / substep(T, 1) from float32 inputs, as test_gpu_np_substep._run; the
model and both oracles run on the same float32-rounded inputs, the model on the contacts the float64 oracle solved.  Contact
and iteration counts equal the float64 oracle's on every state.  Gates: conftest.f32_gate with test_gpu_np_substep's factors
and floors (median 1.5 x / 1e-6, p90 2 x / 1e-5, worst 2 x capped at 5e-2), the yardstick the float32 oracle's distance to
the model, on the snake's velocities, the motor torques, the box's six velocities (|d| / (1 + |v|), like the snake's) and
the box's pose (position and quaternion, absolute) -- one test per case and quantity, and the exact assertions of a case in
an unmarked `structure` test beside them.  A pair beyond a gate that is no wrong rule is a STRICT xfail with its figure
(profiles/r18_box_gates.txt holds every case's GATE lines).

The states are chosen on the CPU when a set is built (box_states.select_for_float32): a candidate is kept only if the
float64 and float32 oracles solve the same contact list and every link-box distance is at least 1e-5 m from the pair's
breaking threshold; at most np_manifold.MAX_LEFT_OUT of the candidates looked at may be left out.  On the GPU no state is
then excused.
"""
import zlib

import numpy as np
import pytest

import box_states as bs
import np_manifold as nm
import np_substep as ns
from conftest import f32_gate
from test_gpu_np_substep import _open, _rel

pytestmark = pytest.mark.gpu

B = 16
_sets = {}


def the_set(oracle_mod, kind, over, mu, motion):
    """16 selected states of (kind of states, parameters, plane friction, box motion): a function of those alone."""
    key = (kind, tuple(sorted(over.items())), mu, motion)
    if key in _sets:
        return _sets[key]
    full = dict(bs.FREE_BOX, residual_threshold=0.0, **over)
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    if kind == "gait":
        S, T, M, BS, BM = bs.gait_box(oracle_mod, 16, B + 1, full)
    else:
        # "apart": no link-box contact in any state (the box 5 mm beyond every link's reach)
        S, T, M, BS, BM = bs.beside_link(oracle_mod, np.random.default_rng(2301), B + 1, full,
                                         touching=0.0 if kind == "apart" else 0.75)
    BS = dict(found=lambda: BS, twisted=lambda: bs.twisted(rng, BS), clamp=lambda: bs.at_the_clamp(rng, BS))[motion]()
    keep, seen = bs.select_for_float32(oracle_mod, full, S, T, M, BS, BM, 1.0 if mu is None else mu, want=B)
    assert len(keep) == B and seen - B <= nm.MAX_LEFT_OUT * seen, (kind, over, mu, motion, len(keep), seen)
    pick = lambda a: None if a is None else np.asarray(a)[keep]      # noqa: E731
    _sets[key] = (full, pick(S), pick(T), pick(M), pick(BS), pick(BM))
    return _sets[key]


def _box_rel(x, ref):
    return (np.abs(x[7:13] - ref[7:13]) / (1 + np.abs(ref[7:13]))).max()


QUANTITIES = ("velocity", "motor torque", "box velocity", "box pose")
_runs = {}


def run(pkg, oracle_mod, name):
    """GPU, float64 oracle (contacts, counts) and float32 oracle from the same float32 inputs, once per case; per env the
    errors of the GPU and of the float32 oracle against the numpy model.  Returns ({quantity: (GPU, float32 oracle)}, the
    float64 oracle's contact lists)."""
    if name in _runs:
        return _runs[name]
    kind, over, mu, motion = CASES[name]
    full, S, T, M, BS, BM = the_set(oracle_mod, kind, dict(over), mu, motion)
    f32 = lambda a: None if a is None else np.asarray(a, np.float32)      # noqa: E731
    S32, T32, M32, BS32, BM32 = map(f32, (S, T, M, BS, BM))
    st = pkg.Stepper(B, n_modules=16, **full)
    if mu is not None:
        st.set_ground_friction(np.full(B, mu, np.float32))
    st.set_state(S32)
    if M32 is not None:
        st.set_manifold(M32)
    st.set_box(BS32, BM32)
    info = st.substep(T32, 1)
    G, GX = st.get_state()
    GB = st.get_box()[0].astype(np.float64)
    st.close()
    o = oracle_mod.OracleEnv(n_modules=16, **bs.MIRROR, **full)
    o32 = oracle_mod.OracleEnv(n_modules=16, f32=True, **bs.MIRROR, **full)
    mup = 1.0 if mu is None else float(np.float32(mu))
    E = {k: ([], []) for k in QUANTITIES}
    lists = []
    for i in range(B):
        d = lambda a: None if a is None else a[i].astype(np.float64)      # noqa: E731
        s64, t64, m64, box = d(S32), d(T32), d(M32), (d(BS32), d(BM32))
        for e in (o, o32):
            bs.run_oracle(e, s64, t64, m64, box, mup)
        C = o.last_contacts_full()
        lists.append(C)
        assert info[i, 1] == o.last_num_contacts == len(C), (name, i, info[i], len(C))
        assert info[i, 0] == o.last_iterations, (name, i, info[i], o.last_iterations)
        lam0 = None
        if full.get("warm_start"):
            lam0 = bs.start_impulses(o.params, s64, m64, box, C)
        r = ns.substep(o.params, s64, t64, C, mu_plane=mup, lam0=lam0, box=box[0])
        sc = max(1.0, np.abs(r["tau_motor"]).max())
        b32 = o32.get_box()[0]
        for k, g, f in (("velocity", _rel(G[i].astype(np.float64), r["state"], 16), _rel(o32.get_state(), r["state"], 16)),
                        ("motor torque", np.abs(GX[i, :16] - r["tau_motor"]).max() / sc,
                         np.abs(o32.get_aux()[0] - r["tau_motor"]).max() / sc),
                        ("box velocity", _box_rel(GB[i], r["box"]), _box_rel(b32, r["box"])),
                        ("box pose", np.abs(GB[i, :7] - r["box"][:7]).max(), np.abs(b32[:7] - r["box"][:7]).max())):
            E[k][0].append(g)
            E[k][1].append(f)
    print("  [%s] %d envs, %d contacts (%d link-box in %d envs, %d box-ground), iterations %s"
          % (name, B, sum(map(len, lists)), sum(int((C[:, 5] == -2).sum()) for C in lists), with_link_box(lists),
             sum(int((C[:, 4] < 0).sum()) for C in lists), sorted(set(int(x) for x in info[:, 0]))))
    E = {k: (np.array(g), np.array(f)) for k, (g, f) in E.items()}
    for k, (g, f) in E.items():
        assert np.isfinite(g).all(), (name, k)
        print("  DIAG np box %s: %s per state, GPU %s | float32 oracle %s"
              % (name, k, " ".join("%.1e" % x for x in g), " ".join("%.1e" % x for x in f)))
    _runs[name] = (E, lists)
    return _runs[name]


def with_link_box(lists):
    return sum(bool((C[:, 5] == -2).any()) for C in lists)


# case: (kind of states, parameters, plane friction, box motion)
CASES = {
    # the box as placed, at rest beside a link: what moves it is the link pushing and its own weight on one corner
    "default": ("beside", {}, None, "found"),
    # |omega| up to 5, |v| up to 2 added: the gyroscopic term, the damping, a sliding ground contact, link-box rows with the
    # box's velocity in their right-hand sides
    "twisted box": ("beside", {}, None, "twisted"),
    # 0.5 kg: the box's block of M^-1 J^T dominates a link-box row
    "light box": ("beside", dict(obstacle_mass=0.5), None, "twisted"),
    # the box's inertia is (1, 100, 1)
    "inertia_from_file 1": ("beside", dict(inertia_from_file=1), None, "twisted"),
    # The box-ground coefficient is min(mu_obstacle x mu_plane, 10) = 3: combined, then clamped.  Clamped first, as the
    # kernels had it (the snake's min(mu_link x mu_plane, 10) / mu_link x mu_obstacle = 2.5), the sliding box loses a
    # different 2e-3 m/s in this substep: velocity median 3.9e-4 against the float32 oracle's 2.4e-5 (16 x) before the fix.
    "plane friction 6": ("beside", {}, 6.0, "twisted"),
    # Plane friction 0 on states WITHOUT link-box contacts ("apart"): at mu_ground 0 the kernels' pair friction vanishes with
    # the ground's (test_gpu_rows.test_link_link_friction_without_ground_friction, an open rule of its own), which a link-box
    # contact would meet here; the box's own ground contacts have a zero cone under the rule and in the kernels alike.
    "plane friction 0": ("apart", {}, 0.0, "twisted"),
    # every box velocity component at +-99.5 ... 100: the clamp on v + a dt and on v_free + dv, the angular motion limit
    "velocity clamp": ("beside", {}, None, "clamp"),
    "cone_friction 0": ("beside", dict(cone_friction=0), None, "twisted"),
    # gait states run under warm_start 1, handed over with the snake's caches and the box's: its ground contacts start at
    # their cached points' impulses
    "warm start": ("gait", dict(warm_start=1), None, "found"),
}

# The (case, quantity) pairs that miss a gate, with the figure that misses it by most.  None is a wrong rule -- what one looks
# like is in CASES: it moves the MEDIAN by 16 x.  These are tails of 16 states (a p90 of 16 is the second largest value) and
# medians at 1.5 ... 2.0 x: the worst states are the ones where the float32 oracle is furthest from the model too (per-state
# DIAG lines), and the model's own velocity spread under one-float32-ulp input noise on them is given with each.
OPEN = {
    ("default", "velocity"): "worst 2.8e-01 against the float32 oracle's 8.3e-02 (3.3 x), state 0, where the oracle is at its "
                             "worst too; the model's own spread there 1e-4, at worst 4.6e-4; median 1.07 x",
    ("light box", "velocity"): "p90 1.4e-03 against 4.5e-04 (3.0 x): states 0 and 7, float32 oracle 1.3e-3 / 4.5e-4, the "
                               "model's spread on state 7 1.1e-3; median 0.59 x",
    ("inertia_from_file 1", "motor torque"): "median 1.135e-06 against 7.39e-07 (1.54 x), limit 1.109e-06",
    ("plane friction 6", "velocity"): "median 4.0e-05 against 2.4e-05 (1.65 x); worst state 21 against the oracle's 15, the "
                                      "model's own spread there 0.88",
    ("plane friction 6", "motor torque"): "median 5.6e-06 against 3.3e-06 (1.68 x)",
    ("plane friction 6", "box velocity"): "worst 7.8e-02 against 3.0e-02 (2.6 x), state 9: the snake's velocities there are 21 "
                                          "/ 15 from the model, whose own spread is 0.88 (box: 4.1e-3); median 0.51 x",
    ("velocity clamp", "motor torque"): "median 5.2e-06 against 2.9e-06 (1.83 x)",
    ("velocity clamp", "box velocity"): "p90 2.4e-05 against 9.7e-06 (2.5 x): the second largest of 16, 3.8e-5 against 1.4e-5; "
                                        "worst 9.8e-4 against the oracle's 5.3e-2",
    ("cone_friction 0", "velocity"): "worst 1.9 against 0.15 (12.6 x), state 7, the model's own spread there 7.8e-2; the "
                                     "streamed-row solve's open cone_friction 0 finding (test_gpu_np_substep: 41 x over 128 states)",
    ("cone_friction 0", "motor torque"): "p90 2.8e-04 against 3.5e-05 (7.9 x), the same two states",
    ("warm start", "motor torque"): "median 7.8e-06 against 3.8e-06 (2.04 x)",
}


@pytest.mark.parametrize("name", list(CASES))
def test_box_structure(pkg, oracle_mod, name):
    """The exact part of a case alone, so that an xfail cannot hide it: contact and iteration counts equal to the float64
    oracle's on every state, finite outputs; and the contacts the case is about are there -- a link-box contact in at least
    half of the states (none at plane friction 0, above), the box's own ground contacts in every state."""
    _, lists = run(pkg, oracle_mod, name)
    if CASES[name][0] == "apart":
        assert with_link_box(lists) == 0
    else:
        assert with_link_box(lists) >= B // 2
    assert all((C[:, 4] < 0).any() for C in lists)


@pytest.mark.parametrize("name,what", [pytest.param(c, q, marks=[_open(OPEN[(c, q)])] if (c, q) in OPEN else [])
                                       for c in CASES for q in QUANTITIES])
def test_box_gates(pkg, oracle_mod, name, what):
    g, f = run(pkg, oracle_mod, name)[0][what]
    ok = f32_gate("np box %s: %s median of %d" % (name, what, B), np.median(g), np.median(f), 1.5, 1e-6)
    ok &= f32_gate("np box %s: %s p90" % (name, what), np.percentile(g, 90), np.percentile(f, 90), 2.0, 1e-5)
    ok &= f32_gate("np box %s: %s worst" % (name, what), g.max(), f.max(), 2.0, 5e-2)
    assert ok
