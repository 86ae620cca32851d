"""The streamed-row substep stage by stage: contact records, free motion, M^-1, the rows, the Gauss-Seidel
steps -- each against its own reference, on the 16-link streamed-row kernels (SNK_FORCE_STREAMED) and the 32-link chain.

After substep(T, 1) a workgroup's block of rows holds every record the solve read (Stepper.debug_rows; decoded by
tests/np_rows.py), and a handle with n_iterations 0 returns the free velocity untouched: pgs_v1's sweep loop is
`for (; it < n_iter; it++)` (snk_pgs_v1.hpp), and what follows it -- the motors' accumulated impulses written back (zero),
the returned delta-v (zero outside warm starting), substep_v1's steps (6) and (7) -- does not depend on a sweep having run;
the oracle's loop has the same form.

One error measure everywhere (test_np_rows.relerr): |gpu - ref|_inf / |ref|_inf per row or vector, collected over all rows
of a set; the gates are conftest.f32_gate's with the project's factors and floors (median 1.5 x / 1e-6, p90 2 x / 1e-5, worst
2 x with the p90's floor, 1e-5 -- a hundred float32 roundings, what the comparison of one row of single-precision numbers
cannot resolve -- and cap 5e-2) against the float32 oracle's figure for the same quantity on the same states (stage E: the float32
replay's).  Scalars that can be zero are measured against a floor that is written where it is used.  References are
computed from the same float32-rounded inputs; contact counts equal the float64 oracle's on every state.

Cases beyond a gate are STRICT xfails with the measured figure (profiles/r15_rows_stages.txt holds every case's GATE line).
"""
import numpy as np
import pytest

import np_rows as nr
import np_substep as ns
from box_states import FREE_BOX, gait_box
from conftest import f32_gate, random_state
from test_gpu_np_substep import PATHS, _ground, _open, _path
from test_gpu_np_sweeps import SCENARIOS, _scenario
from test_np_rows import BOX, MIRROR, folded32, model_dirs, relerr, static_box

pytestmark = pytest.mark.gpu

ROW_PATHS = [p[0] for p in PATHS if p[0] != "register-resident"]
G = nr.GEO_FIELDS


class Set:
    def __init__(self, n, S, T, over=None, mu=None, M=None, box=None):
        self.n, self.S, self.T, self.over, self.mu, self.M, self.box = n, S, T, dict(over or {}), mu, M, box
        self.over.setdefault("residual_threshold", 0.0)


_sets = {}


def the_set(oracle_mod, path, name):
    """The states of (path, set name): a function of the two alone."""
    key = (path, name)
    if key in _sets:
        return _sets[key]
    _, n, streamed = next(p for p in PATHS if p[0] == path)
    B = 16 if n == 16 else 8
    if name in SCENARIOS:
        S, T, over, mu, _ = _scenario(name, n, streamed)
        s = Set(n, S, T, over, mu)
    elif name == "in the air":
        rng = np.random.default_rng(2900 + n)
        s = Set(n, np.array([random_state(rng, n, z=1.0, qamp=0.8, vamp=3.0) for _ in range(B)]), rng.uniform(-0.5, 0.5, (B, n)))
    elif name == "folded":
        if n == 32:
            s = Set(n, *folded32(oracle_mod, 8))
        else:
            rng = np.random.default_rng(1500)
            e = oracle_mod.OracleEnv(**MIRROR)
            S = []
            while len(S) < B:
                x = _ground(rng, 16, 1, qamp=1.7)[0]
                e.set_state(x.astype(np.float32).astype(np.float64))
                C = e.contacts_full()
                if len(C) and (C[:, 5] >= 0).sum() >= 2:
                    S.append(x)
            s = Set(n, np.array(S), rng.uniform(-0.5, 0.5, (B, n)))
    elif name == "static box":
        if n == 16:
            S, T, M = static_box(oracle_mod, 8)
            s = Set(n, S, T, BOX, M=M)
        else:
            S, T, M, _, _ = gait_box(oracle_mod, n, 4, BOX)
            s = Set(n, S, T, BOX, M=M)
    elif name in ("free box", "free box, plane friction 6"):
        assert n == 16
        S, T, M, BS, BM = gait_box(oracle_mod, n, 8, FREE_BOX)
        s = Set(n, S, T, FREE_BOX, 6.0 if name.endswith("6") else None, M=M, box=(BS, BM))
    else:
        raise KeyError(name)
    _sets[key] = s
    return s


# ------------------------------------------------------------------------------------------------------------------
# one GPU substep with its block read out; the oracles and the model on the same float32-rounded inputs
# ------------------------------------------------------------------------------------------------------------------
_gpu = {}


def gpu_run(pkg, path, name, s, **extra):
    key = (path, name, tuple(sorted(extra.items())))
    if key in _gpu:
        return _gpu[key]
    B = len(s.S)
    st = pkg.Stepper(B, n_modules=s.n, **dict(s.over, **extra))
    if s.mu is not None:
        st.set_ground_friction(np.full(B, s.mu, np.float32))
    st.set_state(np.asarray(s.S, np.float32))
    if s.M is not None:
        st.set_manifold(np.asarray(s.M, np.float32))
    if s.box is not None:
        st.set_box(np.asarray(s.box[0], np.float32), np.asarray(s.box[1], np.float32))
    info = st.substep(np.asarray(s.T, np.float32), 1)
    blocks = st.debug_rows()
    state, aux = st.get_state()
    out = dict(info=info, blocks=blocks, state=state.astype(np.float64), aux=aux.astype(np.float64), manifold=st.get_manifold(),
               box=st.get_box()[0].astype(np.float64) if s.box is not None else None, layout=st.debug_rows_layout())
    st.close()
    _gpu[key] = out
    return out


def inputs64(s, i):
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)      # noqa: E731
    return (f(s.S[i]), f(s.T[i]), None if s.M is None else f(s.M[i]), None if s.box is None else (f(s.box[0][i]), f(s.box[1][i])),
            1.0 if s.mu is None else float(np.float32(s.mu)))


def oracle_run(e, s, i):
    s64, t64, M, box, mu = inputs64(s, i)
    e.hard_reset()
    e.set_plane_friction(mu)
    if M is not None:
        e.set_manifold(M)
    if box is not None:
        e.set_box(*box)
    e.set_state(s64)
    e.substep(t64)


def velocities(x, n):
    return np.concatenate([x[7:13], x[13 + n:]])


_refs = {}


def refs(oracle_mod, path, name, s, **extra):
    """Per state: the float64 and float32 oracles' contacts, rows and results under s.over + extra, the two oracles' free
    velocity (n_iterations 0) and M^-1, and the numpy model's rows, free velocity and mass matrix (None for the sets with
    the free box: their stages keep the float64 oracle as the reference; tests/test_gpu_np_box.py holds the kernels to the
    model's box)."""
    key = (path, name, tuple(sorted(extra.items())))
    if key in _refs:
        return _refs[key]
    n = s.n
    mk = lambda f32, **kw: oracle_mod.OracleEnv(n_modules=n, f32=f32, **MIRROR, **dict(s.over, **dict(extra, **kw)))   # noqa: E731
    o, o32, z, z32 = mk(False), mk(True), mk(False, n_iterations=0), mk(True, n_iterations=0)
    out = []
    for i in range(len(s.S)):
        d = {}
        for tag, e in (("o", o), ("o32", o32), ("z", z), ("z32", z32)):
            oracle_run(e, s, i)
            if tag in ("o", "o32"):
                d[tag] = dict(C=e.last_contacts_full(), iters=e.last_iterations, state=e.get_state(), tau=e.get_aux()[0],
                              normal=e.last_normal_impulses(512),
                              rows={k: e.last_rows(k) for k in ("noncontact", "normals", "frictions")})
            else:
                d[tag] = dict(v=velocities(e.get_state(), n), box=e.get_box()[0] if s.box is not None else None)
                e.set_state(inputs64(s, i)[0])
                d[tag]["minv"] = np.array([e.minv_mul(np.eye(6 + n)[j]) for j in range(6 + n)])
        d["params"] = o.params
        d["model"] = None
        if s.box is None:
            s64, t64, _, _, mu = inputs64(s, i)
            d["model"] = ns.substep(o.params, s64, t64, d["o"]["C"], mu_plane=mu, n_iterations=0)
        out.append(d)
    _refs[key] = out
    return out


def body_of(link, L):
    """The composite body of the kernels' records for a tree link of the oracle's (-1: the free box)."""
    return L["kBoxBody"] if link < 0 else (ns.cylinder_of_link(int(link)) + 1) >> 1


def decoded(g, r, i):
    """The decoded block of state i, after the count and body checks every stage starts with."""
    C = r[i]["o"]["C"]
    assert g["info"][i, 1] == len(C), ("contact count", i, g["info"][i], len(C))
    nplane = int(((C[:, 4] >= 0) & (C[:, 5] == -1)).sum()) if len(C) else 0
    assert (C[:nplane, 5] == -1).all() and (C[:nplane, 4] >= 0).all(), "the snake's ground contacts come first"
    return nr.decode(g["blocks"][i], g["layout"], len(C), nplane)


_stages = {}


def collected(fn):
    """A stage's collector: the exact assertions of one case and its error samples, computed once per case.  The unmarked
    `structure` tests call it for the assertions alone, the gated tests (some of them strict xfails) gate what it returns --
    so that an xfail cannot hide a structural failure."""
    def wrapper(pkg, oracle_mod, monkeypatch, *case):
        key = (fn.__name__,) + case
        if key not in _stages:
            _path(monkeypatch, case[0])
            _stages[key] = fn(pkg, oracle_mod, *case)
        return _stages[key]
    return wrapper


class Stage:
    """Collects (gpu, float32 yardstick) error samples per quantity and gates them."""

    def __init__(self, what):
        self.what, self.g, self.f, self.states = what, {}, {}, []

    def add(self, q, gpu, f32=None):
        self.g.setdefault(q, []).append(gpu)
        if f32 is not None:
            self.f.setdefault(q, []).append(f32)

    def gate(self):
        ok = True
        for q, g in self.g.items():
            g, f = np.array(g), np.array(self.f.get(q, [0.0]))
            assert np.isfinite(g).all(), (self.what, q)
            name = "%s: %s" % (self.what, q)
            ok &= f32_gate(name + " median of %d" % len(g), np.median(g), np.median(f), 1.5, 1e-6)
            ok &= f32_gate(name + " p90", np.percentile(g, 90), np.percentile(f, 90), 2.0, 1e-5)
            ok &= f32_gate(name + " worst", g.max(), f.max(), 2.0, 1e-5, 5e-2)
        return ok


def depth_err(x, ref):
    """A contact's distance: relative to a millimetre at least (it crosses zero; the collision margin is a millimetre)."""
    return abs(x - ref) / max(abs(ref), 1e-3)


def rhs_err(x, ref, dinv):
    """A row's rhs = target x dinv: relative to a target of 1e-3 (m/s, rad/s) at least (it crosses zero)."""
    return abs(x - ref) / max(abs(ref), 1e-3 * dinv)


# ------------------------------------------------------------------------------------------------------------------
# A. contact records
# ------------------------------------------------------------------------------------------------------------------
A_SETS_0 = [(p, s) for p in ROW_PATHS for s in ("default", "folded", "static box")] + [("streamed-row", "free box")]
# (plane friction 6: where the clamp of a combined coefficient at 10 bites, 2 x 6 -- the box's own is 0.5 x 6 = 3)
A_SETS = A_SETS_0 + [("streamed-row", "free box, plane friction 6")]


@collected
def stage_a(pkg, oracle_mod, path, name):
    """Per compact contact, in the solve's order: P, dist, normal, PB (two-body contacts) against the float64 oracle's
    contacts; the two friction directions against plane_space / aniso of the numpy model (test_np_rows.model_dirs: link A's
    anisotropy, then link B's; the box has none), yardstick the float32 oracle's rows' directions; bodies, counts and (to 2
    float32 ulps: three roundings) the friction scale exactly -- the pair's own coefficient, combined and then clamped at 10,
    over the snake's with the ground: min(mu_link^2, 10), min(mu_link mu_obstacle, 10), and for the free box against the
    ground min(mu_obstacle mu_plane, 10)."""
    s = the_set(oracle_mod, path, name)
    g, r = gpu_run(pkg, path, name, s), refs(oracle_mod, path, name, s)
    L = g["layout"]
    st = Stage("A %s, %s" % (path, name))
    two_body = box_ground = 0
    for i in range(len(s.S)):
        dec = decoded(g, r, i)
        C = r[i]["o"]["C"]
        F = model_dirs(r[i]["params"], inputs64(s, i)[0], C)
        C32, F32 = r[i]["o32"]["C"], r[i]["o32"]["rows"]["frictions"]["dir"]
        same = len(C32) == len(C) and np.array_equal(C32[:, 4:6], C[:, 4:6])
        p = r[i]["params"]
        mu_plane = inputs64(s, i)[4]
        mu_g = min(p.mu_link * mu_plane, 10.0)
        for ci, c in enumerate(C):
            geo = dec["geo"][dec["slot"][ci]].astype(np.float64)
            la, lb = int(c[4]), int(c[5])
            assert int(geo[G["kA"]]) == body_of(la, L), (i, ci, geo[G["kA"]], la)
            kB = body_of(lb, L) if lb >= 0 else (L["kBoxBody"] if lb == -2 and p.obstacle == 2 else -1)
            assert int(geo[G["kB"]]) == kB, (i, ci, geo[G["kB"]], lb)
            if la >= 0 and lb == -1:
                assert geo[G["fscale"]] == 1.0
            elif mu_g == 0:
                pass            # (no finite scale: test_link_link_friction_without_ground_friction)
            else:
                if lb >= 0:
                    rho = min(p.mu_link ** 2, 10.0) / mu_g
                elif la >= 0:
                    rho = min(p.mu_link * p.mu_obstacle, 10.0) / mu_g
                else:
                    box_ground += 1
                    rho = min(p.mu_obstacle * mu_plane, 10.0) / mu_g
                assert abs(geo[G["fscale"]] - rho) <= 2.0 ** -22 * rho, (i, ci, la, lb, geo[G["fscale"]], rho)
            c32 = C32[ci] if same else None
            y = lambda f: None if c32 is None else f(c32)                  # noqa: E731
            st.add("P", relerr(geo[G["P"]], c[0:3]), y(lambda x: relerr(x[0:3], c[0:3])))
            st.add("dist", depth_err(geo[G["dist"]], c[3]), y(lambda x: depth_err(x[3], c[3])))
            st.add("normal", relerr(geo[G["normal"]], c[6:9]), y(lambda x: relerr(x[6:9], c[6:9])))
            if lb != -1:
                two_body += 1
                st.add("PB", relerr(geo[G["PB"]], c[9:12]), y(lambda x: relerr(x[9:12], c[9:12])))
            st.add("direction A", relerr(geo[G["dirA"]], F[2 * ci]), relerr(F32[2 * ci], F[2 * ci]) if same else None)
            st.add("direction B", relerr(geo[G["dirB"]], F[2 * ci + 1]), relerr(F32[2 * ci + 1], F[2 * ci + 1]) if same else None)
    if name != "default":
        assert two_body > 0
    if name.startswith("free box"):
        assert box_ground >= len(s.S), "the box's own ground contacts are among the records"
    return st


# the sets that miss a gate, with the figure that misses it by most
A_OPEN = {
    ("streamed-row", "folded"): "direction A worst 1.0e-04 against the float32 oracle's 4.9e-05 (2.1 x)",
    ("streamed-row", "static box"): "direction A worst 1.6e-05 against the float32 oracle's 7.3e-06 (2.1 x)",
    ("32 links", "static box"): "direction B worst 1.1e-05 against the float32 oracle's 1.5e-06 (7.3 x)",
}


@pytest.mark.parametrize("path,name", A_SETS)
def test_stage_a_structure(pkg, oracle_mod, monkeypatch, path, name):
    stage_a(pkg, oracle_mod, monkeypatch, path, name)


@pytest.mark.parametrize("path,name", [pytest.param(p, s, marks=[_open(A_OPEN[(p, s)])] if (p, s) in A_OPEN else [])
                                       for p, s in A_SETS])
def test_stage_a_contact_records(pkg, oracle_mod, monkeypatch, path, name):
    assert stage_a(pkg, oracle_mod, monkeypatch, path, name).gate()


# ------------------------------------------------------------------------------------------------------------------
# B. free motion
# ------------------------------------------------------------------------------------------------------------------
B_SETS = [(p, s) for p in ROW_PATHS for s in ("default", "velocity clamp", "in the air")] + [("streamed-row", "free box")]


@pytest.mark.parametrize("path,name", B_SETS)
def test_stage_b_free_motion(pkg, oracle_mod, monkeypatch, path, name):
    """n_iterations 0 (module docstring: where the epilogue is read): the output velocities are clamp(v_free), against the
    numpy model's v_free; with the free box, which the model leaves out, against the float64 oracle at n_iterations 0
    (the box's six components as a vector of their own)."""
    _path(monkeypatch, path)
    s = the_set(oracle_mod, path, name)
    g, r = gpu_run(pkg, path, name, s, n_iterations=0), refs(oracle_mod, path, name, s)
    st = Stage("B %s, %s" % (path, name))
    for i in range(len(s.S)):
        assert g["info"][i, 0] == 0
        ref = r[i]["model"]["v_free"] if r[i]["model"] is not None else r[i]["z"]["v"]
        st.add("v_free", relerr(velocities(g["state"][i], s.n), ref), relerr(r[i]["z32"]["v"], ref))
        assert np.all(g["aux"][i, :s.n] == 0), "no sweep: no motor impulse"
        if s.box is not None:
            st.add("box v_free", relerr(g["box"][i, 7:13], r[i]["z"]["box"][7:13]),
                   relerr(r[i]["z32"]["box"][7:13], r[i]["z"]["box"][7:13]))
    if name == "velocity clamp":
        assert (np.abs(np.array([velocities(x, s.n) for x in g["state"]])) == 100.0).any()
    assert st.gate()


# ------------------------------------------------------------------------------------------------------------------
# C. M^-1
# ------------------------------------------------------------------------------------------------------------------
def box_minv(p, quat):
    """diag(R I^-1 R^T, 1 / m) of the free box: btBoxShape's inertia of the nominal box (snk_model.hpp)."""
    x, y, z, w = quat
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    l = 2 * np.array(p.obstacle_half[:])
    m = p.obstacle_mass
    I = m / 12 * np.array([l[1] ** 2 + l[2] ** 2, l[0] ** 2 + l[2] ** 2, l[0] ** 2 + l[1] ** 2])
    out = np.zeros((6, 6))
    out[:3, :3] = R @ np.diag(1 / I) @ R.T
    out[3:, 3:] = np.eye(3) / m
    return out


@pytest.mark.parametrize("path,name", [(p, "default") for p in ROW_PATHS] + [(p, "folded") for p in ROW_PATHS]
                         + [("streamed-row", "free box")])
def test_stage_c_inverse_mass_matrix(pkg, oracle_mod, monkeypatch, path, name):
    """The block's ND x ND part row by row against inv(M) of the numpy model (free box: the float64 oracle's M^-1); its
    asymmetry |row j - column j| / |row j| to the same gate; columns >= ND exactly zero; the six rows behind it zero
    without a free box and diag(R I^-1 R^T, 1 / m) with one (R from the box state handed over, float32 round-off: 1e-6)."""
    _path(monkeypatch, path)
    s = the_set(oracle_mod, path, name)
    g, r = gpu_run(pkg, path, name, s), refs(oracle_mod, path, name, s)
    L = g["layout"]
    ND = L["ND"]
    st = Stage("C %s, %s" % (path, name))
    for i in range(len(s.S)):
        dec = decoded(g, r, i)
        A = dec["minv"][:ND, :ND].astype(np.float64)
        ref = np.linalg.inv(r[i]["model"]["M"]) if r[i]["model"] is not None else r[i]["z"]["minv"]
        y = r[i]["z32"]["minv"]
        for j in range(ND):
            e32 = relerr(y[j], ref[j])
            st.add("row", relerr(A[j], ref[j]), e32)
            st.add("asymmetry", relerr(A[:, j], A[j]), e32)
        if s.box is None:
            assert np.all(dec["minv"][:ND, ND:] == 0) and np.all(dec["minv"][ND:] == 0)
        else:
            assert np.all(dec["minv"][:ND, ND:] == 0) and np.all(dec["minv"][ND:, :ND] == 0)
            assert np.all(dec["minv"][ND:, ND + 6:] == 0)
            want = box_minv(r[i]["params"], inputs64(s, i)[3][0][3:7])
            got = dec["minv"][ND:, ND:ND + 6].astype(np.float64)
            assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), (i, got, want)
    assert st.gate()


# ------------------------------------------------------------------------------------------------------------------
# D. rows
# ------------------------------------------------------------------------------------------------------------------
def reference_rows(d):
    """Per kind n / A / B the reference rows of one state, [(J dinv, M^-1 J^T, den, rhs, dinv)]: the numpy model's, or the
    float64 oracle's where the model has none (free box); and the float32 oracle's in the same form (None: other counts)."""
    def of_oracle(rows):
        N, F = rows["normals"], rows["frictions"]
        f = lambda R, k: (R["J"][k] * R["dinv"][k], R["M"][k], 1 / R["dinv"][k] if R["dinv"][k] else 0.0, R["rhs"][k],   # noqa: E731
                          R["dinv"][k])
        nc = len(N["dinv"])
        return dict(n=[f(N, k) for k in range(nc)], A=[f(F, 2 * k) for k in range(nc)], B=[f(F, 2 * k + 1) for k in range(nc)])
    if d["model"] is not None:
        f = lambda m: (m.J * m.dinv, m.Mi, 1 / m.dinv if m.dinv else 0.0, m.rhs, m.dinv)      # noqa: E731
        ref = dict(n=[f(m) for m in d["model"]["normals"]], A=[f(a) for a, _ in d["model"]["pairs"]],
                   B=[f(b) for _, b in d["model"]["pairs"]])
    else:
        ref = of_oracle(d["o"]["rows"])
    y = of_oracle(d["o32"]["rows"])
    return ref, (y if len(y["n"]) == len(ref["n"]) else None)


D_SETS = A_SETS_0 + [(p, s) for p in ROW_PATHS for s in ("plane friction 6", "friction_directions 1")]
# The sets that miss a gate, with the figure that misses it by most: medians of the normal rows' den, J / den and rhs, and
# single worst rows at 2 to 4.4 x the float32 oracle's worst.  DESIGN.md 3 says where the den's error comes from
# (test_stage_d_den_decomposition prints it).
D_OPEN = {
    ("streamed-row", "default"): "friction M^-1 J^T worst 4.6e-05 against the float32 oracle's 1.4e-05 (3.3 x)",
    ("streamed-row", "folded"): "normal J/den worst 2.5e-04 against the float32 oracle's 5.7e-05 (4.3 x)",
    ("streamed-row", "static box"): "normal rhs median 2.1e-06 against the float32 oracle's 1.1e-06 (1.9 x)",
    ("32 links", "default"): "normal rhs median 1.4e-06 against the float32 oracle's 7.4e-07 (1.9 x)",
    ("32 links", "folded"): "normal rhs worst 3.9e-03 against the float32 oracle's 1.9e-03 (2.0 x)",
    ("32 links", "static box"): "normal J/den median 1.3e-06 against the float32 oracle's 5.4e-07 (2.5 x)",
    ("streamed-row", "free box"): "normal rhs median 1.9e-06 against the float32 oracle's 1.0e-06 (1.8 x)",
    ("streamed-row", "plane friction 6"): "normal J/den median 1.1e-06 against the float32 oracle's 4.8e-07 (2.2 x)",
    ("streamed-row", "friction_directions 1"): "friction M^-1 J^T worst 3.2e-05 against the float32 oracle's 1.2e-05 (2.7 x)",
    ("32 links", "friction_directions 1"): "normal J/den median 1.4e-06 against the float32 oracle's 7.8e-07 (1.8 x)",
}


@collected
def stage_d(pkg, oracle_mod, path, name):
    """J / den, M^-1 J^T, den and rhs of every normal and both friction rows of every contact against the numpy model's
    rows (free box: the float64 oracle's), in the model's units (np_rows.contact_rows undoes the friction scale of a
    two-body pair).  A row whose den is not above the kernel's threshold holds J / den = 0 and rhs = 0 (under
    friction_directions 1 every second tangent: its direction is scaled by 0); the columns beyond the velocity components
    are zero."""
    s = the_set(oracle_mod, path, name)
    g, r = gpu_run(pkg, path, name, s), refs(oracle_mod, path, name, s)
    L = g["layout"]
    st = Stage("D %s, %s" % (path, name))
    dead = 0
    for i in range(len(s.S)):
        dec = decoded(g, r, i)
        rows, raw = nr.contact_rows(dec, L), nr.record_rows(dec, L)
        ref, y = reference_rows(r[i])
        one_dir = int(r[i]["params"].friction_directions) == 1
        for kind, tag in (("n", "normal"), ("A", "friction"), ("B", "friction")):
            R = rows[kind]
            for ci, (Jd, Mv, den, rhs, dinv) in enumerate(ref[kind]):
                nd = len(Jd)
                assert np.all(R["Jd"][ci, nd:] == 0) and np.all(R["M"][ci, nd:] == 0), (i, kind, ci)
                if not raw[kind]["den"][ci] > nr.DEN_MIN:
                    # the kernel's threshold is float32's epsilon on the record's own den, the float32 oracle's rule; the
                    # float64 programs keep a row down to THEIR epsilon -- the reference's den must be at the threshold too
                    dead += 1
                    assert np.all(R["Jd"][ci] == 0) and R["rhs"][ci] == 0, (i, kind, ci)
                    unit = raw[kind]["den"][ci] / R["den"][ci] if R["den"][ci] > 0 else 1.0      # (the pair's friction scale)
                    assert (kind == "B" and one_dir) or den * unit <= 2 * nr.DEN_MIN, (i, kind, ci, raw[kind]["den"][ci], den)
                    continue
                assert dinv != 0, (i, kind, ci)
                f = None if y is None or y[kind][ci][4] == 0 else y[kind][ci]
                st.add(tag + " J/den", relerr(R["Jd"][ci, :nd], Jd), None if f is None else relerr(f[0], Jd))
                st.add(tag + " M^-1 J^T", relerr(R["M"][ci, :nd], Mv), None if f is None else relerr(f[1], Mv))
                st.add(tag + " den", abs(R["den"][ci] / den - 1), None if f is None else abs(f[2] / den - 1))
                st.add(tag + " rhs", rhs_err(R["rhs"][ci], rhs, dinv), None if f is None else rhs_err(f[3], rhs, dinv))
    if name == "friction_directions 1":
        assert dead > 0
    return st


@pytest.mark.parametrize("path,name", D_SETS)
def test_stage_d_structure(pkg, oracle_mod, monkeypatch, path, name):
    """The exact part of stage D alone: counts, zero columns, the dead-row rule."""
    stage_d(pkg, oracle_mod, monkeypatch, path, name)


@pytest.mark.parametrize("path,name", [pytest.param(p, s, marks=[_open(D_OPEN[(p, s)])] if (p, s) in D_OPEN else [])
                                       for p, s in D_SETS])
def test_stage_d_rows(pkg, oracle_mod, monkeypatch, path, name):
    assert stage_d(pkg, oracle_mod, monkeypatch, path, name).gate()


@pytest.mark.parametrize("path", ROW_PATHS)
def test_stage_d_den_decomposition(pkg, oracle_mod, monkeypatch, path):
    """Where a normal row's den gets its error, on the default set; every figure a median over the set's normal
    rows, printed as a DIAG line.  Asserted: the wave reduction.  The stored den against J . M^-1 J^T of the same record
    summed in float64 is within (38 + 2) float32 roundings of sum |J_d M_d| (a 38-term float32 sum of float32 products of a
    J recovered as (J / den) den)."""
    _path(monkeypatch, path)
    s = the_set(oracle_mod, path, "default")
    g, r = gpu_run(pkg, path, "default", s), refs(oracle_mod, path, "default", s)
    e = {k: [] for k in ("stored den : own J.M", "J", "M^-1 J^T", "GPU J . model M^-1 J^T : model den",
                         "model J . GPU M^-1 J^T : model den", "float32 oracle den : model den",
                         "float32 oracle M^-1 J^T", "float32 oracle J.M : model den")}
    for i in range(len(s.S)):
        dec = decoded(g, r, i)
        rows = nr.record_rows(dec, g["layout"])["n"]
        R = r[i]["o32"]["rows"]["normals"]
        for ci, m in enumerate(r[i]["model"]["normals"]):
            nd, den, dm = len(m.J), rows["den"][ci], 1 / m.dinv
            Jg, Mg = rows["Jd"][ci, :nd] * den, rows["M"][ci, :nd]
            own = Jg @ Mg
            assert abs(den - own) <= 40 * 2.0 ** -24 * np.abs(Jg * Mg).sum(), (i, ci, den, own)
            e["stored den : own J.M"].append(abs(den / own - 1))
            e["J"].append(relerr(Jg, m.J))
            e["M^-1 J^T"].append(relerr(Mg, m.Mi))
            e["GPU J . model M^-1 J^T : model den"].append(abs(Jg @ m.Mi / dm - 1))
            e["model J . GPU M^-1 J^T : model den"].append(abs(m.J @ Mg / dm - 1))
            if len(R["dinv"]) == len(r[i]["model"]["normals"]) and R["dinv"][ci]:
                e["float32 oracle den : model den"].append(abs(1 / R["dinv"][ci] / dm - 1))
                e["float32 oracle M^-1 J^T"].append(relerr(R["M"][ci], m.Mi))
                e["float32 oracle J.M : model den"].append(abs(R["J"][ci] @ R["M"][ci] / dm - 1))
    assert len(e["J"]) > 100
    for k, v in e.items():
        print("  DIAG D %s, default, %d normal rows: %-38s median %.2e p90 %.2e worst %.2e"
              % (path, len(v), k, np.median(v), np.percentile(v, 90), max(v)))


@_open("the friction scale of every link-link contact is 0 at plane friction 0 (snk_selfcol.hpp: rho = mu_ground > 0 ? mu_self / "
       "mu_ground : 0), its pair's M^-1 J^T records are zero")
def test_link_link_friction_without_ground_friction(pkg, oracle_mod, monkeypatch):
    """Plane friction 0 on the 16-link folded set.  The rule (np_substep, the oracle): a link-link pair is bounded by
    min(mu_link^2, 10) lambda_n whatever the plane's coefficient is.  The kernels bound every pair by mu_ground lambda_n
    and write a two-body pair's rows in units of mu_pair / mu_ground, which has no finite value at mu_ground 0: they write
    0, the pair's M^-1 J^T is zero and link-link friction vanishes with the ground's.  Open: the fix changes device code."""
    _path(monkeypatch, "streamed-row")
    f = the_set(oracle_mod, "streamed-row", "folded")
    s = Set(f.n, f.S, f.T, f.over, 0.0)
    g, r = gpu_run(pkg, "streamed-row", "folded at 0", s), refs(oracle_mod, "streamed-row", "folded at 0", s)
    pairs = 0
    for i in range(len(s.S)):
        dec = decoded(g, r, i)
        F = r[i]["o"]["rows"]["frictions"]
        for ci, c in enumerate(r[i]["o"]["C"]):
            if c[5] >= 0 and F["dinv"][2 * ci] != 0:
                pairs += 1
                assert np.abs(dec["fMA"][ci]).max() > 0, (i, ci, dec["geo"][dec["slot"][ci]][G["fscale"]])
    assert pairs > 0


@pytest.mark.parametrize("path", ROW_PATHS)
def test_rows_do_not_depend_on_ground_friction(pkg, oracle_mod, monkeypatch, path):
    """Ground contacts only: the whole block is bit-equal between plane friction 0 and 6."""
    _path(monkeypatch, path)
    s6 = the_set(oracle_mod, path, "plane friction 6")
    s0 = Set(s6.n, s6.S, s6.T, s6.over, 0.0)
    a, b = gpu_run(pkg, path, "plane friction 6", s6), gpu_run(pkg, path, "plane friction 6 at 0", s0)
    assert np.array_equal(a["info"][:, 1], b["info"][:, 1]) and a["info"][:, 1].max() > 0
    assert np.array_equal(a["blocks"].view(np.uint32), b["blocks"].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------
# E. the solve on the kernel's own rows
# ------------------------------------------------------------------------------------------------------------------
# The cases that miss a gate, with the figure that misses it by most.  The samples are small and bimodal (states with and
# without contacts), and float32 evaluations of equal validity scatter as far (test_stage_e_float32_orderings).
E_OPEN = {
    ("streamed-row", "default", 1): "velocity median 2.1e-06 against the float32 replay's 1.4e-06 (1.5 x)",
    ("streamed-row", "cone_friction 0", 2): "velocity worst 1.1e-05 against the float32 replay's 5.2e-06 (2.1 x)",
    ("streamed-row", "friction_directions 1", 2): "normal impulse median 2.9e-06 against the float32 replay's 1.8e-06 (1.6 x)",
    ("streamed-row", "friction_directions 1", 5): "velocity median 1.1e-06 against the float32 replay's 5.4e-07 (2.0 x)",
    ("streamed-row", "plane friction 0", 2): "normal impulse median 2.3e-06 against the float32 replay's 1.5e-06 (1.6 x)",
    ("streamed-row", "velocity clamp", 5): "normal impulse median 1.1e-06 against the float32 replay's 5.7e-07 (2.0 x)",
    ("streamed-row", "past the limits", 5): "normal impulse median 3.3e-06 against the float32 replay's 1.4e-06 (2.3 x)",
    ("32 links", "default", 2): "velocity median 1.2e-05 against the float32 replay's 3.8e-06 (3.3 x)",
    ("32 links", "default", 5): "velocity median 3.0e-05 against the float32 replay's 7.5e-06 (4.0 x)",
    ("32 links", "cone_friction 0", 5): "motor torque worst 2.2e-05 against the float32 replay's 8.8e-06 (2.5 x)",
    ("32 links", "friction_directions 1", 5): "normal impulse median 9.8e-06 against the float32 replay's 4.6e-06 (2.1 x)",
    ("32 links", "plane friction 0", 1): "normal impulse worst 4.1e-05 against the float32 replay's 2.0e-05 (2.1 x)",
    ("32 links", "plane friction 6", 5): "motor torque p90 7.6e-05 against the float32 replay's 2.5e-05 (3.0 x)",
    ("32 links", "past the limits", 2): "normal impulse median 2.8e-06 against the float32 replay's 1.8e-06 (1.6 x)",
    ("32 links", "past the limits", 5): "normal impulse worst 1.2e-05 against the float32 replay's 5.7e-06 (2.2 x)",
}


def _e_cases():
    for path in ROW_PATHS:
        for scenario in SCENARIOS:
            for k in (1, 2, 5):
                why = E_OPEN.get((path, scenario, k))
                yield pytest.param(path, scenario, k, marks=[_open(why)] if why else [])


def cached_normals(manifold, n):
    """The normal impulses the substep wrote back to the contact cache, in the order of the compact list: cylinder by
    cylinder, cached point by cached point."""
    return np.array([manifold[c, 7 + 7 * j] for c in range(2 * n) for j in range(int(manifold[c, 0]))], np.float64)


@collected
def stage_e(pkg, oracle_mod, path, scenario, k):
    """replay(float64) on the decoded float32 records -- the non-contact rows from the block's M^-1 and stage B's float32
    v_free -- against the GPU's motor torques, the normal impulses in the contact cache and clip(v_free + dv); yardstick:
    replay(float32) against replay(float64) on the same records.  No row building in this stage: it gates row_step_normal,
    row_step_normal2 (its coupling scalar included: the replay takes the rows one by one), row_step_cone, the pyramid path
    and the limit / motor steps."""
    s = the_set(oracle_mod, path, scenario)
    n = s.n
    g = gpu_run(pkg, path, scenario, s, n_iterations=k)
    g0 = gpu_run(pkg, path, scenario, s, n_iterations=0)
    o = oracle_mod.OracleEnv(n_modules=n, **MIRROR, **dict(s.over, n_iterations=k))
    L = g["layout"]
    st = Stage("E %s, %s, %d sweeps" % (path, scenario, k))
    mx = float(o.params.max_coord_vel)
    for i in range(len(s.S)):
        oracle_run(o, s, i)
        C = o.last_contacts_full()
        assert g["info"][i, 1] == len(C), (i, g["info"][i], len(C))
        nplane = int((C[:, 5] == -1).sum())
        assert (C[:nplane, 5] == -1).all()
        dec = nr.decode(g["blocks"][i], L, len(C), nplane)
        assert np.array_equal(dec["minv"], nr.decode(g0["blocks"][i], L, len(C), nplane)["minv"])
        v32 = velocities(g0["state"][i], n).astype(np.float32)
        S32, T32 = np.asarray(s.S[i], np.float32), np.asarray(s.T[i], np.float32)
        nonc = nr.noncontact_of_block(dec, L, o.params, S32[13:13 + n], T32, v32)
        rows = nr.record_rows(dec, L, np.float32)
        mu = float(np.float32(min(np.float32(o.params.mu_link) * np.float32(inputs64(s, i)[4]), np.float32(10.0))))
        a = nr.replay(rows, nonc, mu, o.params, k, np.float64, thr=-1.0)
        b = nr.replay(rows, nonc, mu, o.params, k, np.float32, thr=-1.0)
        nd = 6 + n
        out = lambda x: np.clip(v32.astype(np.float64) + np.asarray(x["dv"], np.float64)[:nd], -mx, mx)      # noqa: E731
        dt = float(o.params.dt)
        lam = cached_normals(g["manifold"][i].astype(np.float64), n)
        assert len(lam) == nplane, (i, len(lam), nplane)      # (a link-link contact has no cache: its impulse is not read)
        st.add("velocity", relerr(velocities(g["state"][i], n), out(a)), relerr(out(b), out(a)))
        st.states.append(dict(rows=rows, nonc=nonc, mu=mu, a=a,
                              out=lambda x, v=v32: np.clip(v.astype(np.float64) + np.asarray(x["dv"], np.float64)[:nd], -mx, mx), gpu=velocities(g["state"][i], n), nc=len(C)))
        sc = max(np.abs(a["motor"]).max(), dt)            # (a torque of 1 at least: the floor of test_gpu_np_substep._run)
        st.add("motor torque", np.abs(g["aux"][i, :n] * dt - a["motor"]).max() / sc,
               np.abs(b["motor"].astype(np.float64) - a["motor"]).max() / sc)
        if nplane:
            st.add("normal impulse", relerr(lam, a["normal"][:nplane]), relerr(b["normal"][:nplane], a["normal"][:nplane]))
    return st


@pytest.mark.parametrize("path,scenario,k", [(p, sc, k) for p in ROW_PATHS for sc in SCENARIOS for k in (1, 2, 5)])
def test_stage_e_structure(pkg, oracle_mod, monkeypatch, path, scenario, k):
    """The exact part of stage E alone: counts, the bit-equal M^-1 of the two handles, one cached impulse per ground contact."""
    stage_e(pkg, oracle_mod, monkeypatch, path, scenario, k)


@pytest.mark.parametrize("path,scenario,k", list(_e_cases()))
def test_stage_e_solve_on_the_kernels_rows(pkg, oracle_mod, monkeypatch, path, scenario, k):
    assert stage_e(pkg, oracle_mod, monkeypatch, path, scenario, k).gate()


@pytest.mark.parametrize("scenario", ["default", "plane friction 6"])
def test_stage_e_float32_orderings(pkg, oracle_mod, monkeypatch, scenario):
    """How far equally valid float32 evaluations of the SAME sweep lie apart, on the 32-link states at 2 sweeps:
    the float32 replay taking the rows one by one (the yardstick), with the kernel's normal pairs and coupling scalar, with
    the kernel's motor step, with both (np_rows.replay_kernel_order; tests/test_np_rows.py holds it to replay() in float64)
    -- each one's velocity error against replay(float64), printed as DIAG lines beside the GPU's.  Asserted, per state with
    contacts: the GPU is within 10 x the furthest of the four (one decimal of scatter among them is what they show)."""
    st = stage_e(pkg, oracle_mod, monkeypatch, "32 links", scenario, 2)
    p = oracle_mod.OracleEnv(n_modules=32, **MIRROR, **dict(the_set(oracle_mod, "32 links", scenario).over, n_iterations=2)).params
    E = {k: [] for k in ("GPU", "rows one by one", "normal pairs", "motor form", "pairs and motor form")}
    for d in st.states:
        ref = d["out"](d["a"])
        E["GPU"].append(relerr(d["gpu"], ref))
        E["rows one by one"].append(relerr(d["out"](nr.replay(d["rows"], d["nonc"], d["mu"], p, 2, np.float32, thr=-1.0)), ref))
        for key, kw in (("normal pairs", dict(motor_form=False)), ("motor form", dict(pairs=False)), ("pairs and motor form", {})):
            E[key].append(relerr(d["out"](nr.replay_kernel_order(d["rows"], d["nonc"], d["mu"], p, 2, np.float32, **kw)), ref))
        if d["nc"]:
            assert E["GPU"][-1] <= 10 * max(E[k][-1] for k in E if k != "GPU"), {k: v[-1] for k, v in E.items()}
    for k, v in E.items():
        print("  DIAG E 32 links, %s, 2 sweeps, velocity of %d states: %-22s median %.2e worst %.2e | per state %s"
              % (scenario, len(v), k, np.median(v), max(v), " ".join("%.1e" % x for x in v)))


# ------------------------------------------------------------------------------------------------------------------
# F. hygiene, and the read-out's contract
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,name", [(p, s) for p in ROW_PATHS for s in ("default", "folded")])
def test_stage_f_hygiene_under_poison(pkg, oracle_mod, monkeypatch, path, name):
    """SNK_POISON=1: every float of the normal and friction records below nc_pad (nc rounded up to 8) is finite, the records
    between nc and nc_pad are zero, and so are the three trailing rows and the pad columns (and, without a free box, the
    six last rows) of the M^-1 block."""
    _path(monkeypatch, path)
    monkeypatch.setenv("SNK_POISON", "1")
    s = the_set(oracle_mod, path, name)
    B = len(s.S)
    st = pkg.Stepper(B, n_modules=s.n, **s.over)
    st.set_state(np.asarray(s.S, np.float32))
    info = st.substep(np.asarray(s.T, np.float32), 1)
    blocks = st.debug_rows()
    L = st.debug_rows_layout()
    st.close()
    odd = 0
    for i in range(B):
        nc = int(info[i, 1])
        pad = (nc + 7) // 8 * 8
        odd += nc & 1
        dec = nr.decode(blocks[i], L, nc, max(nc - 32, 0))      # (any admissible split: the geometry slots are not read here)
        for k in ("nJ", "nM", "fJA", "fJB", "fMA", "fMB"):
            assert np.isfinite(dec[k][:pad]).all(), (i, k)
            assert np.all(dec[k][nc:pad] == 0), (i, k, nc, pad)
        assert np.all(dec["zero"] == 0)
        assert np.all(dec["minv"][:L["ND"], L["ND"]:] == 0) and np.all(dec["minv"][L["ND"]:] == 0)
        assert np.isfinite(dec["minv"]).all()
    assert info[:, 1].max() > 0 and odd > 0


def test_debug_rows_contract(pkg, monkeypatch):
    """debug_rows refuses, with a message that names the condition: a register-resident handle; a streamed-row handle
    before any substep and after step().  The third refusal -- more environments than resident waves -- is left to reading
    snk_debug_rows: the condition is `n_envs > grid_waves`, a handle that meets it holds more environments than the card
    has resident waves (thousands), and the host code has no path without a device."""
    st = pkg.Stepper(2)
    st.substep(np.zeros((2, 16), np.float32), 1)
    with pytest.raises(RuntimeError, match="register-resident"):
        st.debug_rows()
    st.close()
    monkeypatch.setenv("SNK_FORCE_STREAMED", "1")
    st = pkg.Stepper(2)
    with pytest.raises(RuntimeError, match="was not a substep"):
        st.debug_rows()
    st.substep(np.zeros((2, 16), np.float32), 1)
    assert st.debug_rows().shape == (2, st.debug_rows_layout()["kRowFloats"])
    st.reset()
    st.step(np.zeros((2, st.act_dim), np.float32))
    with pytest.raises(RuntimeError, match="was not a substep"):
        st.debug_rows()
    st.substep(np.zeros((2, 16), np.float32), 1)
    st.debug_rows()
    st.get_state()
    st.debug_rows()                     # (an accessor is no launch)
    st.reset()
    with pytest.raises(RuntimeError, match="was not a substep"):
        st.debug_rows()
    st.close()
