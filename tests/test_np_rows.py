"""tests/np_rows.py and the oracle's kept rows (CPU): the decoder of the streamed-row solve's block of rows against its
inverse and the layout restated from snk_lds.hpp; the float64 oracle's rows (OracleEnv.last_rows) against the rows of the
numpy model (tests/np_substep.py); the replayed sweep (np_rows.replay) against the oracle's own impulses; and the
yardstick table of tests/test_gpu_rows.py -- the float32 oracle's distance to the float64 reference stage by stage
(profiles/r15_rows_yardstick.txt is this file's output under SNK_WRITE_PROFILES=1).
"""
import os

import numpy as np
import pytest

import np_rows as nr
import np_substep as ns
from test_gpu_np_substep import _ground
from test_gpu_np_sweeps import _scenario
from test_np_substep import TOL_VEL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIRROR = dict(max_contacts=0, max_self_contacts=32)      # the kernels' room for link-link / box contacts (test_gpu_np_substep._run)
BOX = dict(obstacle=1, obstacle_pos=[0.100, 0.0, 0.1])

# snk_lds.hpp, Lds<N, false>, restated: ND = N + 6, NC = 8 N, kRing = 32 = kMaxSelf, NCT = NC + 32, kRows = 3 NCT + 3,
# kFric = NCT, kRS = 80, kMO = 40, kSpec = kMO - 2, kGeo = 20, kGeoOff = kRows kRS, kMmOff = kGeoOff + NCT kGeo,
# kYOff = kMmOff + (N + 12) kMO, kRowFloats = kYOff + (N + 2) 6 kMO, kBoxBody = N + 1
LAYOUT = {
    16: dict(ND=22, NC=128, NCT=160, kRows=483, kFric=160, kRS=80, kMO=40, kSpec=38, kGeo=20, kGeoOff=38640, kMmOff=41840,
             kYOff=42960, kRowFloats=47280, kBoxBody=17),
    32: dict(ND=38, NC=256, NCT=288, kRows=867, kFric=288, kRS=80, kMO=40, kSpec=38, kGeo=20, kGeoOff=69360, kMmOff=75120,
             kYOff=76880, kRowFloats=85040, kBoxBody=33),
}


def relerr(x, ref):
    """THE error measure of the row stages: |x - ref|_inf / |ref|_inf of one row or vector (0 / 0 = 0)."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    s = np.abs(ref).max()
    d = np.abs(x - ref).max()
    return d / s if s > 0 else (0.0 if d == 0 else np.inf)


# ------------------------------------------------------------------------------------------------------------------
# layout and round trip
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 32])
def test_layout_is_the_headers(pkg, n):
    from importlib import import_module
    lib = import_module("bullet-envs_amd._lib")
    got = lib.rows_layout(n)
    assert list(got) == list(lib.ROWS_LAYOUT)
    assert got == LAYOUT[n]
    assert got["NC"] == 8 * n and got["NCT"] == got["NC"] + 32 and got["kSpec"] + 2 == got["kMO"]


@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("nc", [0, 1, 2, 7, 8, 9, 15, 16, 17, 33, 128])
def test_round_trip(n, nc):
    """decode(encode(x)) == x and encode(decode(b)) == b bit for bit: nc 0, odd, even, a multiple of 8 and that +-1, with
    link-link contacts behind the ground's (their geometry slots start at NC)."""
    L = LAYOUT[n]
    rng = np.random.default_rng(100 * n + nc)
    b = rng.integers(0, 2 ** 32, L["kRowFloats"], dtype=np.uint64).astype(np.uint32)
    b &= np.uint32(0xFF7FFFFF)                   # no NaN payloads: every bit pattern a value numpy copies unchanged
    block = b.view(np.float32)
    nplane = nc - min(nc // 3, 32)
    dec = nr.decode(block, L, nc, nplane)
    again = nr.encode(dec, L)
    assert again.dtype == np.float32 and np.array_equal(again.view(np.uint32), b)
    dec2 = nr.decode(again, L, nc, nplane)
    for k, v in dec.items():
        assert np.array_equal(np.asarray(v).view(np.uint32) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v,
                              np.asarray(dec2[k]).view(np.uint32) if isinstance(v, np.ndarray) and v.dtype == np.float32
                              else dec2[k]), k
    # where a contact's numbers sit, from the layout comment alone
    ks = L["kSpec"]
    for ci in sorted({0, nc // 2, nc - 1} - {-1}) if nc else []:
        for d in (0, 5, ks, ks + 1):
            o = (ci >> 1) * 2 * L["kRS"] + 4 * d + 2 * (ci & 1)
            assert dec["nJ"][ci, d] == block[o] and dec["nM"][ci, d] == block[o + 1]
            o = (L["kFric"] + 2 * ci) * L["kRS"] + 4 * d
            assert (dec["fJA"][ci, d], dec["fJB"][ci, d], dec["fMA"][ci, d], dec["fMB"][ci, d]) == tuple(block[o:o + 4])
        slot = ci if ci < nplane else L["NC"] + ci - nplane
        assert dec["slot"][ci] == slot
        assert np.array_equal(dec["geo"][slot], block[L["kGeoOff"] + slot * 20:L["kGeoOff"] + slot * 20 + 20])
        rr = nr.record_rows(dec, L, np.float32)
        assert rr["n"]["rhs"][ci] == -dec["nJ"][ci, ks] and rr["n"]["den"][ci] == dec["nM"][ci, ks + 1]
    assert np.array_equal(dec["minv"][7], block[L["kMmOff"] + 7 * 40:L["kMmOff"] + 8 * 40])


# ------------------------------------------------------------------------------------------------------------------
# the state sets of the row stages (tests/test_gpu_rows.py runs the same)
# ------------------------------------------------------------------------------------------------------------------
def folded32(oracle_mod, k=3):
    """32 links folded onto themselves until the oracle finds link-link contacts."""
    rng = np.random.default_rng(3200)
    e = oracle_mod.OracleEnv(n_modules=32, **MIRROR)
    S = []
    while len(S) < k:
        s = _ground(rng, 32, 1, qamp=1.7)[0]
        e.set_state(s.astype(np.float32).astype(np.float64))
        C = e.contacts_full()
        if len(C) and (C[:, 5] >= 0).sum() >= 2:
            S.append(s)
    return np.array(S), rng.uniform(-0.5, 0.5, (k, 32))


def static_box(oracle_mod, k=4):
    """obstacle 1: gait states pushed into the box, with their contact caches (test_gpu_np_substep.test_static_box's)."""
    from bench import gait_actions
    rng = np.random.default_rng(1600)
    e = oracle_mod.OracleEnv(**BOX)
    S, M = [], []
    for i in range(k):
        e.hard_reset()
        e.reset()
        for j in range(8 + i % 6):
            e.env_step(gait_actions(np.array([i + 1]), j)[0], vec_mode=True)
        S.append(e.get_state())
        M.append(e.get_manifold())
    return np.array(S), rng.uniform(-0.5, 0.5, (k, 16)), np.array(M)


def state_sets(oracle_mod):
    """(name, n, S, T, parameter overrides, manifolds or None): every set of the oracle-rows comparison."""
    out = []
    for path, n, streamed in (("streamed-row", 16, True), ("32 links", 32, False)):
        for scenario in ("default", "past the limits"):
            S, T, over, mu, _ = _scenario(scenario, n, streamed)
            assert mu is None
            out.append(("%s, %s" % (path, scenario), n, S, T, over, None))
    S, T = folded32(oracle_mod)
    out.append(("32 links folded", 32, S, T, dict(residual_threshold=0.0), None))
    S, T, M = static_box(oracle_mod)
    out.append(("16 links against the static box", 16, S, T, dict(BOX, residual_threshold=0.0), M))
    return out


def model_dirs(params, s64, C):
    """[2 nc, 3]: the two friction directions of every contact of C as the numpy model makes them -- plane_space of the
    normal, each tangent scaled by R diag(aniso) R^T of link A, then of link B (a link-link contact); a box has none."""
    ch = ns.Chain(params)
    pos, quat, q, _ = ch.split(np.asarray(s64, float))
    Rw = ch.kinematics(pos, quat, q)[0]
    an = np.array(list(params.aniso), float)
    out = []
    for c in np.asarray(C).reshape(-1, 12):
        for d in ns.plane_space(c[6:9]):
            for link in (int(c[4]), int(c[5])):
                if link >= 0:
                    d = Rw[link] @ (an * (Rw[link].T @ d))
            out.append(d)
    return np.array(out).reshape(-1, 3)


def oracle_substep(e, s32, t32, M=None, mu=1.0):
    e.hard_reset()
    e.set_plane_friction(mu)
    if M is not None:
        e.set_manifold(np.asarray(M, np.float32).astype(np.float64))
    e.set_state(np.asarray(s32, np.float32).astype(np.float64))
    e.substep(np.asarray(t32, np.float32).astype(np.float64))


@pytest.fixture(scope="module")
def sets(oracle_mod):
    return state_sets(oracle_mod)


# ------------------------------------------------------------------------------------------------------------------
# the oracle's rows against the numpy model's
# ------------------------------------------------------------------------------------------------------------------
def test_oracle_rows_against_the_model(oracle_mod, sets):
    """Every state of every set: J, M^-1 J^T and 1 / dinv of every row to 100 cond(M) eps64 relative to the row's largest
    entry (the rows are solves with M: that is their conditioning), cond(M) taken per state.  rhs = target x dinv, the
    target -J . v_free plus position terms that both programs compute from the same inputs: v_free is held to TOL_VEL
    (1 + |v|) per component by tests/test_np_substep.py, so |d rhs| <= dinv TOL_VEL sum_i |J_i| (1 + |v_free_i|) (+ the
    row's own relative bound for its dinv)."""
    eps = np.finfo(np.float64).eps
    worst = {}
    for name, n, S, T, over, M in sets:
        o = oracle_mod.OracleEnv(n_modules=n, **MIRROR, **over)
        w = dict(J=0.0, M=0.0, den=0.0, rhs=0.0, rows=0)
        for i in range(len(S)):
            oracle_substep(o, S[i], T[i], None if M is None else M[i])
            s64, t64 = S[i].astype(np.float32).astype(np.float64), T[i].astype(np.float32).astype(np.float64)
            r = ns.substep(o.params, s64, t64, o.last_contacts_full(), n_iterations=0)
            tol = 100 * np.linalg.cond(r["M"]) * eps
            # the rows' world directions: the contact's normal, and plane_space / aniso of the model (1e-12: a handful of
            # float64 products on unit vectors)
            C = o.last_contacts_full()
            if len(C):
                assert np.abs(o.last_rows("normals")["dir"] - C[:, 6:9]).max() == 0
                dd = np.abs(o.last_rows("frictions")["dir"] - model_dirs(o.params, s64, C)).max()
                assert dd <= 1e-12, (name, i, dd)
                w["dir"] = max(w.get("dir", 0.0), dd)
            fr = [x for pair in r["pairs"] for x in pair]
            for kind, model in (("noncontact", r["noncontact"]), ("normals", r["normals"]), ("frictions", fr)):
                got = o.last_rows(kind)
                assert len(got["dinv"]) == len(model), (name, i, kind, len(got["dinv"]), len(model))
                for k, m in enumerate(model):
                    if kind == "noncontact":
                        assert got["joint"][k] == m.joint and (got["kind"][k] == 1) == (m.kind == "motor")
                    e = dict(J=relerr(got["J"][k], m.J), M=relerr(got["M"][k], m.Mi))
                    assert (got["dinv"][k] == 0) == (m.dinv == 0), (name, i, kind, k)
                    e["den"] = abs(m.dinv / got["dinv"][k] - 1) if m.dinv != 0 else 0.0
                    bound = m.dinv * (TOL_VEL * np.sum(np.abs(m.J) * (1 + np.abs(r["v_free"]))) + tol * abs(m.rhs / m.dinv
                                                                                                           if m.dinv else 0))
                    e["rhs"] = abs(got["rhs"][k] - m.rhs) / bound if bound > 0 else float(got["rhs"][k] != m.rhs)
                    for q in ("J", "M", "den"):
                        assert e[q] <= tol, (name, i, kind, k, q, e[q], tol)
                        w[q] = max(w[q], e[q] / tol)
                    assert e["rhs"] <= 1.0, (name, i, kind, k, got["rhs"][k], m.rhs, bound)
                    w["rhs"] = max(w["rhs"], e["rhs"])
                    w["rows"] += 1
        worst[name] = w
        print("  BOUND oracle rows, %-34s %4d rows: J %.2g, M^-1 J^T %.2g, 1/dinv %.2g, rhs %.2g of their bounds; directions %.1e"
              % (name, w["rows"], w["J"], w["M"], w["den"], w["rhs"], w.get("dir", 0.0)))
        assert w["rows"] > 0


# ------------------------------------------------------------------------------------------------------------------
# the replay against the oracle's own sweep
# ------------------------------------------------------------------------------------------------------------------
def oracle_rows_for_replay(o):
    fr = o.last_rows("frictions")
    N = o.last_rows("normals")
    rows = dict(n=nr.rows_of_oracle(N), A=nr.rows_of_oracle(fr, slice(0, None, 2)), B=nr.rows_of_oracle(fr, slice(1, None, 2)),
                start=N["start"])
    return rows, nr.noncontact_of_oracle(o.last_rows("noncontact"))


SWITCHES = {"cone_friction 1": {}, "cone_friction 0": dict(cone_friction=0), "friction_directions 1": dict(friction_directions=1),
            "warm_start 1": dict(warm_start=1)}


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("k", [1, 2, 5, 50])
def test_replay_reproduces_the_oracle(oracle_mod, sets, switch, k):
    """replay(float64) on the float64 oracle's own rows: its normal, friction and motor impulses to 1e-9 of the state's
    largest impulse -- the same arithmetic in the same precision, only the order of the sums differs.  States: the first
    two of every set; under warm_start 1 the sets that come with a contact cache (its points carry impulses)."""
    checked = 0
    for name, n, S, T, over, M in sets:
        if switch == "warm_start 1" and M is None:
            continue
        o = oracle_mod.OracleEnv(n_modules=n, **MIRROR, **dict(over, n_iterations=k, **SWITCHES[switch]))
        for i in range(2):
            oracle_substep(o, S[i], T[i], None if M is None else M[i])
            rows, nonc = oracle_rows_for_replay(o)
            C = o.last_contacts_full()
            mus = np.array([min(o.params.mu_link ** 2, 10.0) if lb >= 0 else
                            (min(o.params.mu_link * o.params.mu_obstacle, 10.0) if lb == -2 else
                             min(o.params.mu_link * 1.0, 10.0)) for lb in C[:, 5].astype(int)])
            if switch == "warm_start 1":
                assert np.abs(rows["start"]).max() > 0
            r = nr.replay(rows, nonc, mus, o.params, k, np.float64, thr=0.0)
            assert r["sweeps"] == o.last_iterations, (name, i, r["sweeps"], o.last_iterations)
            Nn, Ff, mot = o.last_normal_impulses(512), o.last_friction_impulses(512), o.get_aux()[0] * o.params.dt
            sc = max(np.abs(Nn).max() if len(Nn) else 0.0, np.abs(Ff).max() if len(Ff) else 0.0, np.abs(mot).max())
            err = max(np.abs(r["normal"] - Nn).max() if len(Nn) else 0.0, np.abs(r["friction"] - Ff).max() if len(Ff) else 0.0,
                      np.abs(r["motor"] - mot).max())
            print("  BOUND replay %-34s state %d, %2d sweeps, %s: %.2e <= 1e-09 (of %.3g)" % (name, i, k, switch, err / sc, sc))
            assert err <= 1e-9 * sc, (name, i, k, switch, err, sc)
            checked += 1
    assert checked >= 2


def test_kernel_order_replay_is_the_same_sweep(oracle_mod, sets):
    """replay_kernel_order in float64 -- normals in pairs with the coupling scalar, the motors' (rhs den - dv) / den -- against
    replay on the oracle's rows: 1e-9 of the largest impulse (the same sweep, reassociated)."""
    for name, n, S, T, over, M in sets:
        o = oracle_mod.OracleEnv(n_modules=n, **MIRROR, **dict(over, n_iterations=5))
        oracle_substep(o, S[1], T[1], None if M is None else M[1])
        rows, nonc = oracle_rows_for_replay(o)
        nc = len(rows["start"])
        if nc:
            a = nr.replay(rows, nonc, 2.0, o.params, 5, np.float64, thr=-1.0)
            b = nr.replay_kernel_order(rows, nonc, 2.0, o.params, 5, np.float64)
            sc = max(np.abs(a["normal"]).max(), np.abs(a["motor"]).max())
            assert np.abs(a["normal"] - b["normal"]).max() <= 1e-9 * sc and np.abs(a["motor"] - b["motor"]).max() <= 1e-9 * sc
            assert np.abs(a["dv"] - b["dv"]).max() <= 1e-9 * max(1.0, np.abs(a["dv"]).max())


def block_of_oracle(o, L, mu_ground):
    """A block as build_rows_v1 would leave it, encoded from the float64 oracle's last substep (values rounded to float32):
    the records in the solve's units (a two-body pair scaled by its coefficient over the ground's), geometry slots, M^-1."""
    C = o.last_contacts_full()
    N, F = o.last_rows("normals"), o.last_rows("frictions")
    nc, nd, ks = len(C), o.nd, L["kSpec"]
    nplane = int(((C[:, 4] >= 0) & (C[:, 5] == -1)).sum()) if nc else 0
    z = lambda *shape: np.zeros(shape, np.float32)                                  # noqa: E731
    dec = dict(nJ=z(L["NCT"], L["kMO"]), nM=z(L["NCT"], L["kMO"]), fJA=z(L["NCT"], L["kMO"]), fJB=z(L["NCT"], L["kMO"]),
               fMA=z(L["NCT"], L["kMO"]), fMB=z(L["NCT"], L["kMO"]), zero=z(3, L["kRS"]), geo=z(L["NCT"], L["kGeo"]),
               minv=z(L["ND"] + 6, L["kMO"]), Y=z(L["kRowFloats"] - L["kYOff"]))
    scale = []
    for ci in range(nc):
        lb = int(C[ci, 5])
        mu = min(o.params.mu_link ** 2, 10.0) if lb >= 0 else (min(o.params.mu_link * o.params.mu_obstacle, 10.0) if lb == -2
                                                              else mu_ground)
        sc = mu / mu_ground
        scale.append(sc)
        for J, M, R, k, f in (("nJ", "nM", N, ci, 1.0), ("fJA", "fMA", F, 2 * ci, sc), ("fJB", "fMB", F, 2 * ci + 1, sc)):
            den = 1 / R["dinv"][k] if R["dinv"][k] else 0.0
            dec[J][ci, :nd] = R["J"][k] * R["dinv"][k] / f
            dec[J][ci, ks] = -R["rhs"][k] / f
            dec[M][ci, :nd] = R["M"][k] * f
            dec[M][ci, ks + 1] = den * f
        slot = ci if ci < nplane else L["NC"] + ci - nplane
        g = dec["geo"][slot]
        g[0:3], g[3], g[4:7], g[7:10], g[10:13], g[13:16] = C[ci, 0:3], C[ci, 3], F["dir"][2 * ci], F["dir"][2 * ci + 1], C[ci, 6:9], C[ci, 9:12]
        g[16], g[17], g[18], g[19] = C[ci, 4], lb, sc, N["start"][ci]
    e = np.eye(nd)
    dec["minv"][:nd, :nd] = [o.minv_mul(e[j]) for j in range(nd)]
    return nr.encode(dec, L), nc, nplane, np.array(scale)


def test_decoded_block_is_the_oracles_rows(oracle_mod, sets):
    """A block encoded from the oracle's rows, in the solve's units: contact_rows gives the oracle's rows back to float32
    round-off (the friction scale of a two-body pair undone), and the float64 replay on its records -- one friction
    coefficient, the ground's, for every contact -- gives the oracle's impulses to the same."""
    two_body, worst = 0, 0.0
    for name, n, S, T, over, M in sets:
        L = LAYOUT[n]
        o = oracle_mod.OracleEnv(n_modules=n, **MIRROR, **dict(over, n_iterations=5))
        for i in range(2):
            oracle_substep(o, S[i], T[i], None if M is None else M[i])
            Nn, mot = o.last_normal_impulses(512), o.get_aux()[0] * o.params.dt
            nonc = nr.noncontact_of_oracle(o.last_rows("noncontact"))
            N, F = o.last_rows("normals"), o.last_rows("frictions")
            o.set_state(np.asarray(S[i], np.float32).astype(np.float64))
            mu_g = min(o.params.mu_link * 1.0, 10.0)
            block, nc, nplane, scale = block_of_oracle(o, L, mu_g)
            two_body += int((scale != 1).sum())
            dec = nr.decode(block, L, nc, nplane)
            rows = nr.contact_rows(dec, L)
            for kind, R, sel in (("n", N, slice(None)), ("A", F, slice(0, None, 2)), ("B", F, slice(1, None, 2))):
                ref = nr.rows_of_oracle(R, sel)
                for q in ("Jd", "M", "rhs", "den"):
                    got = rows[kind][q][:, :o.nd] if q in ("Jd", "M") else rows[kind][q]
                    sc = np.abs(ref[q]).max(axis=-1, keepdims=q in ("Jd", "M")) if nc else 1.0
                    assert np.all(np.abs(got - ref[q]) <= 2.0 ** -22 * np.maximum(sc, 1e-30)), (name, i, kind, q)
            r = nr.replay(nr.record_rows(dec, L), nonc, mu_g, o.params, 5, np.float64, thr=0.0)
            sc = max(np.abs(Nn).max() if nc else 0.0, np.abs(mot).max())
            err = max(np.abs(r["motor"] - mot).max(), np.abs(r["normal"] - Nn).max() if nc else 0.0) / sc
            print("  BOUND replay on the re-encoded block, %-34s state %d: %.1e <= 1e-04" % (name, i, err))
            worst = max(worst, err)
    assert two_body > 0
    # every record entry rounded to float32, then five float64 sweeps: no more than what rounding EVERY operation to float32
    # costs on these sets (the yardstick table's E5 lines: medians 1e-6, worst 1e-4)
    assert worst <= 1e-4, worst


# ------------------------------------------------------------------------------------------------------------------
# the yardstick: what float32 costs at every stage
# ------------------------------------------------------------------------------------------------------------------
def summary(x):
    x = np.asarray(x, np.float64)
    return (np.median(x), np.percentile(x, 90), x.max()) if len(x) else (0.0, 0.0, 0.0)


def oracle_stage_errors(oracle_mod, n, S, T, over, M, mu=1.0, sweeps=(1, 2, 5)):
    """The float32 oracle against the float64 one (and for stage E the float32 replay against the float64 replay on the
    float32-rounded rows of the float64 oracle), per quantity a list of relerr values over every row / vector of the set.
    Keys: "A P", "A dist", "A normal", "B v_free", "C M^-1", "D <kind> J/den | M^-1 J^T | den | rhs", "E<k> dv | normal |
    motor"."""
    mk = lambda f32, **kw: oracle_mod.OracleEnv(n_modules=n, f32=f32, **MIRROR, **dict(over, **kw))      # noqa: E731
    o, o32, z, z32 = mk(False), mk(True), mk(False, n_iterations=0), mk(True, n_iterations=0)
    out = {}
    add = lambda key, v: out.setdefault(key, []).append(v)                                               # noqa: E731
    for i in range(len(S)):
        for e in (o, o32, z, z32):
            oracle_substep(e, S[i], T[i], None if M is None else M[i], mu)
        C, C32 = o.last_contacts_full(), o32.last_contacts_full()
        if len(C) == len(C32) and np.array_equal(C[:, 4:6], C32[:, 4:6]):
            for c, c32 in zip(C, C32):
                add("A P", relerr(c32[0:3], c[0:3]))
                add("A dist", abs(c32[3] - c[3]) / max(abs(c[3]), 1e-3))      # (a depth: relative to a millimetre at least)
                add("A normal", relerr(c32[6:9], c[6:9]))
        nd = 6 + n
        vf = lambda e: np.concatenate([e.get_state()[7:13], e.get_state()[13 + n:]])                      # noqa: E731
        add("B v_free", relerr(vf(z32), vf(z)))
        for e in (z, z32):                       # M^-1 at the pose the substep started from
            e.set_state(np.asarray(S[i], np.float32).astype(np.float64))
        Mi, Mi32 = (np.array([e.minv_mul(np.eye(nd)[j]) for j in range(nd)]) for e in (z, z32))
        for j in range(nd):
            add("C M^-1", relerr(Mi32[j], Mi[j]))
        for kind in ("normals", "frictions"):
            a, b = o.last_rows(kind), o32.last_rows(kind)
            if len(a["dinv"]) != len(b["dinv"]):
                continue
            for k in range(len(a["dinv"])):
                if a["dinv"][k] == 0 or b["dinv"][k] == 0:
                    continue
                add("D %s J/den" % kind, relerr(b["J"][k] * b["dinv"][k], a["J"][k] * a["dinv"][k]))
                add("D %s M^-1 J^T" % kind, relerr(b["M"][k], a["M"][k]))
                add("D %s den" % kind, abs(a["dinv"][k] / b["dinv"][k] - 1))
                add("D %s rhs" % kind, abs(b["rhs"][k] - a["rhs"][k]) / max(abs(a["rhs"][k]), 1e-3 * a["dinv"][k]))
        rows, nonc = oracle_rows_for_replay(o)
        r32 = lambda d: {k: (np.asarray(v, np.float32) if np.asarray(v).dtype.kind == "f" else v) if not isinstance(v, dict)  # noqa: E731
                         else r32(v) for k, v in d.items()}
        rows, nonc = r32(rows), r32(nonc)
        mus = np.array([min(o.params.mu_link ** 2, 10.0) if lb >= 0 else
                        (min(o.params.mu_link * o.params.mu_obstacle, 10.0) if lb == -2 else min(o.params.mu_link * mu, 10.0))
                        for lb in C[:, 5].astype(int)])
        for k in sweeps:
            a = nr.replay(rows, nonc, mus, o.params, k, np.float64, thr=-1.0)
            b = nr.replay(rows, nonc, mus, o.params, k, np.float32, thr=-1.0)
            for q in ("dv", "normal", "motor"):
                add("E%d %s" % (k, q), relerr(b[q], a[q]))
    return out


def test_yardstick_table(oracle_mod, sets):
    lines = ["float32 oracle against the float64 oracle, |x - ref|_inf / |ref|_inf per row or vector (stage E: float32 replay",
             "against float64 replay on the float64 oracle's rows rounded to float32): count, median, p90, worst", ""]
    for name, n, S, T, over, M in sets:
        lines.append("[%s] %d states" % (name, len(S)))
        for key, v in sorted(oracle_stage_errors(oracle_mod, n, S, T, over, M).items()):
            med, p90, mx = summary(v)
            lines.append("  %-28s %5d  %.3e  %.3e  %.3e" % (key, len(v), med, p90, mx))
            assert np.isfinite(mx), (name, key)
    text = "\n".join(lines) + "\n"
    print(text)
    if os.environ.get("SNK_WRITE_PROFILES"):
        with open(os.path.join(ROOT, "profiles", "r15_rows_yardstick.txt"), "w") as f:
            f.write(text)
