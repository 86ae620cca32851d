"""The HIP kernels' contact-cache update (manifold_core / manifold_sort_cached at their call sites in find_contacts_v2
and find_contacts_manifold_v1, and the free box's copy in find_box_ground_v1) against tests/np_manifold.py, the float64
numpy model written from the rules.

One update per case, teacher-forced: Stepper.set_state(S32), set_manifold(M32), substep(T, 1), then get_manifold() and
info[:, 1]; the model runs on the same float32-representable state and cache.  `a` and `b` of the returned cache do not
depend on the solve; `lam` is not compared here.  Paths as in tests/test_gpu_np_substep.py (register-resident,
SNK_FORCE_STREAMED, 32 links), self_collision 0; switch sets np_manifold.SWITCH_SETS; the case families of
tests/test_np_manifold.py (the model's answers are computed once per process and shared between the paths).

On retained cases (np_manifold.MARGIN_BOUND, chosen on the CPU) counts, slot order and info[:, 1] equal the model's:
no flip allowance.  Values go through conftest.f32_gate against the float32 oracle's distance to the model on the same
cases: 1.5 x for medians, 2 x for worst values and for 32 links.  The floors are np_manifold.F32_FLOOR: the float32
oracle's own figures, the MAXIMUM over the families of a chain length, as tests/test_np_manifold.py measures and asserts
them on the CPU (m): 16 links median 3.8e-8, worst 5.1e-7; 32 links median 8.7e-8, worst 1.1e-6; the box median 3.8e-8,
worst 1.2e-7.  A family whose own float32 figure is smaller is held to factor x that figure or the floor, whichever is
larger; no floor exceeds factor x the smallest family figure it stands in for (16 links: 1.5 x 2.6e-8 median, 2 x
2.8e-7 worst), so the floors loosen no family's gate."""
import numpy as np
import pytest

import np_manifold as nm
from conftest import f32_gate

pytestmark = pytest.mark.gpu

PATHS = [("register-resident", 16, False), ("streamed-row", 16, True), ("32 links", 32, False)]
FLOOR = nm.F32_FLOOR


def _path(monkeypatch, path):
    _, n, streamed = next(p for p in PATHS if p[0] == path)
    if streamed:
        monkeypatch.setenv("SNK_FORCE_STREAMED", "1")
    return n, streamed


def _launch_all(pkg, ref, n, over):
    """Every launch of a family on one handle: (caches per launch [B, 2n, 29], info[:, 1] per launch, overflow)."""
    B = len(ref["launches"][0]["S"])
    st = pkg.Stepper(B, n_modules=n, self_collision=0, **over)
    T = np.zeros((B, n), np.float32)
    caches, counts = [], []
    for L in ref["launches"]:
        st.set_state(np.asarray(L["S"], np.float32))
        st.set_manifold(np.asarray(L["M"], np.float32))
        info = st.substep(T, 1)
        caches.append(st.get_manifold().astype(np.float64))
        counts.append(info[:, 1].copy())
    ovf = st.contact_overflow()
    st.close()
    return caches, counts, ovf


@pytest.mark.parametrize("family", ["synth", "trajectory"])
@pytest.mark.parametrize("switch", list(nm.SWITCH_SETS))
@pytest.mark.parametrize("path", [p[0] for p in PATHS])
def test_link_caches_against_the_model(pkg, oracle_mod, monkeypatch, path, switch, family):
    n, streamed = _path(monkeypatch, path)
    ref = nm.reference(switch, n, family)
    caches, counts, ovf = _launch_all(pkg, ref, n, nm.SWITCH_SETS[switch])
    total = sum(len(r["margin"]) for L in ref["launches"] for r in L["res"])
    left = sum(int((~nm.retained(r)).sum()) for L in ref["launches"] for r in L["res"])
    assert left <= nm.MAX_LEFT_OUT * total
    dist, bad = nm.cache_distances(ref, caches)
    for k, e, c in bad[:8]:
        r = ref["launches"][k]["res"][e]
        print("  DISAGREES launch %d env %d cylinder %d margin %.2e %s\n    GPU   %s\n    model %s"
              % (k, e, c, r["margin"][c], r["events"][c], caches[k][e][c], r["M"][c]))
    whole = over64 = maybe64 = 0
    for k, L in enumerate(ref["launches"]):
        for e, r in enumerate(L["res"]):
            assert counts[k][e] == caches[k][e][:, 0].sum(), (k, e)          # info[:, 1] is what the cache holds
            if nm.retained(r).all():
                whole += 1
                assert counts[k][e] == len(r["contacts"]), (k, e, counts[k][e], len(r["contacts"]))
                over64 += len(r["contacts"]) > 64
            else:                      # a left-out cylinder may hold any count, up to four away from the model's
                amb = 4 * int((~nm.retained(r)).sum())
                over64 += len(r["contacts"]) - amb > 64
                maybe64 += len(r["contacts"]) - amb <= 64 < len(r["contacts"]) + amb
    print("  %s, %s, %s: %d cylinder cases, %d left out, %d whole environments, %d environments beyond 64 points, overflow %s"
          % (path, switch, family, total, left, whole, over64, ovf))
    assert not bad, (len(bad), bad[:8])
    assert whole > 0
    if family == "synth" and n == 16:
        assert over64 >= 4                     # the model's full count came back (asserted above), beyond the 64 slots
    if n == 16 and not streamed:
        # a register-resident handle counts the substeps it hands to the streamed-row solve, and leaves no point out:
        # the MODEL's environments beyond 64 points (exactly that many when no cylinder of the family is left out)
        assert left > 0 or maybe64 == 0
        assert over64 <= ovf[0] <= over64 + maybe64 and ovf[1:] == (0, 0), (ovf, over64, maybe64)
    else:
        assert ovf == (0, 0, 0), ovf
    d32, bad32 = nm.cache_distances(ref, [np.array([m for m, _, _ in row]) for row in
                                          nm.oracle_answers(switch, n, family, True)])
    assert not bad32
    fm, fw = (1.5, 2.0) if n == 16 else (2.0, 2.0)
    name = "np manifold %s, %s, %s" % (path, switch, family)
    f32_gate(name + ": median of %d" % len(dist), np.median(dist), np.median(d32), fm, FLOOR[n][0])
    f32_gate(name + ": worst", dist.max(), d32.max(), fw, FLOOR[n][1])


@pytest.mark.parametrize("switch", ["default", "hull+manifold@0.02"])
def test_box_cache_against_the_model(pkg, oracle_mod, switch):
    """obstacle 2 (16 links, the streamed-row kernels): the copied update of find_box_ground_v1, through set_box /
    get_box; the snake hangs in the air, the box's points are the substep's only contacts."""
    ref = nm.box_reference(switch)
    B = len(ref["S"])
    over = dict(nm.SWITCH_SETS[switch], obstacle=2, self_collision=0)
    S = np.zeros((B, 13 + 2 * 16), np.float32)
    S[:, 2], S[:, 6] = 1.0, 1.0
    st = pkg.Stepper(B, **over)
    st.set_state(S)
    st.set_box(np.asarray(ref["S"], np.float32), np.asarray(ref["M"], np.float32))
    info = st.substep(np.zeros((B, 16), np.float32), 1)
    _, G = st.get_box()
    ovf = st.contact_overflow()
    st.close()
    o32 = oracle_mod.OracleEnv(f32=True, max_contacts=0, **over)
    dist, d32, left = [], [], 0
    for e, r in enumerate(ref["res"]):
        if r["margin"] < nm.MARGIN_BOUND:
            left += 1
            continue
        assert nm.same_structure(G[e].astype(np.float64), r["cache"]), (e, r["margin"], r["events"], G[e], r["cache"])
        assert info[e, 1] == int(r["cache"][0]), (e, info[e], r["cache"][0])
        o32.hard_reset()
        o32.set_state(S[0].astype(np.float64))
        o32.set_box(ref["S"][e], ref["M"][e])
        o32.substep(np.zeros(16))
        for M, lst in ((G[e].astype(np.float64), dist), (o32.get_box()[1], d32)):
            d = nm.cache_distance(M, r["cache"])
            if not np.isnan(d):
                lst.append(d)
    assert left <= nm.MAX_LEFT_OUT * B and ovf == (0, 0, 0)
    f32_gate("np manifold box %s: median of %d" % (switch, len(dist)), np.median(dist), np.median(d32), 1.5, FLOOR["box"][0])
    f32_gate("np manifold box %s: worst" % switch, np.max(dist), np.max(d32), 2.0, FLOOR["box"][1])


@pytest.mark.parametrize("path", [p[0] for p in PATHS])
@pytest.mark.parametrize("name", ["ROUND1", "hull"])
def test_stateless_counts_against_the_model(pkg, monkeypatch, path, name):
    """contact_model 0 handles: the count per environment against two rim points per cylinder, active below the
    threshold; environments with a decision below the margin bound are left out."""
    n, _ = _path(monkeypatch, path)
    ref = nm.stateless_reference(name, n)
    B = len(ref["S"])
    st = pkg.Stepper(B, n_modules=n, self_collision=0, **ref["over"])
    st.set_state(np.asarray(ref["S"], np.float32))
    info = st.substep(np.zeros((B, n), np.float32), 1)
    st.close()
    left = sum(int((mg < nm.MARGIN_BOUND).sum()) for _, mg in ref["res"])
    assert left <= nm.MAX_LEFT_OUT * 2 * n * B
    seen = 0
    for e, (act, mg) in enumerate(ref["res"]):
        if (mg >= nm.MARGIN_BOUND).all():
            assert info[e, 1] == act.sum(), (name, path, e, info[e], act.sum())
            seen += act.sum()
    assert seen > 2 * n
