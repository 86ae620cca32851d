"""The oracle's contact-cache update (find_contacts_manifold and the free box's copy) against tests/np_manifold.py, the
float64 numpy model written from the rules -- on the CPU, with the case families tests/test_gpu_np_manifold.py runs on
the kernels.

One update per case, teacher-forced: set_manifold / set_state / substep, then get_manifold, last_contacts_full and
last_num_contacts.  On every retained cylinder case (smallest decision margin >= np_manifold.MARGIN_BOUND) the count
and the slot order must equal the model's; at most np_manifold.MAX_LEFT_OUT of a family's cylinder cases may be left
out.  A retained case that disagrees is a failure.

Values, float64 oracle: TOL = 1e-10 m.  Round-off of float64 (1.1e-16) on coordinates up to 2.5 m through a chain of
up to 98 link frames is ~1e-13 (measured here: 2.2e-15 at worst); 1e-10 leaves room for constants rounded differently
in the two programs, as the sweep-ladder file allows for the same kind of agreement, and is four orders below the
float32 figures it must not be confused with (~1e-6).
Float32 oracle: structure only; its distance to the model is printed -- the yardstick of the GPU file."""
import functools

import numpy as np
import pytest

import np_manifold as nm

TOL = 1e-10

FAMILIES = [(sw, n, fam) for sw in nm.SWITCH_SETS for n in (16, 32) for fam in ("synth", "trajectory")]


def compare(ref, got, n, what, tol=None):
    """Structure on retained cylinder cases (asserted), values (asserted with tol, else returned).  Returns (left-out
    share, distances of the retained caches that hold points, contact-list distances)."""
    left = total = 0
    dist, cdist = [], []
    for L, row in zip(ref["launches"], got):
        for e, (M, C, nc) in enumerate(row):
            r = L["res"][e]
            keep = nm.retained(r)
            total += len(keep)
            left += int((~keep).sum())
            for c in np.nonzero(keep)[0]:
                assert nm.same_structure(M[c], r["M"][c]), (what, "env", e, "cylinder", c, "margin", r["margin"][c],
                                                             r["events"][c], M[c], r["M"][c])
                d = nm.cache_distance(M[c], r["M"][c])
                if not np.isnan(d):
                    dist.append(d)
            if keep.all():
                assert nc == len(C) == len(r["contacts"]), (what, e, nc, len(r["contacts"]))
                if nc:
                    assert np.array_equal(C[:, 4], r["contacts"][:, 4]), (what, e)            # link by link, in order
                    assert np.all(C[:, 5] == -1)
                    cdist.append(np.abs(C[:, :4] - r["contacts"][:, :4]).max())
    dist, cdist = np.array(dist), np.array(cdist)
    if tol is not None:
        assert dist.max() < tol and cdist.max() < tol, (what, dist.max(), cdist.max())
    return left / total, dist, cdist


@pytest.mark.parametrize("switch,n,family", FAMILIES)
def test_link_caches_against_the_model(oracle_mod, switch, n, family):
    ref = nm.reference(switch, n, family)
    share, d64, c64 = compare(ref, nm.oracle_answers(switch, n, family, False), n, "float64 oracle", TOL)
    _, d32, c32 = compare(ref, nm.oracle_answers(switch, n, family, True), n, "float32 oracle")
    cov = nm.coverage([e for L in ref["launches"] for r in L["res"] for e in r["events"]])
    print("  %s n %d %s: %d cached sets compared, left out %.2f %% | float64 oracle worst %.1e (list %.1e) | float32 "
          "oracle median %.2e worst %.2e (list %.2e)" % (switch, n, family, len(d64), 100 * share, d64.max(), c64.max(),
                                                         np.median(d32), d32.max(), c32.max()))
    print("  reached:", cov)
    assert share <= nm.MAX_LEFT_OUT
    assert cov["drop_slots"] >= {"first", "middle", "last"} and cov["double_drops"] > 0
    assert min(cov["actions"][a] for a in ("none", "replace", "append")) > 0
    if family == "synth":
        # full caches with a far new point: drawn for a fifth of the cylinders, a tenth must get there
        assert cov["evict_share"] >= 0.10
        assert cov["evicted"] == {0, 1, 2, 3}
        assert cov["deepest_cached"] > 0 and cov["deepest_new"] > 0 and cov["exception_decided"] > 0
        over64 = sum(len(r["contacts"]) > 64 for r in ref["launches"][0]["res"])
        assert n == 32 or over64 >= 4
    else:
        # trajectories evict at the relative threshold (1.2 mm) only; at 0.02 m a rolling cylinder's next support
        # vertex always replaces (np_manifold.trajectory says why) -- eviction is the synthesised families' business
        print("  trajectory evictions: %d of %d cylinder cases" % (cov["actions"]["evict"], sum(cov["actions"].values())))
        assert cov["actions"]["evict"] > 0 or switch != "default"


@functools.lru_cache(maxsize=None)
def _box_oracle(oracle_mod, switch, f32):
    """The oracle's update of every box case: structure asserted on retained cases; (left-out share, distances)."""
    ref = nm.box_reference(switch)
    B = len(ref["S"])
    o = oracle_mod.OracleEnv(f32=f32, obstacle=2, self_collision=0, max_contacts=0, **nm.SWITCH_SETS[switch])
    s0 = np.zeros(13 + 2 * 16)
    s0[2], s0[6] = 1.0, 1.0                                         # the snake in the air: the box alone touches down
    left, dist = 0, []
    for e in range(B):
        o.hard_reset()
        o.set_state(s0)
        o.set_box(ref["S"][e], ref["M"][e])
        o.substep(np.zeros(16))
        _, M = o.get_box()
        r = ref["res"][e]
        if r["margin"] < nm.MARGIN_BOUND:
            left += 1
            continue
        assert nm.same_structure(M, r["cache"]), ("float32" if f32 else "float64", e, r["margin"], r["events"], M, r["cache"])
        assert o.last_num_contacts == int(r["cache"][0])
        d = nm.cache_distance(M, r["cache"])
        if not np.isnan(d):
            dist.append(d)
    return left / B, np.array(dist)


@pytest.mark.parametrize("switch", ["default", "hull+manifold@0.02"])
def test_box_cache_against_the_model(oracle_mod, switch):
    ref = nm.box_reference(switch)
    stats = {f32: _box_oracle(oracle_mod, switch, f32) for f32 in (False, True)}
    assert max(stats[f32][0] for f32 in stats) <= nm.MAX_LEFT_OUT
    assert stats[False][1].max() < TOL
    cov = nm.coverage([r["events"] for r in ref["res"]])
    print("  box %s: left out %.1f %% | float64 oracle worst %.1e | float32 oracle median %.2e worst %.2e"
          % (switch, 100 * stats[False][0], stats[False][1].max(), np.median(stats[True][1]), stats[True][1].max()))
    print("  reached:", cov)
    assert cov["evicted"] == {0, 1, 2, 3} and cov["drop_slots"] >= {"first", "middle", "last"} and cov["double_drops"] > 0
    assert min(cov["actions"].values()) > 0


def test_float32_floors_are_the_measured_maxima(oracle_mod):
    """np_manifold.F32_FLOOR, the floors of the GPU file's gates, against what the float32 oracle gives here: the
    maximum over the families, to the two digits they are written with (5 %).  A change of the generators that moves
    them fails here, on the CPU, before a GPU run uses a stale figure."""
    got = {}
    for n in (16, 32):
        d = [compare(nm.reference(sw, n, fam), nm.oracle_answers(sw, n, fam, True), n, "float32 oracle")[1]
             for sw, m, fam in FAMILIES if m == n]
        got[n] = (max(np.median(x) for x in d), max(x.max() for x in d))
    d = [_box_oracle(oracle_mod, sw, True)[1] for sw in ("default", "hull+manifold@0.02")]
    got["box"] = (max(np.median(x) for x in d), max(x.max() for x in d))
    for k, floor in nm.F32_FLOOR.items():
        print("  float32 oracle, %s: median %.3e worst %.3e | floors %.1e %.1e" % ((k,) + got[k] + floor))
        assert np.allclose(got[k], floor, rtol=0.05, atol=0), (k, got[k], floor)


@pytest.mark.parametrize("name,n", [("ROUND1", 16), ("hull", 16), ("hull", 32)])
def test_stateless_counts_against_the_model(oracle_mod, name, n):
    """contact_model 0: two rim points per cylinder, active below the threshold -- counts per environment."""
    ref = nm.stateless_reference(name, n)
    left = sum(int((mg < nm.MARGIN_BOUND).sum()) for _, mg in ref["res"])
    assert left <= nm.MAX_LEFT_OUT * 2 * n * len(ref["S"])
    for f32 in (False, True):
        o = oracle_mod.OracleEnv(f32=f32, n_modules=n, self_collision=0, max_contacts=0, **ref["over"])
        seen = 0
        for e, (act, mg) in enumerate(ref["res"]):
            if (mg < nm.MARGIN_BOUND).any():
                continue
            o.hard_reset()
            o.set_state(ref["S"][e])
            o.substep(np.zeros(n))
            assert o.last_num_contacts == act.sum(), (name, n, f32, e)
            seen += act.sum()
        assert seen > 2 * n
