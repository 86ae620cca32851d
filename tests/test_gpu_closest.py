"""GPU tests of the closest-point query (snk_closest_points; include/snk.h, "The closest points"): the solver's narrow phase
run at a caller-given distance, on tensors.

The float64 yardstick is OracleEnv.contacts_full() (for a distance D other than the handle's breaking threshold the
oracle is built with that threshold and room for every pair: np_closest.oracle_overrides).  States are kept as
box_states.select_for_float32 keeps them: the float64 and float32 oracles list the same pairs and no float64 distance lies
within 1e-5 m of D.  On kept states the pair list, its order, the counts and the slot positions must equal the oracle's
exactly; distances and normals of tier-0 records go through conftest.f32_gate (median 1.5, 90th percentile 2.0, the
32-link chain 2.0; floor 1e-6: float32 ulp at coordinates up to a metre is about 1e-7 and several such terms are
combined); witness points are not unique for parallel faces and are judged through the certificate of
tests/np_closest.py alone (the same gate against the float32 oracle's records; membership capped at 1e-5)."""
import ctypes as C

import numpy as np
import pytest

import np_closest as ncl
from conftest import f32_gate, random_state

gpu = pytest.mark.gpu
BOX, LINKS = 1, 2


def threshold(st):
    out = (C.c_double * 6)()
    assert st.lib.snk_params_derived(C.byref(st.params), out) == 0
    return float(np.float32(out[0]))


_refs = {}


def reference(oracle_mod, n, sides, D, boxpos, S, obstacle=1, BS=None):
    """Per state of S: None (not kept) or (box rows, link rows) of the float64 oracle and of the float32 oracle; D None =
    the default threshold."""
    key = (n, sides, D, tuple(boxpos), obstacle, S.tobytes(), None if BS is None else BS.tobytes())
    if key in _refs:
        return _refs[key]
    over = dict(n_modules=n, hull_sides=sides, obstacle=obstacle, obstacle_pos=list(boxpos), **ncl.oracle_overrides(D))
    o, o32 = oracle_mod.OracleEnv(**over), oracle_mod.OracleEnv(f32=True, **over)
    import np_manifold as nm
    thr = nm.link_threshold(o.params) if D is None else D
    out = []
    for i, s in enumerate(S):
        b = None if BS is None else BS[i]
        r64, r32 = ncl.oracle_pairs(o, s, b), ncl.oracle_pairs(o32, s, b)
        same = all(len(x) == len(y) and np.array_equal(x[:, 4:6], y[:, 4:6]) for x, y in zip(r64, r32))
        near = any((np.abs(x[:, 3] - thr) < 1e-5).any() for x in r64)
        out.append((r64, r32) if same and not near else None)
    _refs[key] = (out, o.params)
    return _refs[key]


def f32r(a):
    return np.asarray(a, np.float32).astype(np.float64)


def check_against_oracle(what, pts, cnt, refs, params, n, sides, S, pool, BS=None, want_tiers=()):
    """The exact part and the gated part of checks 1 and 2 for one handle's answer."""
    nc = 2 * n
    m = float(params.collision_margin)
    kept = [i for i, r in enumerate(refs) if r is not None]
    print("%s: kept %d of %d states" % (what, len(kept), len(refs)))
    assert 4 * len(kept) >= 3 * len(refs)
    dev = {"gpu": {"dist": [], "normal": [], "cert": [], "member": []}, "f32": {"dist": [], "normal": [], "cert": [], "member": []}}
    tiers = {0: 0, 1: 0, 2: 0}
    for i in kept:
        (bx, lk), (bx32, lk32) = refs[i]
        P = pts[i].astype(np.float64)
        # exact: the live box slots, the compact link slots in the oracle's order, the counts, zeros elsewhere
        live_box = [c for c in range(nc) if P[c, 14] != 0.0]
        assert live_box == [int(a) for a in bx[:, 4]], (what, i, live_box, bx[:, 4])
        assert tuple(cnt[i]) == (len(bx), len(lk)), (what, i, cnt[i], len(bx), len(lk))
        L = P[nc:nc + len(lk)]
        assert np.array_equal(L[:, 12:14], lk[:, 4:6]) and (L[:, 14] == 1.0).all(), (what, i)
        assert not P[nc + len(lk):].any() and not P[[c for c in range(nc) if c not in live_box]].any()
        for c in live_box:
            assert P[c, 12] == c and P[c, 13] == nc and P[c, 11] == 0.0 and P[c, 15] == 0.0
        cyl, box = ncl.cores(n, S[i], sides, ncl.box_frame(params, None if BS is None else BS[i]), m)
        G = np.concatenate([P[live_box], L])
        R64, R32 = np.concatenate([bx, lk]), np.concatenate([bx32, lk32])
        for g, r, r32 in zip(G, R64, R32):
            t = int(g[10])
            tiers[t] += 1
            a, b = int(g[12]), int(g[13])
            A, B = cyl[a], (box if b == nc else cyl[b])
            assert g[9] > -2 * m - 1e-6 or t > 0, (what, "a tier-0 record deeper than both margins", g)
            assert t == 0 or not ncl.surely_tier0(r[3], m), (what, "tier", t, "at a distance only tier 0 gives", g, r)
            if t == 0:
                for who, x in (("gpu", (g[0:3], g[3:6], g[6:9], g[9])), ("f32", (r32[0:3], r32[9:12], r32[6:9], r32[3]))):
                    dev[who]["dist"].append(abs(x[3] - r[3]))
                    dev[who]["normal"].append(np.abs(x[2] - r[6:9]).max())
                    res = ncl.certificate(A, B, x[0], x[1], x[2], x[3], m)
                    dev[who]["cert"].append(max(res.values()))
                    dev[who]["member"].append(max(res["member_a"], res["member_b"]))
            elif t == 1:
                # n = (pa - pb) / d with d the length of the simplex' closest point: the witness points are sums of up to
                # three weighted vertices at coordinates up to a metre (float32 ulp 6e-8), so pa - pb carries up to
                # 8 x 6e-8 m of round-off whatever d is, and |n| - 1 is that over the shrunk cores' distance d
                d_core = max(g[9] + 2 * (m + ncl.SHRINK), 1e-9)
                assert abs(np.linalg.norm(g[6:9]) - 1.0) < max(1e-6, 8 * 6e-8 / d_core), (g, d_core)
                assert np.abs(g[0:3] - g[3:6] - g[6:9] * g[9]).max() < 1e-6, g
            if t == 2:
                d = A.c - B.c
                want_p = A.c if b == nc else 0.5 * (A.c + B.c)
                assert np.abs(g[6:9] - d / np.linalg.norm(d)).max() < 1e-6 and abs(g[9] + 2 * (m + ncl.SHRINK)) < 1e-6, g
                assert np.abs(g[0:3] - want_p).max() < 1e-6 and np.array_equal(g[0:3], g[3:6]), g
    print("%s: records by tier %s" % (what, tiers))
    for t in want_tiers:
        assert tiers[t] > 0, (what, "no tier-%d record in this family" % t)
    for who in dev:
        for k in dev[who]:
            pool[who][k] += dev[who][k]
    return tiers


def new_pool():
    return {who: {"dist": [], "normal": [], "cert": [], "member": []} for who in ("gpu", "f32")}


def gate(what, pool, factor):
    """The gated part: the deviations of one configuration's tier-0 records, pooled over its distances and box placements.
    (A percentile needs a sample: at the handle's own threshold, 1.2 mm, a placement has one or two tier-0 records, and the
    ratio of two single float32 round-offs is bounded by nothing.)"""
    assert len(pool["gpu"]["dist"]) >= 30, (what, len(pool["gpu"]["dist"]))
    for k in ("dist", "normal", "cert"):
        g, f = np.array(pool["gpu"][k]), np.array(pool["f32"][k])
        print("%s: %s over %d records, worst GPU %.3e, float32 oracle %.3e (not gated)" % (what, k, len(g), g.max(), f.max()))
        f32_gate("%s %s median" % (what, k), np.median(g), np.median(f), factor, 1e-6)
        f32_gate("%s %s p90" % (what, k), np.percentile(g, 90), np.percentile(f, 90), 2.0, 1e-6)
    assert max(pool["gpu"]["member"]) < 1e-5, (what, max(pool["gpu"]["member"]))


def family_states(n):
    return np.concatenate([ncl.family(n, 8, seed=900 + n), ncl.family(n, 4, seed=950 + n)])


# 1, 2. pair list, distances and the certificate against the oracle
@gpu
@pytest.mark.parametrize("n,sides,Ds", [(16, 32, (None, 0.05)), (16, 0, (None, 0.05)), (32, 32, (None, 0.05, 0.5))])
def test_pairs_and_distances_match_the_oracle(pkg, oracle_mod, n, sides, Ds):
    """Exact per state: pair list, order, counts, slots, tiers 1 and 2.  Gated per configuration: distance, normal and
    certificate residual of the tier-0 records.
    The implicit cylinders (hull_sides 0) are why the query runs their GJK further than the solver does (snk_world.hpp:
    gjk_distance_fine): with the solver's termination, a duality gap of 1e-5 against the float32 oracle's 1e-6, the
    normals' 90th percentile was 4.0e-4 against the oracle's 1.6e-4 (ratio 2.52 over 632 records); now 1.8e-4 (1.16)."""
    S = family_states(n)
    tiers = {0: 0, 1: 0, 2: 0}
    pool = new_pool()
    for D in Ds:
        for pos, sl in ((ncl.BOX_FAR, slice(0, 8)), (ncl.BOX_NEAR, slice(8, 12))):
            if D == 0.5 and pos is ncl.BOX_NEAR:
                continue                                   # (the one D = 0.5 case: the eight states beside the box)
            Sx = S[sl]
            st = pkg.Stepper(len(Sx), n_modules=n, hull_sides=sides, obstacle=1, obstacle_pos=list(pos))
            st.set_state(Sx.astype(np.float32))
            assert st.link_pairs == {16: 465, 32: 1953}[n] and st.closest_slots(7) == 2 * n + 7
            dist = threshold(st) if D is None else D
            pts, clr, cnt = st.closest_points(dist)        # max_pairs = all
            refs, params = reference(oracle_mod, n, sides, D, pos, Sx)
            t = check_against_oracle("n %d sides %d D %s box %s" % (n, sides, D, pos), pts, cnt, refs, params, n, sides, Sx, pool)
            for k in t:
                tiers[k] += t[k]
            st.close()
    assert tiers[1] > 0 and tiers[2] > 0, "the box on the snake's head gave no deep pair"
    gate("n %d sides %d" % (n, sides), pool, 2.0 if n == 32 else 1.5)


# 3. the free box
@gpu
def test_free_box(pkg, oracle_mod):
    import box_states
    over = dict(box_states.FREE_BOX)
    S, _, _, BS, _ = box_states.beside_link(oracle_mod, np.random.default_rng(31), 4, over)
    S, BS = f32r(S), f32r(BS)
    st = pkg.Stepper(4, n_modules=16, **over)
    st.set_box(BS.astype(np.float32), np.zeros((4, 29), np.float32))
    st.set_state(S.astype(np.float32))
    pool = new_pool()
    for D in (None, 0.05):
        pts, clr, cnt = st.closest_points(threshold(st) if D is None else D)
        refs, params = reference(oracle_mod, 16, 32, D, over["obstacle_pos"], S, obstacle=2, BS=BS)
        check_against_oracle("free box D %s" % D, pts, cnt, refs, params, 16, 32, S, pool, BS=BS)
        assert cnt[:, 0].sum() > 0
    st.close()
    gate("free box", pool, 1.5)


# 4. the folded snake
@gpu
def test_folded_snake(pkg, oracle_mod):
    """The 16-link folded family of test_gpu_self_collision.py (test_sixteen_links_folded_onto_themselves builds it inline:
    the same generator and seed here, its first 48 states): at the handle's threshold the live link-link list is the
    oracle's default contacts_full() pair rows."""
    B, n = 48, 16
    rng = np.random.default_rng(4321)
    S = np.zeros((B, 13 + 2 * n), np.float32)
    for i in range(B):
        s = random_state(rng, n, z=0.026, qamp=1.7, vamp=0.3, flat=True)
        s[9] *= 0.1; s[7:9] *= 0.1
        S[i] = s
    st = pkg.Stepper(B)
    st.set_state(S)
    pts, clr, cnt = st.closest_points(threshold(st), flags=LINKS)
    st.close()
    o = oracle_mod.OracleEnv(max_contacts=0, max_self_contacts=4096)
    o32 = oracle_mod.OracleEnv(max_contacts=0, max_self_contacts=4096, f32=True)
    import np_manifold as nm
    thr = nm.link_threshold(o.params)
    kept = touching = 0
    for i in range(B):
        _, lk = ncl.oracle_pairs(o, S[i].astype(np.float64))
        _, lk32 = ncl.oracle_pairs(o32, S[i].astype(np.float64))
        if len(lk) != len(lk32) or not np.array_equal(lk[:, 4:6], lk32[:, 4:6]) or (np.abs(lk[:, 3] - thr) < 1e-5).any():
            continue
        kept += 1
        touching += len(lk) > 0
        L = pts[i, 2 * n:2 * n + len(lk)]
        assert cnt[i, 1] == len(lk) and cnt[i, 0] == 0 and np.array_equal(L[:, 12:14], lk[:, 4:6]), i
        assert not pts[i, 2 * n + len(lk):].any() and not pts[i, :2 * n].any()
    print("folded snakes: kept", kept, "of", B, "with link-link pairs", touching)
    assert 4 * kept >= 3 * B and touching >= 4


def _crowded(pkg, n=16, E=4, **over):
    """a handle whose envs hold many pairs within 0.05 m"""
    st = pkg.Stepper(E, n_modules=n, obstacle=1, obstacle_pos=list(ncl.BOX_FAR), **over)
    st.set_state(ncl.family(n, E, seed=77).astype(np.float32))
    return st


# 5. clearance
@gpu
def test_clearance(pkg):
    st = _crowded(pkg)
    n, D = 16, 0.05
    pts, clr, cnt = st.closest_points(D)
    assert cnt[:, 1].min() > 3 and cnt[:, 0].sum() > 0
    want = np.full((4, 2, 2 * n), np.float32(D), np.float32)
    for e in range(4):
        for r in pts[e]:
            if r[14] == 0.0:
                continue
            a, b = int(r[12]), int(r[13])
            if b == 2 * n:
                want[e, 0, a] = min(want[e, 0, a], r[9])
            else:
                want[e, 1, a] = min(want[e, 1, a], r[9])
                want[e, 1, b] = min(want[e, 1, b], r[9])
    assert np.array_equal(clr.view(np.int32), want.view(np.int32))
    assert (clr == np.float32(D)).any() and (clr < np.float32(D)).any()
    for mp in (0, 3):
        assert np.array_equal(st.closest_points(D, max_pairs=mp)[1].view(np.int32), clr.view(np.int32))
    only_box = st.closest_points(D, flags=BOX)[1]
    only_links = st.closest_points(D, flags=LINKS)[1]
    assert np.array_equal(only_box[:, 0], clr[:, 0]) and (only_box[:, 1] == np.float32(D)).all()
    assert np.array_equal(only_links[:, 1], clr[:, 1]) and (only_links[:, 0] == np.float32(D)).all()
    st.close()


# 6. truncation and layout
@gpu
def test_truncation_and_layout(pkg):
    st = _crowded(pkg)
    n, D = 16, 0.05
    full, _, cnt = st.closest_points(D)
    three, _, cnt3 = st.closest_points(D, max_pairs=3)
    none, _, cnt0 = st.closest_points(D, max_pairs=0)
    assert full.shape[1] == 2 * n + 465 and three.shape[1] == 2 * n + 3 and none.shape[1] == 2 * n
    assert cnt[:, 1].min() > 3 and np.array_equal(cnt, cnt3) and np.array_equal(cnt, cnt0)
    assert np.array_equal(three.view(np.int32), full[:, :2 * n + 3].view(np.int32))
    assert np.array_equal(none.view(np.int32), full[:, :2 * n].view(np.int32))
    live = full[:, :, 14] != 0.0
    assert not full[~live].any() and (full[live][:, 14] == 1.0).all()
    for e in range(4):
        assert live[e, 2 * n:].sum() == cnt[e, 1] and live[e, 2 * n:2 * n + cnt[e, 1]].all()
    st.close()
    bare = pkg.Stepper(2)                        # no obstacle: the box part is empty, not refused
    bare.set_state(ncl.family(16, 2, seed=77).astype(np.float32))
    p, c, k = bare.closest_points(D)
    assert not p[:, :2 * n].any() and (k[:, 0] == 0).all() and (c[:, 0] == np.float32(D)).all() and k[:, 1].min() > 0
    bare.close()


# 7. ids and independence
@gpu
def test_ids_and_independence(pkg):
    st = _crowded(pkg)
    D = 0.05
    base = st.closest_points(D, max_pairs=40)
    again = st.closest_points(D, max_pairs=40)
    for x, y in zip(base, again):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    ids = [3, 0, 3, 99, -1, 1]
    import torch
    dev = torch.device("cuda", 0)
    w = pkg.DeviceWorld(stepper=st)
    got = [t.cpu().numpy() for t in w.closest_points(D, env_ids=torch.tensor(ids, dtype=torch.int32, device=dev), max_pairs=40)]
    for k, e in enumerate(ids):
        for x, y in zip(got, base):
            if 0 <= e < 4:
                assert np.array_equal(x[k].view(np.int32), y[e].view(np.int32)), (k, e)
            else:
                assert not x[k].any(), (k, e)
    # the row-stride loop: more rows than blocks, clearance alone
    rows = 65536 + 3
    big_ids = (torch.arange(rows, dtype=torch.int32, device=dev) % 4).contiguous()
    out = torch.empty((rows, 2, 32), dtype=torch.float32, device=dev)
    st.closest_points_device(big_ids.data_ptr(), rows, D, 3, 0, clearance_ptr=out.data_ptr(),
                             stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    want = torch.from_numpy(base[1]).to(dev)[big_ids.long()]
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    st.close()


# 8. nothing is written
@gpu
def test_nothing_is_written(pkg):
    import torch
    import box_states
    dev = torch.device("cuda", 0)
    st = pkg.Stepper(4, obstacle=2, obstacle_pos=list(ncl.BOX_FAR))
    S, _, _, BS, _ = box_states.in_the_air(np.random.default_rng(5), 4)
    BS[:, 0:3] = S[:, 0:3] + [0.3, 0.2, 0.0]                  # the box beside the snake's root, both in the air
    st.set_box(BS.astype(np.float32), np.zeros((4, 29), np.float32))
    st.set_state(S.astype(np.float32))
    st.substep(np.zeros((4, 16), np.float32), 2)
    before = (st.get_state(), st.get_manifold(), st.get_box())
    n, mp, fill = 16, 5, 1234.5
    sizes = (4 * (2 * n + mp) * 16, 4 * 2 * 2 * n, 4 * 2)
    bufs = [torch.full((k + 64,), fill, dtype=torch.float32, device=dev) for k in sizes[:2]]
    bufs.append(torch.full((sizes[2] + 64,), 77, dtype=torch.int32, device=dev))
    st.closest_points_device(0, 4, 0.05, 3, mp, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                             torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert (bufs[0][sizes[0]:] == fill).all() and (bufs[1][sizes[1]:] == fill).all() and (bufs[2][sizes[2]:] == 77).all()
    host = st.closest_points(0.05, max_pairs=mp)
    for b, h, k in zip(bufs, host, sizes):
        assert np.array_equal(b[:k].cpu().numpy().view(np.int32), h.reshape(-1).view(np.int32))
    after = (st.get_state(), st.get_manifold(), st.get_box())

    def flat(x):
        return [x] if isinstance(x, np.ndarray) else [z for y in x for z in flat(y)]
    for x, y in zip(flat(before), flat(after)):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    st.close()


# 9. stream order
@gpu
def test_stream_order(pkg):
    import torch
    dev = torch.device("cuda", 0)
    w = pkg.DeviceWorld(4, n_modules=16, obstacle=1, obstacle_pos=list(ncl.BOX_FAR))
    w.stepper.set_state(ncl.family(16, 4, seed=11).astype(np.float32))
    targets = torch.zeros((4, 16), dtype=torch.float32, device=dev)
    w.step_simulation(targets, 3)
    got = w.closest_points(0.05, max_pairs=30)
    clr = w.clearance(0.05)
    torch.cuda.synchronize(dev)
    want = w.stepper.closest_points(0.05, max_pairs=30)
    for g, h in zip(got, want):
        assert np.array_equal(g.cpu().numpy().view(np.int32), h.view(np.int32))
    assert np.array_equal(clr.cpu().numpy().view(np.int32), want[1].view(np.int32))
    assert want[2][:, 1].min() > 0
    w.close()


# 10. refusals
@gpu
def test_refusals(pkg):
    import torch
    dev = torch.device("cuda", 0)
    st = pkg.Stepper(4, obstacle=1)
    buf = torch.zeros(4 * (32 + 465) * 16 + 4, dtype=torch.float32, device=dev)
    p = buf.data_ptr()

    def refused(msg, *a, **k):
        with pytest.raises(RuntimeError, match=msg):
            st.closest_points_device(*a, **k)
    refused("n_rows must be at least 1", 0, 0, 0.05, 3, 0, p)
    refused("distance must be finite and not negative", 0, 4, float("nan"), 3, 0, p)
    refused("distance must be finite and not negative", 0, 4, float("inf"), 3, 0, p)
    refused("distance must be finite and not negative", 0, 4, -0.01, 3, 0, p)
    refused("flags must be", 0, 4, 0.05, 0, 0, p)
    refused("flags must be", 0, 4, 0.05, 4, 0, p)
    refused("max_pairs -1 is outside 0 .. 465", 0, 4, 0.05, 3, -1, p)
    refused("max_pairs 466 is outside 0 .. 465", 0, 4, 0.05, 3, 466, p)
    refused("points, clearance and count are all null", 0, 4, 0.05, 3, 0)
    refused("points_dev must be 16-byte aligned", 0, 4, 0.05, 3, 0, p + 4)
    with pytest.raises(RuntimeError, match="max_pairs 466 is outside"):
        st.closest_slots(466)
    for bad, msg in ((dict(distance=-1.0), "distance must be finite"), (dict(distance=0.05, flags=8), "flags must be"),
                     (dict(distance=0.05, max_pairs=500), "max_pairs 500 is outside"),
                     (dict(distance=0.05, env_ids=[0, 4]), r"env_ids\[1\] = 4 is outside 0 .. 3"),
                     (dict(distance=0.05, env_ids=[]), "n_rows must be at least 1")):
        with pytest.raises(RuntimeError, match=msg):
            st.closest_points(**bad)
    cnt = (C.c_int32 * 16)()
    assert st.lib.snk_closest_points_host(st.h, None, 5, 0.05, 3, 0, None, None, cnt) != 0
    assert "n_rows 5 without env_ids is more than the handle's 4 envs" in pkg._lib.last_error()
    st.debug_raise_alarm()
    for call in (lambda: st.closest_points(0.05), lambda: st.closest_points_device(0, 4, 0.05, 3, 0, p)):
        with pytest.raises(RuntimeError, match="a bounded wait ran out"):
            call()
    assert st.lib.snk_link_pairs(st.h) == 0 and st.lib.snk_closest_slots(st.h, 3) == 0
    st.close()


# 11. the client
@gpu
def test_client(pkg):
    D = 0.05
    p = pkg.BulletClient()
    plane = p.loadURDF("plane.urdf")
    snake = p.loadURDF("snake/snake.urdf", flags=p.URDF_USE_SELF_COLLISION)
    block = p.loadURDF("snake/block.urdf", basePosition=ncl.BOX_FAR, useFixedBase=1)
    st = p._stepper()
    st.set_state(ncl.family(16, 4, seed=77)[3:4].astype(np.float32))      # (the one of the four with the box within reach)
    pts, _, cnt = st.closest_points(D)
    links = st.contact_links()
    assert cnt[0, 0] > 0 and cnt[0, 1] > 1

    def tuples(rows, other):
        return [(0, snake, other, int(links[int(r[12])]), -1 if other == block else int(links[int(r[13])]),
                 tuple(float(v) for v in r[0:3]), tuple(float(v) for v in r[3:6]), tuple(float(v) for v in r[6:9]), float(r[9]),
                 0.0, 0.0, (0.0, 0.0, 0.0), 0.0, (0.0, 0.0, 0.0)) for r in rows if r[14] != 0.0]
    want_box, want_links = tuples(pts[0, :32], block), tuples(pts[0, 32:], snake)
    assert p.getClosestPoints(snake, block, D) == want_box and p.getClosestPoints(block, snake, D) == want_box
    assert p.getClosestPoints(snake, snake, D) == want_links and all(len(t) == 14 for t in want_links)
    la = want_box[0][3]
    assert p.getClosestPoints(snake, block, D, linkIndexA=la) == [t for t in want_box if t[3] == la]
    assert p.getClosestPoints(block, snake, D, linkIndexB=la) == [t for t in want_box if t[3] == la]
    assert p.getClosestPoints(block, snake, D, linkIndexA=-1) == want_box and p.getClosestPoints(snake, block, D, linkIndexB=5) == []
    la, lb = want_links[0][3], want_links[0][4]
    assert p.getClosestPoints(snake, snake, D, linkIndexA=la) == [t for t in want_links if t[3] == la]
    assert p.getClosestPoints(snake, snake, D, linkIndexB=lb) == [t for t in want_links if t[4] == lb]
    for a, b in ((snake, plane), (plane, snake), (block, plane), (snake, 7), (block, block)):
        with pytest.raises(NotImplementedError):
            p.getClosestPoints(a, b, D)
    with pytest.raises(NotImplementedError):
        p.getClosestPoints(snake, block, D, physicsClientId=0)
    p.close()
