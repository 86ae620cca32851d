"""The ray test without a device: known answers of the independent numpy model (tests/np_rays.py, written from the contract
in include/snk.h, "The ray test"); its consistency with the render's contract (the ray through a pixel centre gives that
pixel's id and distance) and with the link states (a ray in a link's frame is the same ray turned into the world by that
link's row of np_link_states); the header's constants against the Python side's; and the float32 twin: the retention
displacement np_rays.DELTA is DETERMINED here -- the smallest of {1e-6, 1e-5, 1e-4} at which the twin flips no id on the
retained rays of every set of tests/ray_sets.py -- with the condition that at DELTA every (kind, set) but `degenerate` keeps
at least 98 % of its rays.
"""
import importlib
import os
import re

import numpy as np
import pytest

import np_link_states as NL
import np_model
import np_rays as NR
import np_render as R
import ray_sets as RY
import render_scenes as RS
from conftest import ROOT


def rest_state(n):
    s = np.zeros(13 + 2 * n)
    s[6] = 1.0
    return s


BLOCK = (np.array([2.0, 0.0, 0.1]), None, np.array([0.1, 0.1, 0.1]))       # snake_gait_test.py:51's block, half extent 0.1


def test_vertical_ray_onto_the_ground():
    m = NR.ray_test(16, rest_state(16), None, [[5, 5, 1, 5, 5, -1], [5, 5, 1, 5, 5, 0.5], [5, 5, -1, 5, 5, 1]])
    assert np.array_equal(m["id"], [0, -1, 0])
    assert np.allclose(m["hits"][0], [0.5, 5, 5, 0, 0, 0, 1, 0], atol=1e-15)
    assert np.array_equal(m["hits"][1], NR.MISS)                        # ends above the ground
    assert np.allclose(m["hits"][2], [0.5, 5, 5, 0, 0, 0, 1, 0], atol=1e-15)      # from below: the plane is met from either side


@pytest.mark.parametrize("n", [16, 32])
def test_ray_onto_the_static_block(n):
    sc = R.scene(n, rest_state(n))
    assert (sc["C"][:, 2] + sc["r"]).max() <= 0.052 + 1e-9              # the resting snake reaches only z = 0.052
    ray = [[0, 0, 0.1, 3, 0, 0.1]]
    m = NR.ray_test(n, rest_state(n), BLOCK, ray)
    assert m["id"][0] == 1 + 2 * n
    assert np.allclose(m["hits"][0], [1.9 / 3, 1.9, 0, 0.1, -1, 0, 0, 1 + 2 * n], atol=1e-12)
    miss = NR.ray_test(n, rest_state(n), BLOCK, ray, flags=NR.GROUND | NR.SNAKE)
    assert np.array_equal(miss["hits"][0], NR.MISS) and miss["id"][0] == -1 and np.isinf(miss["t"][0])
    # lowered into the chain, the same ray meets the base's cap instead -- unless the snake is masked out
    low = [[0.5, 0, 0.03, -3, 0, 0.03]]
    on = NR.ray_test(n, rest_state(n), BLOCK, low)
    assert 1 <= on["id"][0] <= 2 * n and abs(abs(on["hits"][0, 4]) - 1) < 1e-9
    assert NR.ray_test(n, rest_state(n), BLOCK, low, flags=NR.GROUND | NR.BOX)["id"][0] == -1


def test_degenerate_rays_of_the_model():
    n = 16
    s = rest_state(n)
    sc = R.scene(n, s)
    c = sc["C"][9]
    rays = [np.concatenate([c, c + [0, 0.5, 0]]),                 # from inside a cylinder: open along the ray
            [2, 0, 0.1, 2, 0, 1.1],                               # from inside the block
            [1, 1, 1, 1, 1, 1],                                   # zero length
            [0, 1, 0.5, 1, 1, 0.5],                               # parallel to the ground
            [np.nan, 0, 1, 0, 0, -1], [0, 0, 1, 0, np.inf, -1]]   # non-finite entries
    m = NR.ray_test(n, s, BLOCK, rays)
    assert (m["id"] == -1).all() and all(np.array_equal(h, NR.MISS) for h in m["hits"])
    assert NR.retained(n, s, BLOCK, rays).all()


def test_rays_through_pixel_centres_give_the_render():
    """Consistency of the two contracts: from = the pixel centre on the near plane, to = on the far plane."""
    kind, call = "16s", "B"
    n = RS.KINDS[kind][0]
    W, H, shadow, ids, cams, shared, _ = RS.call_inputs(kind, call)
    S, B = RS.states(kind), RS.boxes(kind)
    cam = cams[0].astype(np.float64)
    Minv = np.linalg.inv(cam[16:].reshape(4, 4).T @ cam[:16].reshape(4, 4).T)
    i, j = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    x, y = 2 * i / W - 1, 1 - 2 * j / H
    one = np.ones_like(x)
    a = np.stack([x, y, -one, one], -1) @ Minv.T
    b = np.stack([x, y, one, one], -1) @ Minv.T
    rays = np.concatenate([a[..., :3] / a[..., 3:], b[..., :3] / b[..., 3:]], -1).reshape(-1, 6)
    for k in (1, 3):
        e = ids[k]
        m = NR.ray_test(n, S[e].astype(np.float64), B[e], rays)
        img = R.render(R.scene(n, S[e].astype(np.float64), B[e]), cam[:16], cam[16:], W, H)
        assert np.array_equal(m["id"].reshape(H, W), img["seg"])
        hit = img["seg"] >= 0
        assert hit.any() and (img["seg"] > 0).any()
        assert np.allclose(m["t"].reshape(H, W)[hit], img["t"][hit], rtol=0, atol=1e-11)


@pytest.mark.parametrize("kind", list(RS.KINDS))
def test_parent_frames_are_the_link_states(kind):
    """A ray in the frame of row r is the same ray turned into the world by row r of the link states: origin the COM
    (floats 0-2), orientation the quaternion (floats 3-6).  The float32 twin's frames are np_link_states.twin's."""
    n = RS.KINDS[kind][0]
    S, B = RS.states(kind), RS.boxes(kind)
    rays = RY._fan()[::7]
    for e, row in ((1, 0), (2, 1), (3, 3 * n + 1), (4, 17)):
        st = S[e].astype(np.float64)
        ls = NL.reference(st, n)[row]
        Rl = np_model.quat_to_mat(ls[3:7])
        world = np.concatenate([ls[0:3] + rays[:, 0:3] @ Rl.T, ls[0:3] + rays[:, 3:6] @ Rl.T], -1)
        a, b = NR.ray_test(n, st, B[e], rays, parent_row=row), NR.ray_test(n, st, B[e], world)
        assert np.array_equal(a["id"], b["id"]) and np.allclose(a["hits"], b["hits"], rtol=0, atol=1e-12)
        Rt, ot = NR.parent_frame(n, S[e], row, np.float32)
        tw = NL.twin(S[e], n)[row]
        assert Rt.dtype == np.float32 and np.array_equal(ot, tw[0:3]) and np.array_equal(NL.quat_of(Rt), tw[3:7])
    with pytest.raises(IndexError):
        NR.parent_frame(n, S[0], 3 * n + 2)


def test_constants_are_the_headers(pkg):
    lib = importlib.import_module("bullet-envs_amd._lib")
    text = open(os.path.join(ROOT, "include", "snk.h")).read()
    d = {k: int(v) for k, v in re.findall(r"#define (SNK_(?:RAYS?|HIT)_\w+)\s+(\d+)", text)}
    assert d == dict(SNK_RAY_FLOATS=lib.RAY_FLOATS, SNK_HIT_FLOATS=lib.HIT_FLOATS, SNK_RAYS_GROUND=lib.RAYS_GROUND,
                     SNK_RAYS_SNAKE=lib.RAYS_SNAKE, SNK_RAYS_BOX=lib.RAYS_BOX, SNK_RAYS_SHARED=lib.RAYS_SHARED)
    assert (NR.GROUND, NR.SNAKE, NR.BOX) == (lib.RAYS_GROUND, lib.RAYS_SNAKE, lib.RAYS_BOX) and lib.RAYS_ALL == NR.ALL
    assert pkg.RAYS_ALL == 7 and callable(pkg.BulletClient.rayTest) and callable(pkg.BulletClient.rayTestBatch)
    assert callable(pkg.DeviceWorld.ray_test) and callable(pkg.DeviceWorld.ranges)
    assert "snk_ray_test" in lib.SYMBOLS and "snk_ray_test_host" in lib.SYMBOLS


# ---- the float32 twin: DELTA and the share of rays kept ----
def _twin_flips(delta):
    """(retained rays on which the twin's id differs from the float64 model's, rays left out, rays) over every set, and
    the smallest share of a (kind, set) other than `degenerate` that is kept."""
    bad = out = total = 0
    least = 1.0
    for kind, name in RY.CASES:
        m64, m32, keep = RY.expected(kind, name)
        if delta != NR.DELTA:
            keep = RY.retained(kind, RY.call_inputs(kind, name), delta=delta, base=m64)
        bad += int(((m64["id"] != m32["id"]) & keep).sum())
        out += int((~keep).sum())
        total += keep.size
        if name != "degenerate":
            least = min(least, keep.mean())
    return bad, out, total, least


def test_float32_twin_determines_delta():
    res = {d: _twin_flips(d) for d in (1e-6, 1e-5, 1e-4)}
    for d, (bad, out, total, least) in res.items():
        print("  delta %g: twin flips %d retained ids; %d of %d rays left out; a set keeps at least %.2f %%"
              % (d, bad, out, total, 100 * least))
    agree = [d for d in sorted(res) if all(res[e][0] == 0 for e in res if e >= d)]
    assert agree and min(agree) == NR.DELTA, res
    assert res[NR.DELTA][3] >= 0.98, res


@pytest.mark.parametrize("kind,name", RY.CASES)
def test_share_kept_and_what_the_sets_meet(kind, name):
    """At DELTA every (kind, set) but `degenerate` keeps at least 98 % of its rays, and the sets meet what they are meant
    to: ground, cylinders through side and cap, the box where there is one, and nothing."""
    n = RS.KINDS[kind][0]
    inp = RY.call_inputs(kind, name)
    m64, m32, keep = RY.expected(kind, name)
    ids = m64["id"]
    assert ids.shape == keep.shape == (len(inp["env_ids"]), inp["rays"].shape[-2])
    print("  %s %s: %.2f %% of %d rays kept" % (kind, name, 100 * keep.mean(), keep.size))
    if name != "degenerate":
        assert keep.mean() >= 0.98, (kind, name, keep.mean())
    if name.startswith("fan"):
        assert (ids == 0).any() and (ids == -1).any()
    if name in ("scan", "random257", "random600", "one"):
        assert (ids == 0).any() and ((ids >= 1) & (ids <= 2 * n)).any()
    if name.startswith("random"):
        assert (ids == -1).any() and inp["rays"].shape[1] in (257, 600)
        cyl = (ids >= 1) & (ids <= 2 * n)
        axis = np.abs((m64["hits"][..., 4:7] * np.stack([RY.scenes(kind)[e]["A"][np.clip(ids[r] - 1, 0, 2 * n - 1)]
                                                        for r, e in enumerate(inp["env_ids"])])).sum(-1))
        assert (cyl & (axis > 0.999)).any() and (cyl & (axis < 1e-6)).any()        # cap entries and side entries
        if kind != "32":
            assert (ids == 1 + 2 * n).any()
    if name == "degenerate":
        D = RY.DEGENERATE
        assert (ids[:, D.index("inside_cylinder")] != 1 + RY.DEG_CYL).all()
        assert (ids[:, D.index("inside_box")] != 1 + 2 * n).all()
        assert (m64["hits"][:, D.index("zero_length")] == NR.MISS).all()
        for what in ("level", "in_the_ground_plane"):              # (a lifted chain may be in the way; the ground never is)
            assert (ids[:, D.index(what)] != 0).all(), what
        along = m64["hits"][:, D.index("along_axis")]
        assert (along[:, 7] >= 1).all()
        assert abs(abs(along[0, 4:7] @ RY.scenes(kind)[0]["A"][RY.DEG_CYL]) - 1) < 1e-9      # env 0 lies straight: a cap
