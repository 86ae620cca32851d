"""The bits the query kernels produce, pinned (csrc/snk_world.hpp: link_state_kernel, contacts_kernel,
closest_points_kernel; csrc/snk_render.hpp: render_scene_kernel + render_rays_kernel, ray_scene_kernel + ray_cast_kernel):
sha256 over every output array of the device forms on five environments, for the three kernel variants (16 links
register-resident, 16 links on the streamed-row LDS image -- SNK_FORCE_STREAMED and the free-box handle --, 32 links).  The
accuracy tests of these kernels compare against float64 models through gates of 1.5 to 2 times the float32 twin's error: an
edit that reorders a sum passes them.  An edit that is meant to leave the arithmetic alone (moving code into a shared
helper, a re-layout of a stage) must leave THESE hashes alone.  No physics step runs: states, caches and boxes are written
with set_state / set_manifold / set_box, so these pins do not move when the step kernels' (tests/test_gpu_bits.py) do.

Every id-taking call gets the list IDS -- a repeat and an id outside the handle -- and is called once without a list.
`tools/bits_hash.py query` prints the same hashes for any library of the same ABI (SNK_LIB); `--pins` prints the block of
tests/golden/query_bits.json.  The pins belong to ONE toolchain and flag set and are keyed as tests/test_gpu_bits.py keys
its own (tests/bit_pins.py), over every stamp that describes these units (libsnk.so.toolchain, .cmd, .render.cmd,
.world.cmd); under an unknown key the tests SKIP and say what to do.  A mismatch names the case and the part (which output
array).

test_a_block_taking_a_second_row_... pins nothing: it is the one test of a block that takes a second row (more rows than
the grid's 65536 blocks), where the row loop's trailing barrier is all that keeps the next row's record load from the
lanes still reading this row's."""
import contextlib
import os

import numpy as np
import pytest

import bit_pins
import np_closest as ncl
import ray_sets as RY
import render_scenes as RS
from conftest import random_state
from test_gpu_closest import threshold
from test_gpu_contacts import synthetic_box, synthetic_cache

pytestmark = pytest.mark.gpu

E = 5
IDS = [3, 0, 3, 7, 1]                  # a repeat, and 7: outside a 5-env handle
# variant -> (n_modules, SNK_FORCE_STREAMED): Lds<16, true>, Lds<16, false>, Lds<32, false>
VARIANTS = {"16": (16, False), "16s": (16, True), "32": (32, False)}
# the render's and the ray test's handles: render_scenes' kinds ("16f", the free box, is Lds<16, false> by itself) and
# the static box on the streamed-row image
SCENES = {"16s": ("16s", False), "16f": ("16f", False), "32": ("32", False), "16s-streamed": ("16s", True)}
BOX, LINKS = 1, 2


@contextlib.contextmanager
def stepper(pkg, n, streamed=False, **over):
    """A 5-env handle; `streamed`: created under SNK_FORCE_STREAMED=1 (read at snk_create), the variable put back after."""
    old = os.environ.get("SNK_FORCE_STREAMED")
    if streamed:
        os.environ["SNK_FORCE_STREAMED"] = "1"
    else:
        os.environ.pop("SNK_FORCE_STREAMED", None)
    try:
        st = pkg.Stepper(E, n_modules=n, **over)
    finally:
        if old is None:
            os.environ.pop("SNK_FORCE_STREAMED", None)
        else:
            os.environ["SNK_FORCE_STREAMED"] = old
    try:
        yield st
    finally:
        st.close()


class Dev(object):
    """Tensors on cuda:0 for the device forms, all on the null stream (torch's default): fills, calls and copies are ordered."""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)

    def put(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a), device=self.dev)

    def ids(self, ids):
        return None if ids is None else self.put(np.asarray(ids, np.int32))

    def f32(self, *shape):
        return self.torch.full(shape, -7.0, dtype=self.torch.float32, device=self.dev)

    def i32(self, *shape):
        return self.torch.full(shape, -77, dtype=self.torch.int32, device=self.dev)

    def u8(self, *shape):
        return self.torch.full(shape, 99, dtype=self.torch.uint8, device=self.dev)


def ptr(t):
    return 0 if t is None else t.data_ptr()


def tumbling(n, seed, k=E):
    """k random states with a tumbled base, joints across their range and non-zero twists (test_gpu_world's family)"""
    rng = np.random.default_rng(seed)
    return np.stack([random_state(rng, n, z=0.3, qamp=1.5, vamp=1.0) for _ in range(k)]).astype(np.float32)


def closest_box_states():
    """render_scenes' tumbled boxes moved beside the closest-point family's snakes (bases near the origin)"""
    B = RS.box_states()
    B[:, 0] -= 1.0
    B[:, 1] = 0.45
    return B


def shared_rays():
    """257 rays in a parent's coordinates: ray_sets' two rings at 3 m and at 1.5 m, and one more"""
    fan = RY._fan()
    return np.concatenate([fan, 0.5 * fan, 0.25 * fan[:1]]).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# the cases: name -> function(pkg, d) yielding (part, numpy array)
# ----------------------------------------------------------------------------------------------------------------------
def link_states_case(variant):
    n, streamed = VARIANTS[variant]

    def run(pkg, d):
        with stepper(pkg, n, streamed) as st:
            st.set_state(tumbling(n, 2100 + n), None)
            for part, ids in (("ids", IDS), ("all", None)):
                t, out = d.ids(ids), d.f32(E, st.link_rows, 16)
                st.link_states_device(ptr(t), E, out.data_ptr())
                yield part, out.cpu().numpy()
    return run


def contacts_case(variant, box):
    n, streamed = VARIANTS[variant]

    def run(pkg, d):
        rng = np.random.default_rng(2200 + n)
        with stepper(pkg, n, streamed, **(dict(obstacle=2) if box else {})) as st:
            st.set_state(tumbling(n, 2250 + n), None)
            st.set_manifold(synthetic_cache(rng, n, E))
            if box:
                st.set_box(*synthetic_box(rng, E))
            for tag, ids, with_points in (("ids", IDS, True), ("all", None, True), ("ids_no_points", IDS, False)):
                t = d.ids(ids)
                pts = d.f32(E, st.contact_slots, 16) if with_points else None
                frc, cnt = d.f32(E, 2 * n + 1), d.i32(E)
                st.contacts_device(ptr(t), E, ptr(pts), frc.data_ptr(), cnt.data_ptr())
                if with_points:
                    yield "points_" + tag, pts.cpu().numpy()
                yield "force_" + tag, frc.cpu().numpy()
                yield "count_" + tag, cnt.cpu().numpy()
    return run


def closest_case(variant, sides, obstacle):
    """0.5 m: every env of the family yields hundreds of link-link pairs (358 per env at 16 links), so the
    64-record flush with its carry-over runs; max_pairs 100: below the found count and no multiple of 64."""
    n, streamed = VARIANTS[variant]

    def run(pkg, d):
        over = dict(hull_sides=sides, obstacle=obstacle, obstacle_pos=list(ncl.BOX_NEAR if sides else ncl.BOX_FAR))
        with stepper(pkg, n, streamed, **over) as st:
            st.set_state(ncl.family(n, E, seed=2300 + n).astype(np.float32), None)
            if obstacle == 2:
                st.set_box(closest_box_states(), np.zeros((E, 29), np.float32))
            NP = st.link_pairs
            for tag, ids, D, mp, with_points in (("far_ids", IDS, 0.5, NP, True), ("far_all_clipped", None, 0.5, 100, True),
                                                 ("near_ids_no_points", IDS, 0.05, NP, False)):
                t = d.ids(ids)
                pts = d.f32(E, 2 * n + mp, 16) if with_points else None
                clr, cnt = d.f32(E, 2, 2 * n), d.i32(E, 2)
                st.closest_points_device(ptr(t), E, D, BOX | LINKS, mp, ptr(pts), clr.data_ptr(), cnt.data_ptr())
                cnt_h = cnt.cpu().numpy()
                if tag == "far_all_clipped":
                    assert cnt_h[:, 1].max() > 100, ("no env with more link-link pairs than max_pairs", cnt_h)
                if with_points:
                    yield "points_" + tag, pts.cpu().numpy()
                yield "clearance_" + tag, clr.cpu().numpy()
                yield "count_" + tag, cnt_h
    return run


@contextlib.contextmanager
def scene_handle(pkg, scene):
    kind, streamed = SCENES[scene]
    n, over = RS.KINDS[kind]
    with stepper(pkg, n, streamed, **over) as st:
        st.set_state(RS.states(kind))
        if kind == "16f":
            st.set_box(RS.box_states())
        yield st, kind, n


def rays_case(scene):
    """257 rays per row: one full chunk of 256 and a chunk of one ray"""
    def run(pkg, d):
        with scene_handle(pkg, scene) as (st, kind, n):
            own = RY.call_inputs(kind, "random257")["rays"]                   # [5, 257, 6], world coordinates
            assert own.shape == (E, 257, 6)
            for part, ids, rays, parent, shared in (("hits_own_rays_world_ids", IDS, own, -1, 0),
                                                    ("hits_shared_rays_link_all", None, shared_rays(), 3 * n + 1, 8)):
                t, r, hits = d.ids(ids), d.put(rays), d.f32(E, 257, 8)
                st.ray_test_device(ptr(t), E, r.data_ptr(), 257, parent, 7 | shared, hits.data_ptr())
                yield part, hits.cpu().numpy()
    return run


def render_case(scene):
    """37 x 23: partial tiles on both edges; the shadow flag, depth and segmentation"""
    def run(pkg, d):
        W, H = RS.SIZES["odd"]
        with scene_handle(pkg, scene) as (st, kind, n):
            cm = RS.cameras(kind, W / H)
            names = ("oblique", "reference", "ground", "cut", "oblique")
            each = np.stack([np.concatenate(cm[k][:2]) for k in names]).astype(np.float32)
            for tag, ids, cams, shared in (("ids", IDS, each, False), ("all", None, each[:1], True)):
                t, c = d.ids(ids), d.put(cams)
                rgba, dep, seg = d.u8(E, H, W, 4), d.f32(E, H, W), d.i32(E, H, W)
                st.render_device(ptr(t), E, c.data_ptr(), shared, W, H, 1, rgba.data_ptr(), dep.data_ptr(), seg.data_ptr())
                yield "rgba_" + tag, rgba.cpu().numpy()
                yield "depth_" + tag, dep.cpu().numpy()
                yield "seg_" + tag, seg.cpu().numpy()
    return run


CASES = {}
for _v in VARIANTS:
    CASES["link_states/" + _v] = link_states_case(_v)
    CASES["contacts/" + _v] = contacts_case(_v, False)
    CASES["closest/%s/hull" % _v] = closest_case(_v, 32, 1)
    CASES["closest/%s/implicit" % _v] = closest_case(_v, 0, 1)
CASES["contacts/16+box"] = contacts_case("16", True)
CASES["closest/16+box/hull"] = closest_case("16", 32, 2)
for _s in SCENES:
    CASES["rays/" + _s] = rays_case(_s)
    CASES["render/" + _s] = render_case(_s)


def hashes(pkg, case):
    """{part: sha256[:16]} of a named case, what the test pins and `tools/bits_hash.py query` prints"""
    return bit_pins.array_hashes(CASES[case](pkg, Dev()))


@pytest.mark.parametrize("case", sorted(CASES))
def test_query_bits_are_pinned(pkg, case):
    pytest.importorskip("torch")
    bit_pins.check("query", case, lambda: hashes(pkg, case))


# ----------------------------------------------------------------------------------------------------------------------
# more rows than blocks
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_a_block_taking_a_second_row_gives_the_bits_of_the_first(pkg, variant):
    """The grid of a wave-per-row kernel is capped at 65536 blocks (snk_seam.hpp: grid_for); with 65536 + 3 rows, blocks 0
    to 2 take a second row.  The ids cycle over the five envs, so row r must be, bit for bit, row r - 5: checked on the
    device over every row, those at 65536 and above among them.  Each call's cheap outputs only -- but for
    snk_link_states, whose rows (210 MB at 16 links, 411 MB at 32) are compared where they are."""
    torch = pytest.importorskip("torch")
    n, streamed = VARIANTS[variant]
    d = Dev()
    rows = 65536 + 3
    ids = d.ids(np.arange(rows) % E)
    rng = np.random.default_rng(2500 + n)

    def cyclic(what, t, some=True):
        raw = t.reshape(rows, -1)
        raw = raw if raw.dtype == torch.uint8 else raw.view(torch.int32)
        assert not some or bool(raw[:E].any()), (what, "the first rows hold nothing")
        assert torch.equal(raw[E:], raw[:-E]), (what, "a row differs from the earlier row of the same env")

    with stepper(pkg, n, streamed, obstacle=1, obstacle_pos=list(ncl.BOX_NEAR)) as st:
        S = ncl.family(n, E, seed=2300 + n).astype(np.float32)
        S[:, 7:13] = tumbling(n, 2550 + n)[:, 7:13]
        st.set_state(S, None)
        st.set_manifold(synthetic_cache(rng, n, E))
        out = d.f32(rows, st.link_rows, 16)
        st.link_states_device(ids.data_ptr(), rows, out.data_ptr())
        cyclic("snk_link_states", out)
        del out
        frc, cnt = d.f32(rows, 2 * n + 1), d.i32(rows)
        st.contacts_device(ids.data_ptr(), rows, 0, frc.data_ptr(), cnt.data_ptr())
        cyclic("snk_contacts force", frc)
        cyclic("snk_contacts count", cnt)
        clr, cnt2 = d.f32(rows, 2, 2 * n), d.i32(rows, 2)
        st.closest_points_device(ids.data_ptr(), rows, threshold(st), BOX | LINKS, 0, 0, clr.data_ptr(), cnt2.data_ptr())
        cyclic("snk_closest_points clearance", clr)
        cyclic("snk_closest_points count", cnt2, some=False)      # (at the breaking threshold an env may have no pair)
        ray = d.put(np.array([[0.1, 0.3, 0.5, -0.4, -0.2, -0.1]], np.float32))
        hits = d.f32(rows, 1, 8)
        st.ray_test_device(ids.data_ptr(), rows, ray.data_ptr(), 1, 1, 7 | 8, hits.data_ptr())
        cyclic("snk_ray_test", hits)
        cam = d.put(np.concatenate(RS.cameras("16s", 1.0)["oblique"][:2]).astype(np.float32))
        rgba, dep, seg = d.u8(rows, 1, 1, 4), d.f32(rows, 1, 1), d.i32(rows, 1, 1)
        st.render_device(ids.data_ptr(), rows, cam.data_ptr(), True, 1, 1, 1, rgba.data_ptr(), dep.data_ptr(), seg.data_ptr())
        cyclic("snk_render rgba", rgba)
        cyclic("snk_render depth", dep)
        torch.cuda.synchronize()
