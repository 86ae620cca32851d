"""Snapshot, Stepper.snapshot and Stepper.restore without a GPU: a fake handle records which accessors were called, in
which order, with what (the real ones are pinned on the GPU by tests/test_gpu_snapshot.py)."""
import numpy as np
import pytest

KEYS = ["state", "aux", "ground_friction", "manifold", "box_state", "box_manifold", "reset_pose"]


class FakeStepper:
    """The part of Stepper that snapshot() and restore() touch."""

    def __init__(self, n_envs, n=4, contact_model=1, obstacle=2):
        self.n_envs, self.n, self.calls = n_envs, n, []
        self.params = type("P", (), dict(obstacle=obstacle))()
        rng = np.random.default_rng(n_envs)
        self.data = dict(state=rng.normal(size=(n_envs, 13 + 2 * n)), aux=rng.normal(size=(n_envs, n + 2)),
                         ground_friction=rng.uniform(0.5, 1.5, n_envs), manifold=rng.normal(size=(n_envs, 2 * n, 29)),
                         box_state=rng.normal(size=(n_envs, 13)), box_manifold=rng.normal(size=(n_envs, 29)),
                         reset_pose=rng.normal(size=(n_envs, 7 + n)))
        self.data = {k: v.astype(np.float32) for k, v in self.data.items()}
        if not contact_model:
            self.data["manifold"] = None

    def get_state(self):
        return self.data["state"].copy(), self.data["aux"].copy()

    def get_ground_friction(self):
        return self.data["ground_friction"].copy()

    def get_manifold(self):
        return None if self.data["manifold"] is None else self.data["manifold"].copy()

    def get_box(self):
        self.calls.append(("get_box",))
        return self.data["box_state"].copy(), self.data["box_manifold"].copy()

    def get_reset_pose(self):
        self.calls.append(("get_reset_pose",))
        return self.data["reset_pose"].copy()

    def set_ground_friction(self, mu):
        self.calls.append(("set_ground_friction", mu))

    def set_state(self, state=None, aux=None):
        self.calls.append(("set_state", state, aux))

    def set_manifold(self, m):
        self.calls.append(("set_manifold", m))

    def set_box(self, state=None, manifold=None):
        self.calls.append(("set_box", state, manifold))

    def set_reset_pose(self, pose, mask=None):
        self.calls.append(("set_reset_pose", pose, mask))


def full(pkg, B=5):
    fake = FakeStepper(B)
    return fake, pkg.Stepper.snapshot(fake)


def fields(snap):
    return [getattr(snap, k) for k in KEYS]


def test_snapshot_reads_every_field_the_handle_has(pkg):
    fake, snap = full(pkg)
    for k in KEYS:
        assert np.array_equal(getattr(snap, k), fake.data[k]), k
    assert snap.n_envs == 5
    # no free box, no contact cache, no table asked for: None, and the accessors that would fail are not even called
    bare = FakeStepper(3, contact_model=0, obstacle=1)
    snap = pkg.Stepper.snapshot(bare, reset_pose=False)
    assert snap.manifold is None and snap.box_state is None and snap.box_manifold is None and snap.reset_pose is None
    assert bare.calls == [] and snap.n_envs == 3
    assert np.array_equal(snap.ground_friction, bare.data["ground_friction"])


def test_restore_calls_the_setters_in_the_stated_order(pkg):
    fake, snap = full(pkg)
    target = FakeStepper(5)
    pkg.Stepper.restore(target, snap)
    assert [c[0] for c in target.calls] == ["set_ground_friction", "set_state", "set_manifold", "set_box", "set_reset_pose"]
    got = dict((c[0], c[1:]) for c in target.calls)
    assert got["set_ground_friction"][0] is snap.ground_friction
    assert got["set_state"][0] is snap.state and got["set_state"][1] is snap.aux
    assert got["set_manifold"][0] is snap.manifold
    assert got["set_box"][0] is snap.box_state and got["set_box"][1] is snap.box_manifold
    assert got["set_reset_pose"][0] is snap.reset_pose and got["set_reset_pose"][1] is None      # every env, no mask


def test_restore_skips_what_is_absent(pkg):
    fake, snap = full(pkg)
    snap.manifold = snap.box_state = snap.box_manifold = snap.reset_pose = None
    target = FakeStepper(5)
    pkg.Stepper.restore(target, snap)
    assert [c[0] for c in target.calls] == ["set_ground_friction", "set_state"]
    snap.ground_friction = None
    target.calls = []
    pkg.Stepper.restore(target, snap)
    assert [c[0] for c in target.calls] == ["set_state"]


def test_restore_refuses_another_size(pkg):
    fake, snap = full(pkg, 5)
    target = FakeStepper(4)
    with pytest.raises(ValueError) as ei:
        pkg.Stepper.restore(target, snap)
    assert "5 environments" in str(ei.value) and "this handle 4" in str(ei.value)
    assert target.calls == []                            # refused first: nothing was written
    pkg.Stepper.restore(target, snap[:4])             # a subset of the right size is taken


def test_indexing_applies_to_every_field_present(pkg):
    fake, snap = full(pkg, 6)
    snap.box_state = snap.box_manifold = None
    perm = np.array([3, 0, 5, 1, 4, 2])
    p = snap[perm]
    assert p is not snap and p.n_envs == 6
    for k in KEYS:
        if getattr(snap, k) is None:
            assert getattr(p, k) is None, k
        else:
            assert np.array_equal(getattr(p, k), getattr(snap, k)[perm]), k
    assert np.array_equal(snap.state, fake.data["state"])            # the source is unchanged
    # replicas and subsets are the same operation
    src = np.arange(6)
    src[[1, 4]] = 2
    r = snap[src]
    assert np.array_equal(r.state[1], snap.state[2]) and np.array_equal(r.manifold[4], snap.manifold[2])
    assert np.array_equal(r.ground_friction, snap.ground_friction[src]) and snap[1:3].n_envs == 2


def test_arrays_has_exactly_the_seven_keys(pkg):
    fake, snap = full(pkg)
    arr = snap.arrays()
    assert sorted(arr) == sorted(KEYS)
    for k in KEYS:
        assert arr[k] is getattr(snap, k)
    snap.manifold = snap.reset_pose = None
    arr = snap.arrays()
    assert sorted(arr) == sorted(KEYS)
    for k in ("manifold", "reset_pose"):                 # an empty float32 array stands for an absent field
        assert arr[k].dtype == np.float32 and arr[k].shape == (0,)


@pytest.mark.parametrize("absent", [(), ("manifold",), ("box_state", "box_manifold"), ("reset_pose",),
                                    ("manifold", "box_state", "box_manifold", "reset_pose")])
def test_from_arrays_round_trips(pkg, absent):
    Snapshot = pkg.Snapshot
    fake, snap = full(pkg)
    for k in absent:
        setattr(snap, k, None)
    back = Snapshot.from_arrays(snap.arrays())
    for k in KEYS:
        if k in absent:
            assert getattr(back, k) is None, k
        else:
            assert np.array_equal(getattr(back, k), getattr(snap, k)), k


def test_from_arrays_of_a_mapping_without_the_optional_keys(pkg):
    Snapshot = pkg.Snapshot
    fake, snap = full(pkg)
    arr = snap.arrays()
    old = {k: arr[k] for k in ("state", "aux", "ground_friction")}
    back = Snapshot.from_arrays(old)
    assert back.manifold is None and back.box_state is None and back.box_manifold is None and back.reset_pose is None
    assert np.array_equal(back.state, snap.state) and np.array_equal(back.aux, snap.aux)
    assert np.array_equal(back.ground_friction, snap.ground_friction) and back.n_envs == 5
    extra = dict(arr, n_envs=np.int64(5), format=np.int64(2))        # a checkpoint's other entries are not fields
    assert fields(Snapshot.from_arrays(extra))[0] is arr["state"]
