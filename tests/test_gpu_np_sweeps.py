"""The HIP kernels against tests/np_substep.py sweep by sweep: n_iterations k in 1, 2, 3, 5, 10, 25 without the residual
exit, on the three solves, under the scenarios of tests/test_gpu_np_substep.py (which holds them at 50 sweeps).

Fifty sweeps of a stiff solve blur a wrong rule and amplified round-off into the same heavy tail; one sweep does not.
The float32 oracle's own worst distance to the model is 3e-5 after one sweep where it is 3e-4 ... 0.24 after fifty, so
the same gates (conftest.f32_gate through test_gpu_np_substep._run: median 1.5 x with floor 1e-6, p90 2 x with floor
1e-5, worst 2 x with cap 5e-2; contact and iteration counts equal to the float64 oracle's) are far tighter here.  Sweep 1
takes the non-contact rows backward and meets the friction rows while most normal impulses are still zero (a pair whose
bound is zero is skipped); sweep 2 takes them forward with the bounds live; from sweep 3 on nothing new happens, and
a case that passes there and fails later is amplification, not a rule.

The states of a (path, scenario) are the same at every k: the same states climb the ladder.  16 states on 16 links, 8 on
32.  test_long_ladder climbs from 64 to 512 sweeps on the 32-link states of test_converged_solve (1000 sweeps).

Cases that fail are STRICT xfails with the measured figure (profiles/sweep_ladder.txt holds every case's).
"""
import numpy as np
import pytest

from conftest import random_state
from test_gpu_np_substep import PATHS, _ground, _open, _path, _run

pytestmark = pytest.mark.gpu

LADDER = (1, 2, 3, 5, 10, 25)
LONG_LADDER = (64, 128, 256, 512)
SCENARIOS = ["default", "cone_friction 0", "friction_directions 1", "plane friction 0", "plane friction 6",
             "velocity clamp", "past the limits"]


def _scenario(scenario, n, streamed):
    """(states, targets, parameter overrides, plane friction, compare the iteration count) -- a function of the path and
    the scenario alone, never of k."""
    rng = np.random.default_rng(2000 + n + 7 * streamed + 31 * SCENARIOS.index(scenario))
    B = 16 if n == 16 else 8
    over, mu, check_iters = dict(residual_threshold=0.0), None, True
    if scenario == "cone_friction 0":
        over.update(cone_friction=0)
    elif scenario == "friction_directions 1":
        over.update(friction_directions=1)
    if scenario.startswith("plane friction"):
        mu = float(scenario.split()[-1])
        S = _ground(rng, n, B, vamp=1.0)
    elif scenario == "velocity clamp":
        # as test_velocity_clamp builds it: weak motors, qd near +-100, in the air and on the ground; the exit that
        # test excuses (an exactly zero residual) can come before k sweeps here too
        over.update(max_motor_impulse=0.05)
        check_iters = False
        S = np.zeros((B, 13 + 2 * n))
        for i in range(B):
            S[i] = random_state(rng, n, z=1.0 if i % 2 else 0.026, qamp=0.3, vamp=0.3, flat=i % 2 == 0)
            S[i, 13 + n:] = rng.choice([-1, 1], n) * rng.uniform(99.5, 100.0, n)
    elif scenario == "past the limits":
        S = _ground(rng, n, B)
        for i in range(B):
            S[i, 13:13 + n] = rng.choice([-1, 1], n) * rng.uniform(1.575, 1.8, n) * (rng.uniform(size=n) < 0.4)
    else:
        S = _ground(rng, n, B)
    return S, rng.uniform(-0.5, 0.5, (B, n)), over, mu, check_iters


# The cases that miss a gate, with the figure that misses it by most (GPU against the float32 oracle's, their ratio):
# strict, so a fix turns them into failures until the entry goes.  DESIGN.md 3 says which open finding each belongs to.
OPEN = {
    ("register-resident", "default", 10): "velocity median 2.0e-05 against the float32 oracle's 1.3e-05 (1.5 x)",
    ("register-resident", "cone_friction 0", 5): "velocity worst 2.0e-01 against the float32 oracle's 1.0e-04 (1972.6 x)",
    ("register-resident", "cone_friction 0", 25): "velocity p90 3.5e-04 against the float32 oracle's 8.6e-05 (4.1 x)",
    ("register-resident", "plane friction 6", 3): "velocity p90 1.4e-04 against the float32 oracle's 4.1e-05 (3.3 x)",
    ("register-resident", "plane friction 6", 5): "velocity p90 1.6e-03 against the float32 oracle's 5.7e-04 (2.8 x)",
    ("register-resident", "past the limits", 2): "velocity p90 2.1e-04 against the float32 oracle's 7.1e-05 (2.9 x)",
    ("register-resident", "past the limits", 3): "velocity p90 1.4e-04 against the float32 oracle's 6.0e-05 (2.4 x)",
    ("streamed-row", "default", 1): "velocity p90 6.7e-05 against the float32 oracle's 2.6e-05 (2.6 x)",
    ("streamed-row", "default", 2): "velocity p90 2.5e-04 against the float32 oracle's 9.6e-05 (2.6 x)",
    ("streamed-row", "default", 25): "velocity median 2.0e-05 against the float32 oracle's 1.2e-05 (1.6 x)",
    ("streamed-row", "cone_friction 0", 1): "velocity p90 4.8e-05 against the float32 oracle's 2.0e-05 (2.4 x)",
    ("streamed-row", "cone_friction 0", 5): "velocity p90 4.1e-05 against the float32 oracle's 1.7e-05 (2.4 x)",
    ("streamed-row", "cone_friction 0", 10): "velocity p90 6.9e-05 against the float32 oracle's 3.3e-05 (2.0 x)",
    ("streamed-row", "cone_friction 0", 25): "velocity worst 1.9e-01 against the float32 oracle's 8.4e-02 (2.3 x)",
    ("streamed-row", "friction_directions 1", 2): "velocity p90 1.3e-04 against the float32 oracle's 3.3e-05 (4.0 x)",
    ("streamed-row", "friction_directions 1", 10): "velocity p90 7.1e-05 against the float32 oracle's 3.2e-05 (2.2 x)",
    ("streamed-row", "friction_directions 1", 25): "velocity p90 2.0e-04 against the float32 oracle's 9.5e-05 (2.1 x)",
    ("streamed-row", "plane friction 0", 1): "velocity p90 4.8e-05 against the float32 oracle's 2.3e-05 (2.1 x)",
    ("streamed-row", "plane friction 0", 2): "velocity p90 4.3e-05 against the float32 oracle's 2.0e-05 (2.2 x)",
    ("streamed-row", "plane friction 0", 5): "velocity p90 4.3e-05 against the float32 oracle's 2.0e-05 (2.1 x)",
    ("streamed-row", "plane friction 6", 1): "velocity p90 1.2e-04 against the float32 oracle's 3.2e-05 (3.8 x)",
    ("streamed-row", "plane friction 6", 2): "motor torque p90 1.1e-05 against the float32 oracle's 3.6e-06 (3.1 x)",
    ("streamed-row", "plane friction 6", 3): "velocity p90 3.2e-04 against the float32 oracle's 1.3e-04 (2.4 x)",
    ("streamed-row", "plane friction 6", 10): "motor torque p90 1.6e-05 against the float32 oracle's 6.8e-06 (2.3 x)",
    ("streamed-row", "plane friction 6", 25): "velocity p90 9.5e-04 against the float32 oracle's 3.4e-04 (2.8 x)",
    ("streamed-row", "past the limits", 3): "velocity median 4.6e-05 against the float32 oracle's 2.3e-05 (2.0 x)",
    ("streamed-row", "past the limits", 10): "velocity median 7.8e-05 against the float32 oracle's 3.4e-05 (2.3 x)",
    ("32 links", "default", 1): "velocity p90 7.4e-04 against the float32 oracle's 3.4e-04 (2.2 x)",
    ("32 links", "default", 5): "velocity p90 2.4e-03 against the float32 oracle's 1.1e-03 (2.2 x)",
    ("32 links", "default", 10): "velocity p90 6.1e-03 against the float32 oracle's 1.0e-03 (6.1 x)",
    ("32 links", "default", 25): "velocity p90 4.4e-03 against the float32 oracle's 9.0e-04 (4.9 x)",
    ("32 links", "friction_directions 1", 10): "velocity p90 1.1e-03 against the float32 oracle's 4.4e-04 (2.6 x)",
    ("32 links", "friction_directions 1", 25): "velocity p90 1.8e-03 against the float32 oracle's 4.8e-04 (3.8 x)",
    ("32 links", "plane friction 6", 5): "motor torque p90 6.7e-05 against the float32 oracle's 2.2e-05 (3.0 x)",
    ("32 links", "plane friction 6", 10): "velocity worst 8.6e-02 against the float32 oracle's 2.1e-02 (4.0 x)",
    ("32 links", "plane friction 6", 25): "velocity worst 1.3e+00 against the float32 oracle's 3.1e-01 (4.0 x)",
}


def _cases():
    for path, _, _ in PATHS:
        for scenario in SCENARIOS:
            for k in LADDER:
                why = OPEN.get((path, scenario, k))
                yield pytest.param(path, scenario, k, marks=[_open(why)] if why else [])


@pytest.mark.parametrize("path,scenario,k", list(_cases()))
def test_sweep_ladder(pkg, oracle_mod, monkeypatch, path, scenario, k):
    n, streamed = _path(monkeypatch, path)
    S, T, over, mu, check_iters = _scenario(scenario, n, streamed)
    _run(pkg, oracle_mod, "%s, %s, %d sweeps" % (path, scenario, k), n, S, T, dict(over, n_iterations=k), mu=mu,
         check_iters=check_iters)


LONG_OPEN = {
    64: "velocity median 2.2e-04 against the float32 oracle's 1.2e-04 (1.9 x), p90 1.5e-01 against 1.4e-03 (109 x)",
    128: "velocity median 4.2e-02 against the float32 oracle's 4.0e-03 (10 x)",
    256: "velocity median 6.7e-02 against the float32 oracle's 8.2e-03 (8.2 x)",
    512: "velocity median 1.2e-01 against the float32 oracle's 3.7e-04 (318 x)",
}


@pytest.mark.parametrize("k", [pytest.param(k, marks=[_open(LONG_OPEN[k])] if k in LONG_OPEN else [])
                               for k in LONG_LADDER])
def test_long_ladder(pkg, oracle_mod, monkeypatch, k):
    """The 32-link chain between 50 and 1000 sweeps, on test_converged_solve's 8 states (same seed, same draws): at which
    sweep count its MEDIAN leaves the model."""
    n, streamed = _path(monkeypatch, "32 links")
    rng = np.random.default_rng(1700 + n + 7 * streamed)
    B = 8
    _run(pkg, oracle_mod, "32 links, %d sweeps" % k, n, _ground(rng, n, B), rng.uniform(-0.5, 0.5, (B, n)),
         dict(residual_threshold=0.0, n_iterations=k))
