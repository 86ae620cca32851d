"""Wall-clock ms per call of every host form at a size where the call's own overhead shows (the procedure of
profiles/r17_host_forms_before_after.txt): 64 envs x 16 links after three gait steps, 8 ids (one repeated), 32 x 32
images, 4 (src, dst) pairs, 16 shared rays, 4 Jacobian points; median of 5 rounds of 200 calls after 20 untimed ones,
through the Stepper methods.  One JSON line per form.
    [SNK_LIB=<lib>] python tools/host_forms_rate.py        (on the GPU box)"""
import importlib, json, sys, time
import numpy as np
sys.path.insert(0, '.')
import bench
pkg = importlib.import_module("bullet-envs_amd")
lib = pkg._lib
E, ROUNDS, CALLS, UNTIMED = 64, 5, 200, 20
st = pkg.Stepper(E)
st.reset()
act = [bench.gait_actions(np.arange(E), j).astype(np.float32) for j in range(3)]
for a in act:
    st.step(a.copy())
snap = st.snapshot()
ids = [3, 0, 0, 9, 17, 33, 41, 63]
view, proj = lib.default_camera(32, 32)
targets = np.zeros((E, st.n), np.float32)
rays = np.zeros((16, lib.RAY_FLOATS), np.float32)
rays[:, 0] = np.linspace(-1.0, 3.0, 16)
rays[:, 2], rays[:, 3], rays[:, 5] = 1.0, rays[:, 0], -1.0
FORMS = (
    ("snk_reset_host", lambda: st.reset()),
    ("snk_step_host", lambda: st.step(act[0].copy())),
    ("snk_step_traced_host", lambda: st.step_traced(act[0].copy())),
    ("snk_substep_host", lambda: st.substep(targets)),
    ("snk_get_obs", lambda: st.get_obs()),
    ("snk_link_states_host", lambda: st.link_states(ids)),
    ("snk_contacts_host", lambda: st.contacts(ids)),
    ("snk_closest_points_host", lambda: st.closest_points(0.05, ids, flags=lib.PAIRS_LINKS, max_pairs=16)),
    ("snk_copy_envs_host", lambda: st.copy_envs([3, 0, 9, 17], [1, 2, 4, 5])),
    ("snk_render_host", lambda: st.render(view, proj, 32, 32, env_ids=ids)),
    ("snk_ray_test_host", lambda: st.ray_test(rays, ids)),
    ("snk_dynamics_host", lambda: st.dynamics(ids)),
    ("snk_jacobians_host", lambda: st.jacobians([0, 1, 25, 49], env_ids=ids)),
)
for name, call in FORMS:
    st.restore(snap)
    for _ in range(UNTIMED):
        call()
    ms = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        ms.append((time.perf_counter() - t0) / CALLS * 1e3)
    print(json.dumps({"form": name, "median_ms": round(float(np.median(ms)), 4), "rounds_ms": [round(m, 4) for m in ms]}))
st.close()
