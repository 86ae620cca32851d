"""Generates tests/golden/host_form_refusals.json: snk_last_error's text for every id and count refusal of the four host
forms (snk_render_host, snk_link_states_host, snk_contacts_host, snk_copy_envs_host) on a handle of N_ENVS envs --

    an id of -1, an id of n_envs, a count of n_envs + 1 without an id list     the three forms that take env_ids
    an id of -1 and of n_envs in either list, a repeated dst, a dst that is also a src     the fork

-- and, of the host forms that moved onto that scaffolding later (snk_reset_host, snk_step_host, snk_step_traced_host,
snk_substep_host, snk_get_obs, snk_mean_height, snk_link_positions) --

    a null buffer, k < 0, trace_rows 0 and trace_rows = max_counter     refused before anything is launched
    every one of them on a second handle (one for the seven) after snk_debug_raise_alarm

-- as the library of the commit it is run on words them.  The first fifteen were written on the commit BEFORE the first
four host forms moved onto the shared scaffolding of csrc/snk_seam.hpp, the others on the commit before the rest did
(SNK_LIB names that commit's library; the entries already in the file are kept as they are, and a library that words
one of them differently stops the run); tests/test_gpu_host_forms.py holds every later library to the same strings, and
imports `refusals` from here so that the calls are written once.  Reads nothing but the package; needs a GPU.

Run on a GPU:  python tests/golden/make_host_form_refusals.py [OUTPUT (default: next to this file)]
"""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_ENVS = 4
HANDLES = (dict(n_modules=16), dict(n_modules=16, obstacle=2), dict(n_modules=32))


def refusals(pkg, st):
    """{case: message} on the Stepper `st` (N_ENVS envs); every call is made on the C ABI and must be refused."""
    L, lib, E = st.lib, pkg._lib, st.n_envs
    i32 = C.POINTER(C.c_int32)
    cams, _ = lib.camera_block(*lib.default_camera(8, 8), 1)
    rgba = np.zeros((E + 1, 8, 8, 4), np.uint8)
    links = np.zeros((E + 1, 3 * st.n + 2, lib.LINK_STATE_FLOATS), np.float32)
    force = np.zeros((E + 1, 2 * st.n + 1), np.float32)

    def ptr(ids):
        return None if ids is None else np.asarray(ids, np.int32).ctypes.data_as(i32)

    forms = {
        "render": lambda ids, k: L.snk_render_host(st.h, ptr(ids), k, lib.fptr(cams), 1, 8, 8, 0,
                                                   rgba.ctypes.data_as(C.POINTER(C.c_uint8)), None, None),
        "link_states": lambda ids, k: L.snk_link_states_host(st.h, ptr(ids), k, lib.fptr(links)),
        "contacts": lambda ids, k: L.snk_contacts_host(st.h, ptr(ids), k, None, lib.fptr(force), None),
    }
    out = {}

    def refused(case, rc):
        assert rc != 0, case + " was not refused"
        out[case] = lib.last_error()

    for name, call in forms.items():
        refused(name + ": id -1", call([0, -1], 2))
        refused(name + ": id n_envs", call([E, 0], 2))
        refused(name + ": count n_envs + 1 without ids", call(None, E + 1))
    for case, src, dst in (("src -1", [0, -1], [2, 3]), ("src n_envs", [E, 0], [2, 3]), ("dst -1", [0, 1], [-1, 3]),
                           ("dst n_envs", [0, 1], [2, E]), ("repeated dst", [0, 1, 0], [2, 3, 2]),
                           ("dst also a src", [0, 1], [2, 0])):
        refused("copy_envs: " + case, L.snk_copy_envs_host(st.h, ptr(src), ptr(dst), len(src), 0))

    # the forms that moved later: valid buffers, and what each call is refused for
    u8 = C.POINTER(C.c_uint8)
    act = np.zeros((E, st.act_dim), np.float32)
    obs = np.zeros((E, st.obs_dim), np.float32)
    rew, done, sub = np.zeros(E, np.float32), np.zeros(E, np.uint8), np.zeros(E, np.int32)
    rows = int(st.params.max_counter) + 1
    trace = np.zeros((E, rows, lib.trace_row_floats(st.n)), np.float32)
    tgt, info = np.zeros((E, st.n), np.float32), np.zeros((E, 2), np.int32)
    height, pos = np.zeros(E, np.float32), np.zeros((E, 3 * (st.n + 1)), np.float32)
    step = (lib.fptr(obs), lib.fptr(rew), done.ctypes.data_as(u8), sub.ctypes.data_as(i32))

    def traced(h, trace_ptr, trace_rows):
        return L.snk_step_traced_host(h, lib.fptr(act), *step, trace_ptr, trace_rows, 1)

    refused("step: null actions", L.snk_step_host(st.h, None, *step, 1))
    refused("step_traced: null trace", traced(st.h, None, rows))
    refused("step_traced: trace_rows 0", traced(st.h, lib.fptr(trace), 0))
    refused("step_traced: trace_rows max_counter", traced(st.h, lib.fptr(trace), rows - 1))
    refused("substep: null targets", L.snk_substep_host(st.h, None, 1, info.ctypes.data_as(i32)))
    refused("substep: k < 0", L.snk_substep_host(st.h, lib.fptr(tgt), -1, info.ctypes.data_as(i32)))
    refused("get_obs: null", L.snk_get_obs(st.h, None))
    refused("mean_height: null", L.snk_mean_height(st.h, None))
    refused("link_positions: null", L.snk_link_positions(st.h, None))
    dead = pkg.Stepper(E, params=st.params)
    try:
        dead.debug_raise_alarm()
        refused("reset: alarm", L.snk_reset_host(dead.h, None, lib.fptr(obs)))
        refused("step: alarm", L.snk_step_host(dead.h, lib.fptr(act), *step, 1))
        refused("step_traced: alarm", traced(dead.h, lib.fptr(trace), rows))
        refused("substep: alarm", L.snk_substep_host(dead.h, lib.fptr(tgt), 1, info.ctypes.data_as(i32)))
        refused("get_obs: alarm", L.snk_get_obs(dead.h, lib.fptr(obs)))
        refused("mean_height: alarm", L.snk_mean_height(dead.h, lib.fptr(height)))
        refused("link_positions: alarm", L.snk_link_positions(dead.h, lib.fptr(pos)))
    finally:
        dead.close()
    return out


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    pkg = importlib.import_module("bullet-envs_amd")
    texts = []
    for kw in HANDLES:
        st = pkg.Stepper(N_ENVS, **kw)
        st.reset()
        texts.append(refusals(pkg, st))
        st.close()
    assert texts[0] == texts[1] == texts[2], "the refusals depend on the handle's variant"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "host_form_refusals.json")
    with open(os.path.join(HERE, "host_form_refusals.json")) as f:
        kept = json.load(f)["refusals"]
    changed = sorted(k for k in kept if texts[0].get(k) != kept[k])
    assert not changed, "this library words recorded refusals differently: %s" % changed
    with open(out, "w") as f:
        json.dump({"n_envs": N_ENVS, "refusals": texts[0]}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(texts[0]), "refusals")
    for k in sorted(texts[0]):
        print("  %-44s %s" % (k, texts[0][k]))


if __name__ == "__main__":
    main()
