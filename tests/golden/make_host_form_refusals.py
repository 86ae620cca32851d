"""Generates tests/golden/host_form_refusals.json: snk_last_error's text for every id and count refusal of the four host
forms (snk_render_host, snk_link_states_host, snk_contacts_host, snk_copy_envs_host) on a handle of N_ENVS envs --

    an id of -1, an id of n_envs, a count of n_envs + 1 without an id list     the three forms that take env_ids
    an id of -1 and of n_envs in either list, a repeated dst, a dst that is also a src     the fork

-- as the library of the commit it is run on words them.  It was run once, on the commit BEFORE the host forms moved onto
the shared scaffolding of csrc/snk_seam.hpp; tests/test_gpu_host_forms.py holds every later library to the same strings,
and imports `refusals` from here so that the calls are written once.  Reads nothing but the package; needs a GPU.

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
    with open(out, "w") as f:
        json.dump({"n_envs": N_ENVS, "refusals": texts[0]}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(texts[0]), "refusals")
    for k in sorted(texts[0]):
        print("  %-44s %s" % (k, texts[0][k]))


if __name__ == "__main__":
    main()
