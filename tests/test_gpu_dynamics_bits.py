"""The bits the dynamics queries produce, pinned (csrc/snk_dyn.hpp: dynamics_kernel, jacobians_kernel), as
tests/test_gpu_query_bits.py pins the other query kernels': sha256 over every output array of the device forms on five
environments, for the three kernel variants (16 links register-resident, 16 links on the streamed-row LDS image, 32 links).
The accuracy test of these kernels (tests/test_gpu_dynamics.py) gates at 1.5 to 2 times the float32 twin's error: an edit
that reorders a sum passes it.  An edit that is meant to leave the arithmetic alone must leave THESE hashes alone.  No
physics step runs: the states are written with set_state.

Every call gets the list IDS -- a repeat and an id outside the handle -- and is made once without a list.
tools/dynamics_hash.py prints the same hashes for any library of the same ABI (SNK_LIB); `--pins` prints the block of
tests/golden/dynamics_bits.json.  The pins belong to ONE toolchain and flag set and are keyed over every stamp of the
library (libsnk.so.toolchain, .cmd, .render.cmd, .world.cmd, .dyn.cmd); under an unknown key the tests SKIP and say what to
do.  A mismatch names the case and the part (which output array).  This test names nothing but output hashes."""
import hashlib
import json
import os

import numpy as np
import pytest

import np_dynamics as nd_
from test_gpu_dynamics import VARIANTS, stepper

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dynamics_bits.json")
STAMPS = ("libsnk.so.toolchain", "libsnk.so.cmd", "libsnk.so.render.cmd", "libsnk.so.world.cmd", "libsnk.so.dyn.cmd")

E = 5
IDS = [3, 0, 3, 7, 1]                  # a repeat, and 7: outside a 5-env handle


def toolchain_key():
    pkgdir = os.path.join(os.path.dirname(HERE), "bullet-envs_amd")
    try:
        txt = "\n".join(open(os.path.join(pkgdir, s)).read() for s in STAMPS)
    except OSError:
        return None, "%s are missing (a library not built by bullet-envs_amd/build.py)" % " / ".join(STAMPS)
    return hashlib.sha256(txt.encode()).hexdigest()[:12], txt


def dynamics_case(variant):
    n, streamed = VARIANTS[variant]

    def run(pkg, torch):
        dev = torch.device("cuda", 0)
        nd = n + 6
        # every link of the tree once, each with a point of its own off its COM; then the COMs alone
        rows = np.arange(3 * n + 2, dtype=np.int32)
        local = (0.05 * np.sin(0.7 * np.arange(3 * (3 * n + 2)) + 0.3)).astype(np.float32).reshape(-1, 3)
        rt, lt = torch.as_tensor(rows, device=dev), torch.as_tensor(local, device=dev)
        with stepper(pkg, E, n, streamed) as st:
            st.set_state(nd_.gate_states(n)[:E], None)
            for tag, ids in (("ids", IDS), ("all", None)):
                t = None if ids is None else torch.as_tensor(np.asarray(ids, np.int32), device=dev)
                tp = 0 if t is None else t.data_ptr()
                for flags in (1, 2, 3):
                    M = torch.full((E, nd, nd), -7.0, dtype=torch.float32, device=dev)
                    h = torch.full((E, nd), -7.0, dtype=torch.float32, device=dev)
                    st.dynamics_device(tp, E, flags, M.data_ptr() if flags == 3 else 0, h.data_ptr())
                    if flags == 3:
                        yield "mass_" + tag, M.cpu().numpy()
                    yield "bias%d_%s" % (flags, tag), h.cpu().numpy()
                for part, lp in (("jac_local_", lt.data_ptr()), ("jac_com_", 0)):
                    J = torch.full((E, len(rows), 6, nd), -7.0, dtype=torch.float32, device=dev)
                    st.jacobians_device(tp, E, rt.data_ptr(), lp, len(rows), J.data_ptr())
                    yield part + tag, J.cpu().numpy()
    return run


CASES = {"dynamics/" + v: dynamics_case(v) for v in VARIANTS}


def dynamics_hashes(pkg, cases=None):
    """{case: {part: sha256[:16]}} of the named cases (None: all), what the test pins and tools/dynamics_hash.py prints"""
    import torch
    return {c: {part: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16] for part, a in CASES[c](pkg, torch)}
            for c in (CASES if cases is None else cases)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_dynamics_bits_are_pinned(pkg, case):
    pytest.importorskip("torch")
    key, txt = toolchain_key()
    pinned = json.load(open(GOLDEN))
    if key not in pinned:
        pytest.skip("no pinned dynamics bits for this toolchain / flag set (key %s: %s).  Verify tests/test_gpu_dynamics.py on "
                    "it, then run `python tools/dynamics_hash.py --pins` on the GPU box and add the block it prints to "
                    "tests/golden/dynamics_bits.json." % (key, txt))
    got = dynamics_hashes(pkg, [case])[case]
    want = pinned[key]["cases"][case]
    differ = sorted(p for p in set(got) | set(want) if got.get(p) != want.get(p))
    assert not differ, "%s: %s differ from the pinned bits (got %s)" % (case, ", ".join(differ), got)
