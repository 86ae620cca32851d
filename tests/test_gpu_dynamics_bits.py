"""The bits the dynamics queries produce, pinned (csrc/snk_dyn.hpp: dynamics_kernel, jacobians_kernel), as
tests/test_gpu_query_bits.py pins the other query kernels': sha256 over every output array of the device forms on five
environments, for the three kernel variants (16 links register-resident, 16 links on the streamed-row LDS image, 32 links).
The accuracy test of these kernels (tests/test_gpu_dynamics.py) gates at 1.5 to 2 times the float32 twin's error: an edit
that reorders a sum passes it.  An edit that is meant to leave the arithmetic alone must leave THESE hashes alone.  No
physics step runs: the states are written with set_state.

Every call gets the list IDS -- a repeat and an id outside the handle -- and is made once without a list.
`tools/bits_hash.py dynamics` prints the same hashes for any library of the same ABI (SNK_LIB); `--pins` prints the block of
tests/golden/dynamics_bits.json.  The pins belong to ONE toolchain and flag set and are keyed (tests/bit_pins.py) over every
stamp of the library (libsnk.so.toolchain, .cmd, .render.cmd, .world.cmd, .dyn.cmd); under an unknown key the tests SKIP and
say what to do.  A mismatch names the case and the part (which output array).  This test names nothing but output hashes."""
import numpy as np
import pytest

import bit_pins
import np_dynamics as nd_
from test_gpu_dynamics import VARIANTS, stepper

pytestmark = pytest.mark.gpu

E = 5
IDS = [3, 0, 3, 7, 1]                  # a repeat, and 7: outside a 5-env handle


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


def hashes(pkg, case):
    """{part: sha256[:16]} of a named case, what the test pins and `tools/bits_hash.py dynamics` prints"""
    import torch
    return bit_pins.array_hashes(CASES[case](pkg, torch))


@pytest.mark.parametrize("case", sorted(CASES))
def test_dynamics_bits_are_pinned(pkg, case):
    pytest.importorskip("torch")
    bit_pins.check("dynamics", case, lambda: hashes(pkg, case))
