"""Host side of the traced step (snk_step_traced): the numpy helper that turns a trace buffer into test mode's per-env
lists (SnakeGymEnv.py:43-44: info['internal_observations'], info['link_positions']), and the row geometry the header
promises.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row_floats(n):
    """include/snk.h, snk_trace_row_floats: the payload [obs 3n + 8 | link positions 3(n + 1)] rounded up to a multiple of
    32 floats (whole 128-byte lines)."""
    payload = (3 * n + 8) + 3 * (n + 1)
    return -(-payload // 32) * 32


def test_row_stride_arithmetic(pkg):
    assert (3 * 16 + 8) + 3 * 17 == 107 and _row_floats(16) == 128
    assert (3 * 32 + 8) + 3 * 33 == 203 and _row_floats(32) == 224
    for n in (16, 32):
        assert pkg.trace_row_floats(n) == _row_floats(n)
        assert pkg.trace_row_floats(n) * 4 % 128 == 0
    # the header states the same numbers
    text = open(os.path.join(ROOT, "include", "snk.h")).read()
    assert "snk_trace_row_floats" in text
    assert re.search(r"107\s*->\s*128", text) and re.search(r"203\s*->\s*224", text)


@pytest.mark.parametrize("n", [16, 32])
def test_trace_to_lists(pkg, n):
    no, nl, row = 3 * n + 8, 3 * (n + 1), _row_floats(n)
    B, R = 5, 7
    sub = np.array([0, 1, R, 3, 2], dtype=np.int32)
    rng = np.random.default_rng(n)
    trace = np.full((B, R, row), np.nan, dtype=np.float32)
    want = rng.normal(size=(B, R, no + nl)).astype(np.float32)
    for i in range(B):
        trace[i, :sub[i], :no + nl] = want[i, :sub[i]]          # the padding and the rows >= sub[i] stay NaN
    io, lp = pkg.trace_to_lists(trace, sub, n)
    assert len(io) == len(lp) == B
    for i in range(B):
        assert isinstance(io[i], list) and isinstance(lp[i], list)
        assert len(io[i]) == len(lp[i]) == sub[i]
        for s in range(sub[i]):
            o, l = io[i][s], lp[i][s]
            assert o.dtype == np.float64 and l.dtype == np.float64
            assert o.shape == (no,) and l.shape == (nl,)
            assert np.array_equal(o, want[i, s, :no].astype(np.float64))
            # [x_0..x_n, y_0..y_n, z_0..z_n], straight behind the observation
            assert np.array_equal(l[:n + 1], want[i, s, no:no + n + 1].astype(np.float64))
            assert np.array_equal(l[n + 1:2 * (n + 1)], want[i, s, no + n + 1:no + 2 * (n + 1)].astype(np.float64))
            assert np.array_equal(l[2 * (n + 1):], want[i, s, no + 2 * (n + 1):no + nl].astype(np.float64))
            assert np.isfinite(o).all() and np.isfinite(l).all()      # nothing of an unwritten row or the padding
    # the lists own their data
    io[2][0][:] = 7.0
    assert not (trace[2, 0, :no] == 7.0).any()


def test_trace_to_lists_refuses_what_cannot_be_a_trace(pkg):
    t = np.zeros((2, 3, 128), dtype=np.float32)
    with pytest.raises(ValueError):
        pkg.trace_to_lists(t, np.array([1, 4]), 16)           # more substeps than rows
    with pytest.raises(ValueError):
        pkg.trace_to_lists(t, np.array([1]), 16)              # one count per env
    with pytest.raises(ValueError):
        pkg.trace_to_lists(t, np.array([1, 1]), 32)           # rows too short for 32 links


def test_telemetry_argument_is_checked(pkg):
    mod = __import__("importlib").import_module("bullet-envs_amd.snake_env")
    assert mod.TELEMETRY == ('replay', 'kernel')
    with pytest.raises(ValueError):
        mod._check_telemetry('host')
    with pytest.raises(ValueError):
        pkg.Snake(None, None, None, telemetry='device')
    assert pkg.Snake(None, None, None).telemetry is None and pkg.Snake(None, None, None, telemetry='kernel').telemetry == 'kernel'
