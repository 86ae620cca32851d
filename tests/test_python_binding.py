"""CPU tests of the Python seam's marshalling (bullet-envs_amd/_lib.py, device_env.py): the one host-argument helper and
its exception, that no check in front of a C call is an `assert` statement, and the public surface pinned against
tests/golden/python_surface.json.  No handle, no device."""
import ast
import importlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(pkg):
    return importlib.import_module("bullet-envs_amd._lib")


def test_the_refusal_is_a_value_error_and_an_assertion_error(lib):
    with pytest.raises(ValueError) as e:
        lib._host(np.zeros((4, 7)), np.float32, (4, 8), "actions")
    assert isinstance(e.value, AssertionError) and isinstance(e.value, lib._ArgError)
    assert str(e.value) == "actions must have shape (4, 8), got (4, 7)"
    with pytest.raises(AssertionError):
        lib._host(np.zeros(3), np.float32, (4,), "mu")
    with pytest.raises(lib._ArgError, match=r"^gen_force must be \[4, 22\], got \(4, 21\)$"):       # (a call site's own words)
        lib._host(np.zeros((4, 21)), np.float32, (4, 22), "gen_force", "gen_force must be [4, 22]")


def test_host_argument_forms(lib):
    # converted where the call site converts: another dtype, a list, a strided view
    a = lib._host(np.arange(12.0).reshape(4, 3), np.float32, (4, 3), "x")
    assert a.dtype == np.float32 and a.flags.c_contiguous and a[3, 2] == 11
    assert lib._host([[1, 2], [3, 4]], np.int32, (2, 2), "x").dtype == np.int32
    v = np.arange(24, dtype=np.float32).reshape(4, 6)[:, ::2]
    c = lib._host(v, np.float32, (4, 3), "x")
    assert c.flags.c_contiguous and np.array_equal(c, v)
    same = np.zeros((4, 3), np.float32)
    assert lib._host(same, np.float32, (4, 3), "x") is same                 # nothing to convert: no copy
    # None only where the call allows absence
    assert lib._host(None, np.float32, (4, 3), "x", optional=True) is None
    with pytest.raises(lib._ArgError):
        lib._host(None, np.float32, (4, 3), "x")
    # the call writes into the caller's array: nothing is converted, the wrong dtype or a strided view is refused
    assert lib._host(same, np.float32, (4, 3), "actions", inplace=True) is same
    for bad in (np.zeros((4, 3)), v, [[0.0] * 3] * 4):
        with pytest.raises(lib._ArgError, match="actions must be a C-contiguous float32 ndarray"):
            lib._host(bad, np.float32, (4, 3), "actions", inplace=True)
    with pytest.raises(lib._ArgError, match="actions must have shape"):
        lib._host(np.zeros((4, 2), np.float32), np.float32, (4, 3), "actions", inplace=True)
    # one row for every env
    row = np.arange(3, dtype=np.float64)
    b = lib._host(row, np.float32, (4, 3), "pose", row=True)
    assert b.shape == (4, 3) and b.flags.c_contiguous and b.flags.writeable and np.array_equal(b, np.tile(row, (4, 1)))
    assert lib._host(np.ones((4, 3)), np.float32, (4, 3), "pose", row=True).shape == (4, 3)
    with pytest.raises(lib._ArgError, match=r"got \(2,\)"):
        lib._host(np.zeros(2), np.float32, (4, 3), "pose", row=True)
    with pytest.raises(lib._ArgError):
        lib._host(row, np.float32, (4, 3), "pose")                           # (only where the call site says so)
    # a flat list of any length, and of one length; bool and uint8 masks
    assert lib._host([[0, 1], [2, 3]], np.int32, None, "ids", flat=True).tolist() == [0, 1, 2, 3]
    assert lib._host(np.array([True, False, True]), np.uint8, (3,), "active", flat=True).tolist() == [1, 0, 1]
    assert lib._host(np.ones((3, 1), np.uint8), np.uint8, (3,), "active", flat=True).shape == (3,)
    with pytest.raises(lib._ArgError, match=r"active must be \[3\], got \(4,\)"):
        lib._host(np.ones(4, bool), np.uint8, (3,), "active", "active must be [3]", flat=True)
    assert lib._host(np.zeros((0, 6)), np.float32, None, "rays").shape == (0, 6)         # any shape: the caller checks it


def test_pointers(lib):
    import ctypes as C
    assert lib._ptr(None) is None
    for dtype, ctype in ((np.float32, C.c_float), (np.uint8, C.c_uint8), (np.int32, C.c_int32), (np.float64, C.c_double)):
        a = np.arange(3).astype(dtype)
        p = lib._ptr(a)
        assert isinstance(p, C.POINTER(ctype)) and C.cast(p, C.c_void_p).value == a.ctypes.data and p[2] == 2
    # a device pointer 0 is NULL to the library as None is: the *_device pass-throughs hand their arguments on as they are
    assert lib.load().snk_reset(0, 0, 0, 0) != 0 and "null" in lib.last_error()
    f = np.zeros(2, np.float32)
    assert C.cast(lib.fptr(f), C.c_void_p).value == f.ctypes.data


def test_call_names_the_call_once(lib, pkg):
    with pytest.raises(RuntimeError, match=r"^snk_debug_rows_layout failed: .*16 or 32"):
        lib.rows_layout(24)
    with pytest.raises(ValueError, match=r"camera target must hold 3 values, got \(2,\)"):
        lib.view_matrix_ypr([0, 0], 1.5, 0, 0)
    assert np.array_equal(lib.contact_links(16), lib._contact_links(lib.default_params(n_modules=16)))


def test_no_assert_statement_guards_a_call():
    for name in ("_lib.py", "device_env.py"):
        path = os.path.join(ROOT, "bullet-envs_amd", name)
        tree = ast.parse(open(path).read(), path)
        found = [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)]
        assert not found, "%s: `assert` statements at lines %s vanish under python -O; raise _ArgError" % (name, found)


def test_public_surface_is_the_pinned_one(pkg):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        from make_python_surface import surface
    finally:
        sys.path.pop(0)
    with open(os.path.join(ROOT, "tests", "golden", "python_surface.json")) as f:
        pinned = json.load(f)
    got = surface()
    assert sorted(got) == sorted(pinned)
    for owner in sorted(pinned):
        assert sorted(got[owner]) == sorted(pinned[owner]), owner
        for name in sorted(pinned[owner]):
            assert got[owner][name] == pinned[owner][name], "%s.%s" % (owner, name)
