"""Generates tests/golden/python_surface.json: the public surface of the Python binding as the commit it is run on has it --

    _lib      every public name of bullet-envs_amd/_lib.py (modules aside): a function with its signature, a class, a constant
    classes   Stepper, Snapshot, DeviceVecEnv, DeviceWorld, ShardedVecEnv: the constructor's signature and every public
              method (with its signature), property and class attribute

-- each signature as str(inspect.signature(...)).  The file was written on the commit BEFORE the binding's marshalling
moved into shared helpers; tests/test_python_surface.py recomputes it with `surface` from here and asks for equality, so
a refactor of the binding cannot drop or reshape a public name unnoticed.  A pull request that adds public API runs
this again.  Reads nothing but the package; needs no GPU.

Run:  python tests/golden/make_python_surface.py [OUTPUT (default: next to this file)]
"""
import importlib
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = (("_lib", "Stepper"), ("_lib", "Snapshot"), ("device_env", "DeviceVecEnv"), ("device_env", "DeviceWorld"),
           ("device_env", "ShardedVecEnv"))


def _describe(owner, name):
    raw = inspect.getattr_static(owner, name)
    if isinstance(raw, property):
        return "property"
    obj = getattr(owner, name)
    if inspect.isclass(obj):
        return "class"
    if callable(obj):
        return ("staticmethod " if isinstance(raw, staticmethod) else "classmethod " if isinstance(raw, classmethod) else "") \
            + str(inspect.signature(obj))
    return "constant"


def _public(owner):
    return sorted(n for n in dir(owner) if not n.startswith("_") and not inspect.ismodule(getattr(owner, n)))


def surface(pkg_name="bullet-envs_amd"):
    mods = {m: importlib.import_module("%s.%s" % (pkg_name, m)) for m in ("_lib", "device_env")}
    out = {"_lib": {n: _describe(mods["_lib"], n) for n in _public(mods["_lib"])}}
    for m, c in CLASSES:
        cls = getattr(mods[m], c)
        out[c] = dict({n: _describe(cls, n) for n in _public(cls)}, __init__=str(inspect.signature(cls)))
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "python_surface.json")
    with open(path, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s" % path)
