"""Hashes of the pinned workloads on fixed inputs, to compare two builds bit for bit: the step kernels' (state and outputs
after four gait env-steps), the query kernels' (link states, contacts, closest points, ray test, render) and the dynamics
queries' (snk_dynamics, snk_jacobians) -- the families of tests/bit_pins.py, each with the cases of its test module:
    SNK_LIB=<lib> python tools/bits_hash.py FAMILY [CASE ...]    one line per case and part (no CASE: all)
    python tools/bits_hash.py FAMILY --pins                      the block the family's store under tests/golden/ holds for this build"""
import importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
pkg = importlib.import_module("bullet-envs_amd")
import bit_pins

names = [a for a in sys.argv[1:] if not a.startswith("-")]
if not names or names[0] not in bit_pins.FAMILIES:
    sys.exit(__doc__ + "\nFAMILY: " + " | ".join(bit_pins.FAMILIES))
family = names[0]
T = importlib.import_module(bit_pins.FAMILIES[family].module)
pins = "--pins" in sys.argv
cases = {c: T.hashes(pkg, c) for c in (sorted(T.CASES) if pins or not names[1:] else names[1:])}

if pins:
    key, txt = bit_pins.built_key(family)
    print('"%s": {' % key)
    print('  "built_by": %s,' % json.dumps(txt.replace("\n", " || ")))
    print('  "cases": {')
    print(",\n".join('    %s: %s' % (json.dumps(c), json.dumps(cases[c], sort_keys=True)) for c in sorted(cases)))
    print("  }\n}")
else:
    for c, parts in sorted(cases.items()):
        for p in sorted(parts):
            print("%-28s %-28s %s" % (c, p, parts[p]))
