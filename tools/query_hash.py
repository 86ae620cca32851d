"""Hashes of the query kernels' outputs (link states, contacts, closest points, ray test, render) on fixed inputs, to compare
two builds bit for bit -- tools/state_hash.py's counterpart for the kernels below the fused step:
    SNK_LIB=<lib> python tools/query_hash.py [CASE ...]    one line per case and part (no CASE: all)
    python tools/query_hash.py --pins                      the block tests/golden/query_bits.json holds for this build"""
import importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
pkg = importlib.import_module("bullet-envs_amd")
import test_gpu_query_bits as T

if "--pins" in sys.argv:
    key, txt = T.toolchain_key()
    cases = T.query_hashes(pkg)
    print('"%s": {' % key)
    print('  "built_by": %s,' % json.dumps(txt.replace("\n", " || ")))
    print('  "cases": {')
    print(",\n".join('    %s: %s' % (json.dumps(c), json.dumps(cases[c], sort_keys=True)) for c in sorted(cases)))
    print("  }\n}")
else:
    names = [a for a in sys.argv[1:] if not a.startswith("-")]
    for c, parts in sorted(T.query_hashes(pkg, names or None).items()):
        for p in sorted(parts):
            print("%-28s %-28s %s" % (c, p, parts[p]))
