"""Phase durations inside one physics substep (s_memtime ticks, wave 0 of each env), from the
-DSNK_PROFILE build:  python bullet-envs_amd/build.py --profile  (here), then on the GPU box
SNK_LIB=bullet-envs_amd/libsnk_prof.so python tools/profile_phases.py [16|32]
(16: the register-resident solve's substep; 32: the streamed-row solve's)
The dynamics' own pieces instead of the phases (16 links):  python bullet-envs_amd/build.py --profile-fine, then
SNK_LIB=bullet-envs_amd/libsnk_prof_fine.so python tools/profile_phases.py fine"""
import importlib, os, sys
import numpy as np
sys.path.insert(0, '.')
FINE = "fine" in sys.argv[1:]
want = "libsnk_prof_fine.so" if FINE else "libsnk_prof.so"
assert os.environ.get("SNK_LIB", "").endswith(want), "run with SNK_LIB=bullet-envs_amd/" + want
pkg = importlib.import_module("bullet-envs_amd")
names = ["contacts", "bias + ABA (factor, solve)", "sensor pass 1, v += a dt", "rows: motors (ABA deltas)",
         "rows: friction A (ABA deltas)", "  load 64 slots (A)", "rows: friction B (ABA deltas)", "  load 64 slots (B)",
         "rows: normals (ABA deltas)", "  load 32 slots + motor registers", "coupling scalars", "limit rows",
         "PGS, 50 iterations", "sensor pass 2: contact wrenches, FK", "sensor pass 2: bias + ABA", "integrate + FK"]
NL = int(sys.argv[1]) if len(sys.argv) > 1 and not FINE else 16
if FINE:     # the stamps are not contiguous: slot 4 is everything between the outward sweep and the integration
    names = ["body_bias", "ABA inward sweep", "ABA base inverse", "ABA outward sweep", None, "integrate", "fk_vel"]
    # slots 7..11: the pieces of find_contacts_v2 (printed as a table of their own: they come BEFORE body_bias)
    CONTACTS = ["contacts: obstacle and self-pair tests", "contacts: manifold load, refresh, drop",
                "contacts: support search", "contacts: nearest / sort / insert", "contacts: prefix and stores"]
if NL == 32:
    names = ["ground contacts", "link-link contacts (GJK)", "bias + ABA (factor, solve)", "sensor pass 1, v += a dt",
             "rows: M^-1 columns (38 delta sweeps) + assembly, lane = dof", "PGS, 50 iterations", "sensor pass 2", "integrate", "FK of the new pose"]
for B in (1024, 2048):
    st = pkg.Stepper(B, n_modules=NL, residual_threshold=0.0)
    st.reset()
    T = np.zeros((B, NL), np.float32); T[:, 1::2] = 0.3
    st.substep(T, 3)
    _, aux = st.get_state()
    t = aux[:, :len(names)].astype(np.float64)
    m = t.mean(axis=0)
    if FINE:
        m = np.array([v for n_, v in zip(names, m) if n_])
    print("B=%d (%d wave(s)/SIMD): ticks per phase, mean over envs; total %.0f" % (B, B // 1024, m.sum()))
    for n_, v in zip([n_ for n_ in names if n_], m):
        print("   %-36s %9.0f  %5.1f %%" % (n_, v, 100 * v / m.sum()))
    if FINE:
        c = aux[:, len(names):len(names) + len(CONTACTS)].astype(np.float64).mean(axis=0)
        print("   the contact phase's pieces (find_contacts_v2), total %.0f" % c.sum())
        for n_, v in zip(CONTACTS, c):
            print("   %-40s %9.0f  %5.1f %%" % (n_, v, 100 * v / c.sum()))
    st.close()
