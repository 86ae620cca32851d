"""How often the second sensor pass runs per physics substep under the bench's gait (sensor_pass_needed): the
-DSNK_PROFILE build counts the passes of the register-resident substep in the third overflow counter.
    SNK_LIB=$PWD/bullet-envs_amd/libsnk_prof.so python tools/dbg/sensor_rate.py [env-steps=40]"""
import importlib, os, sys
import numpy as np
sys.path.insert(0, '.')
assert os.environ.get("SNK_LIB", "").endswith("libsnk_prof.so")
from bench import gait_actions
pkg = importlib.import_module("bullet-envs_amd")
K = int(sys.argv[1]) if len(sys.argv) > 1 else 40
B = 4096
st = pkg.Stepper(B, n_modules=16)
st.reset()
for j in range(10):
    st.step(gait_actions(np.arange(B), j, 8).astype(np.float32))
p0 = st.contact_overflow()[2]
sub = 0
for j in range(10, 10 + K):
    sub += int(st.step(gait_actions(np.arange(B), j, 8).astype(np.float32))[3].sum())
passes = st.contact_overflow()[2] - p0
print("16 links, gait, %d envs x %d env-steps: %d substeps (%.2f per env-step), %d sensor passes = %.4f per substep, "
      "%.3f per env-step" % (B, K, sub, sub / (B * K), passes, passes / sub, passes / (B * K)))
