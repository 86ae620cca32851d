// One instantiation of the step kernel by itself (tools/dbg/loop_spills.sh): -DKN=16 -DKV=true | -DKN=16 -DKV=false | -DKN=32 -DKV=false
// (-DKR=1 | 2: a solver-rules variant, snk_lds.hpp: LdsFor; -DKT=true: the traced kernel of snk_step_traced)
#include <hip/hip_runtime.h>
#include "../../include/snk.h"
#include "../../bullet-envs_amd/csrc/snk_device.hpp"
#ifndef KN
#define KN 16
#define KV true
#endif
#ifndef KR
#define KR 0
#endif
#ifndef KT
#define KT false
#endif
template __global__ void snk::env_step_sched_kernel<KN, KV, KR, KT>(snk::StepArgs);
