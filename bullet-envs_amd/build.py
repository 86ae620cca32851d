"""Builds libsnk.so (HIP kernels + C ABI) in-tree for gfx950.

hipcc cross-compiles without a GPU; the .so is git-ignored but travels to the GPU box
with the gpurun snapshot.
"""
import collections
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsnk.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "snk.h")

# The library's translation units, one row each, in the order they are built and stamped: the source under csrc/, how it is
# built, the suffix of its stamp (the command of its last build, kept next to the library) and its object.  A unit with an
# object is a code object of its own, compiled apart and linked in by the unit without one: the library's own command.
#   api     the step kernels and the C ABI.  libsnk.so.cmd stays the command of this unit alone, flags and source (the
#           pinned bits of tests/test_gpu_bits.py are keyed by it and by the toolchain): the objects it links are not in it
#   render  the renderer and the ray test
#   world   the link states, the reported contacts, the closest points and the env fork
#   dyn     the dynamics queries: mass matrix, bias forces, link Jacobians
Unit = collections.namedtuple("Unit", "name source mode stamp obj")
UNITS = (
    Unit("api", "csrc/snk_api.hip", "-shared", ".cmd", None),
    Unit("render", "csrc/snk_render.hip", "-c", ".render.cmd", "snk_render.o"),
    Unit("world", "csrc/snk_world.hip", "-c", ".world.cmd", "snk_world.o"),
    Unit("dyn", "csrc/snk_dyn.hip", "-c", ".dyn.cmd", "snk_dyn.o"),
)
# What the tools and the tests take from the table: the sources (tools/same_isa.py, tools/kernel_resources.py) and the
# files that describe a build of the default library (tests/bit_pins.py keys the pinned bits by prefixes of this list)
SOURCES = tuple(u.source for u in UNITS)
STAMPS = (os.path.basename(LIB) + ".toolchain",) + tuple(os.path.basename(LIB) + u.stamp for u in UNITS)


def sources():
    """Every file under csrc/ is a dependency of the library (snk_api.hip includes the step kernels' headers, snk_render.hip
    the layers it reuses): a stale
    libsnk.so after an edit of ANY of them would travel to the GPU box unnoticed (it is git-ignored, not gpurun-ignored)."""
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".h")))


# The flags every build of the translation unit uses (tools/dbg/loop_spills.sh asks for them: `build.py --print-flags`).
# -greedy-regclass-priority-trumps-globalness: the register-resident solve keeps 192 row registers + 16 motor columns
# alive across its loop; with the allocator's default priorities 4-12 of them ended up in scratch memory, reloaded
# in EVERY Gauss-Seidel iteration, and which ones changed with every edit of unrelated code (round 3: 314 k ...
# 341 k env-steps/s for the same arithmetic).  With this priority rule: two reloads per iteration, 342.8 k.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-mllvm",
         "-greedy-regclass-priority-trumps-globalness=1"]


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else "hipcc"


def _object(unit, target):
    """snk_<unit>.o for the default library, <stem>_<unit>.o next to a variant"""
    return os.path.join(HERE, unit.obj) if target == LIB else os.path.splitext(target)[0] + unit.obj[len("snk"):]


def _command(unit, target=LIB, defines=(), extra=()):
    """The command that builds `unit` for the library `target`: its object, or (the unit without one) the library."""
    out = _object(unit, target) if unit.obj else target
    return [_hipcc()] + FLAGS + [unit.mode, "-fPIC", os.path.join(HERE, unit.source), "-o", out] + \
        ["-D" + d for d in defines] + list(extra)


def toolchain_text():
    """What compiled the library: hipcc's own version lines (HIP version, clang version), kept next to the library
    (libsnk.so.toolchain) -- tests/test_gpu_bits.py keys its pinned hashes by it."""
    try:
        out = subprocess.check_output([_hipcc(), "--version"], text=True, stderr=subprocess.STDOUT)
    except (OSError, subprocess.CalledProcessError):
        return "unknown"
    keep = [ln.strip() for ln in out.splitlines() if ln.startswith("HIP version") or "clang version" in ln]
    return " | ".join(keep) if keep else "unknown"


def _stamp_text(cmd):
    """The command line as it is kept next to the library: paths relative to this directory, so that the copy of the tree
    on a GPU box (another absolute path) does not look like another build."""
    return " ".join(os.path.relpath(a, HERE) if os.path.isabs(a) and a.startswith(os.path.dirname(HERE)) else a for a in cmd)


def stamp_texts(target=LIB, defines=(), extra=()):
    """[(file, text)] of everything a build of `target` leaves next to it, in STAMPS' order: the toolchain, then each
    unit's command.  What build() writes, what an up-to-date library must hold, and what tests/test_bit_pin_keys.py
    computes the pins' keys from without a compile."""
    return [(target + ".toolchain", toolchain_text())] + \
        [(target + u.stamp, _stamp_text(_command(u, target, defines, extra))) for u in UNITS]


def _up_to_date(target, defines=()):
    """The library is there, no source is newer than it, and it was built by THESE command lines (other flags or -D
    defines: mtimes cannot see that)."""
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    if any(os.path.getmtime(d) > t for d in sources() + [HEADER, os.path.abspath(__file__)]):
        return False
    try:
        for u in UNITS:
            with open(target + u.stamp) as f:
                if f.read() != _stamp_text(_command(u, target, defines)):
                    return False
    except OSError:
        return False
    return True


def needs_build():
    """Stale when a source is newer than the library -- or when the library was built by ANOTHER command line (a
    libsnk.so from an experiment would travel to the GPU box as the product).  The command of each unit's last build is
    kept next to the library (libsnk.so.cmd and the other stamps, git-ignored with it)."""
    return not _up_to_date(LIB)


def build(force=False, verbose=False, defines=(), out=None):
    """defines/out: instrumented variants (e.g. -DSNK_PROFILE -> libsnk_prof.so, tools/profile_phases.py).  The default
    output (libsnk.so) is only ever built with the default command: variants and compiler experiments (SNK_EXTRA_FLAGS)
    need an `out` of their own."""
    extra = os.environ.get("SNK_EXTRA_FLAGS", "").split()        # compiler experiments
    if out is None and (defines or extra):
        raise RuntimeError("bullet-envs_amd/build.py: -D defines / SNK_EXTRA_FLAGS need an output of their own (out=...): "
                           "libsnk.so is the product and is built with the default flags only")
    target = out or LIB
    if out is None and not force and not needs_build():
        if not os.path.exists(LIB + ".toolchain"):          # (a library from before round 6: same image, same compiler)
            with open(LIB + ".toolchain", "w") as f:
                f.write(toolchain_text())
        return LIB
    (link,) = [_command(u, target, defines, extra) for u in UNITS if not u.obj]
    objs = [_object(u, target) for u in UNITS if u.obj]
    # (the objects first: hipcc reads every input behind a .hip file as HIP source)
    for r in [_command(u, target, defines, extra) for u in UNITS if u.obj] + [[link[0]] + objs + link[1:]]:
        if verbose:
            r = [r[0], "-Rpass-analysis=kernel-resource-usage"] + r[1:]
            print(" ".join(r))
        subprocess.check_call(r)
    for path, text in stamp_texts(target, defines, extra):
        with open(path, "w") as f:
            f.write(text)
    return target


SCALAR_LIB = os.path.join(HERE, "libsnk_scalar.so")


def build_scalar(force=False):
    """libsnk_scalar.so: the same sources with -DSNK_SCALAR_DYNAMICS, the wave-uniform form of fk_vel and of the velocity
    refresh (csrc/snk_dynamics.hpp) that the shipped kernels' lane form is compared with, byte for byte
    (tests/test_gpu_lane_dynamics.py), and timed against.  Unlike the other variants it belongs to the test suite, so it
    is rebuilt only when stale: a source newer than it, or another command line."""
    if not force and _up_to_date(SCALAR_LIB, ("SNK_SCALAR_DYNAMICS",)):
        return SCALAR_LIB
    return build(force=True, defines=("SNK_SCALAR_DYNAMICS",), out=SCALAR_LIB)


if __name__ == "__main__":
    if "--print-flags" in sys.argv:
        print(" ".join(FLAGS))
    elif "--profile" in sys.argv:
        print(build(force=True, defines=("SNK_PROFILE",), out=os.path.join(HERE, "libsnk_prof.so")))
    elif "--profile-fine" in sys.argv:     # the dynamics' own pieces instead of the phases (tools/profile_phases.py fine)
        print(build(force=True, defines=("SNK_PROFILE", "SNK_PROFILE_FINE"), out=os.path.join(HERE, "libsnk_prof_fine.so")))
    elif "--scalar-dynamics" in sys.argv:  # the wave-uniform form of fk_vel and the sweeps (tests/test_gpu_lane_dynamics.py, A/B timing)
        print(build_scalar(force=True))
    elif "--sched-debug" in sys.argv:      # per-wave accounting of the step kernel's scheduler (tools/sched_stats.py)
        print(build(force=True, defines=("SNK_SCHED_DEBUG",), out=os.path.join(HERE, "libsnk_dbg.so")))
    else:
        build(force="--force" in sys.argv, verbose="-v" in sys.argv)
        print(LIB)
