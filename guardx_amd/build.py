"""Build the project's shared libraries (MAIN, then every entry of LIBRARIES, then of LEARNER_LIBRARIES, then of
UPDATE_LIBRARIES, then of FIT_LIBRARIES, then of GRAD_LIBRARIES, then of ACTOR_LIBRARIES, then of SAFETY_LIBRARIES, in that
order) for gfx950 in-tree with hipcc.

    python -m guardx_amd.build [--force]

hipcc cross-compiles without a GPU; the resulting .so travels with the tree.
-ffp-contract=off: every fp32 operator in the kernels is one IEEE operation
(fused multiply-adds are written fmaf()), which is what makes the device
results reproducible against the CPU checker bit for bit.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
# one translation unit per robot (gx_robot_kernels.inl instantiated for it), compiled in parallel
SOURCES = ["gx_api.hip", "gx_kernels.hip", "gx_gae.hip", "gx_policy_step.hip", "gx_kernels_point.hip", "gx_kernels_point_bare.hip", "gx_kernels_swimmer.hip",
           "gx_kernels_point_split.hip", "gx_kernels_point_bare_split.hip", "gx_kernels_swimmer_split.hip",
           "gx_kernels_ant.hip", "gx_kernels_walker.hip"]
HEADERS = ["gx_device.h", "gx_robot.h", "gx_robot_ant.h", "gx_robot_ant_group.h", "gx_robot_legs.h", "gx_robot_legs_group.h", "gx_policy.h", "gx_kernels.h", "gx_robot_kernels.inl",
           "gx_split_rollout.inl", os.path.join("..", "..", "include", "guardx.h")]
FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]
# No per-source flags.  History: LLVM's inter-procedural register allocation (on by default for
# amdgcn at -O3) lets a noinline callee use, without saving them, the VGPRs in whose lanes the CALLER parks spilled SGPRs
# (exec masks, v254/v255): after the call the masks are garbage and masked-off lanes store through garbage addresses
# (found with rocgdb in round 2 on group_rollout_kernel<WalkerRobot,...> with two call sites of the step; again in round
# 3 with ONE call site once the callee grew).  The cure that held: no call at all.  reset_done's fake step is tabulated
# with the layout pool (Pool::fake), so every kernel steps in one place, and both the Ant's and the Walker's lane-group
# steps are always_inline (gx_robot_ant_group.h, gx_robot_legs_group.h:substep_call); tests/test_native_abi.py asserts
# that no lane-group kernel contains an s_swappc_b64.
# Round 4: LLVM's "max-ilp" machine-scheduling strategy for the translation units that hold the two-kernel rollout of the
# robots whose dynamics pass is ONE wave per SIMD (the serial chains of the Point and the Swimmer; everything else of
# those robots -- step, reset, the closed-loop policy rollout, which lost 2.5 % with it -- keeps the default).  A lone wave issues a dependent vector instruction
# every ~5.75 cycles and an independent one every 4 (tools/probes/chain_clock_probe.hip); the default strategy schedules
# for occupancy / register pressure, this one interleaves independent instructions and halves the s_nop hazard fillers
# (538 -> 291 in the Point's dynamics pass).  Same instructions, same arithmetic, other order: results are bit-identical
# (the parity suite and the soaks run on it).  Same-box A/B: Point dynamics pass 91 -> 86.5 us, observation pass 33.6 ->
# 32.9 us, Swimmer dynamics pass 459 - 467 -> 451 us per 200 steps.  NOT for gx_kernels.hip: the layout sampler's phases are
# 2.4 % faster alone with it (554 -> 541 us) but the epoch, where they share every SIMD with other waves, is 2 % slower
# (0.517 -> 0.527 ms, 774 -> 759 M env-steps/s on one box); and not for the Ant's / Walker's lane-group kernels, which do
# not gain (1272 -> 1280, 2350 -> 2370 us).
_MAX_ILP = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
# The Ant's lane-group step without the SLP vectorizer: its packed-fp32 forms (v_pk_mul_f32 / v_pk_add_f32, 340 in the
# step loop) cost more register shuffles than they save issue slots there -- 1231 -> 1152 us per 200 steps of 2000 envs
# (same-box A/B).  The Walker's is indifferent (2269 -> 2252 / 2274 us) and keeps the default; the Point's dynamics pass
# is 3 % SLOWER without it (87.0 -> 89.3 us).
PER_SOURCE_FLAGS = {"gx_kernels_point_split.hip": _MAX_ILP, "gx_kernels_point_bare_split.hip": _MAX_ILP,
                    "gx_kernels_swimmer_split.hip": _MAX_ILP, "gx_kernels_ant.hip": ["-fno-slp-vectorize"]}
LOCK_FILE = os.path.join(LIB_DIR, ".build.lock")

_COMPILER = None


def compiler_id():
    """`hipcc --version` in one line (HIP version + clang version): part of the build identity, because the kernels
    here are sensitive to what a particular compiler does (hipcc 7.2 miscompiled the CALL form of the Ant's / Walker's
    lane-group step -- the callee clobbered the caller's SGPR-spill VGPRs -- and is worked around by inlining it,
    gx_robot_legs_group.h; the soak and the parity suite were run on this compiler) -- a different compiler is a
    different build."""
    global _COMPILER
    if _COMPILER is None:
        try:
            out = subprocess.run([_hipcc(), "--version"], capture_output=True, text=True, timeout=60).stdout
            keep = [ln.strip() for ln in out.splitlines() if ln.startswith(("HIP version", "AMD clang version"))]
            _COMPILER = "; ".join(keep) or "unknown"
        except Exception:  # noqa: BLE001 - no compiler on this machine: the prebuilt library's own record stands
            _COMPILER = "unknown"
    return _COMPILER


class Library:
    """libguardx_<key>.so from <sources> with -D<macro>="<source_hash()>" compiled in (its gx?_build_id()), checked at
    load time by guardx_amd/_sidelib.py.  Without `obj_dir` one command compiles and links the sources; with it every
    source becomes an object there (reused across builds while its `.id` tag stands, compiled in parallel, each with
    its `per_source_flags`), the first source carries the id and the compiler's name, and the objects are linked."""

    def __init__(self, key, macro, sources, headers, build_id_file, obj_dir=None, per_source_flags=None):
        self.key, self.macro, self.sources, self.headers = key, macro, sources, headers
        self.lib = os.path.join(LIB_DIR, "libguardx_%s.so" % key)
        self.build_id_file = os.path.join(LIB_DIR, build_id_file)
        self.obj_dir, self.per_source_flags = obj_dir, per_source_flags

    def source_hash(self):
        """sha256 over every source, every project header they include, the flags and the compiler version that go
        into the library: the identity of a build.  It is compiled into the library and checked at load time, so a
        stale or foreign .so is never loaded silently, whatever the file times say (the tree is copied to the GPU box
        without them)."""
        import hashlib
        h = hashlib.sha256()
        h.update(compiler_id().encode() + b"\0")
        for n in sorted(set(self.sources) | set(self.headers)):
            h.update(n.encode() + b"\0")
            with open(os.path.join(CSRC, n), "rb") as f:
                h.update(f.read())
        flags = FLAGS if self.per_source_flags is None else (FLAGS, sorted(self.per_source_flags.items()))
        h.update(repr(flags).encode())
        return h.hexdigest()[:24]

    def built_id(self):
        try:
            with open(self.build_id_file) as f:
                return f.read().strip()
        except OSError:
            return None

    def needs_build(self):
        return not os.path.exists(self.lib) or self.built_id() != self.source_hash()

    def _extra(self, src):
        # GX_EXTRA_FLAGS_<source stem>="...": experiments (replaces the per-source defaults when it starts with "=")
        env = os.environ.get("GX_EXTRA_FLAGS_" + os.path.splitext(src)[0], "")
        if env.startswith("="):
            return env[1:].split()
        return self.per_source_flags.get(src, []) + env.split()

    def _obj(self, src):
        return os.path.join(self.obj_dir, os.path.splitext(src)[0] + ".o")

    def _dep_hash(self, src):
        """identity of one object file: its source, every header, its flags (objects are reused across builds)"""
        import hashlib
        h = hashlib.sha256()
        for n in [src] + sorted(set(self.headers)):
            with open(os.path.join(CSRC, n), "rb") as f:
                h.update(n.encode() + b"\0" + f.read())
        h.update(repr((FLAGS, self._extra(src), compiler_id())).encode())
        return h.hexdigest()[:24]

    def _compile(self, src, bid, force, verbose):
        obj, tag = self._obj(src), self._obj(src) + ".id"
        carries_id = src == self.sources[0]
        want = self._dep_hash(src) + (":" + bid if carries_id else "")
        try:
            have = open(tag).read().strip()
        except OSError:
            have = None
        if not force and os.path.exists(obj) and have == want:
            return
        ids = ['-D%s="%s"' % (self.macro, bid), '-DGX_BUILD_COMPILER="%s"' % compiler_id().replace('"', "'")]
        _run([_hipcc()] + FLAGS + self._extra(src) + (ids if carries_id else []) +
             ["-c", os.path.join(CSRC, src), "-o", obj], verbose)
        with open(tag, "w") as f:
            f.write(want)

    def build(self, verbose=False, jobs=None, force=False):
        """Link to a temporary name and rename into place (nobody can dlopen a half-written file), then record the
        id.  The caller holds the lock (build() below).  `force`: compile the cached objects again too."""
        bid = self.source_hash()
        tmp = self.lib + ".tmp.%d" % os.getpid()
        if self.obj_dir is None:
            cmd = [_hipcc()] + FLAGS + ['-D%s="%s"' % (self.macro, bid), "-shared", "-o", tmp] + \
                  [os.path.join(CSRC, s) for s in self.sources]
        else:
            from concurrent.futures import ThreadPoolExecutor
            os.makedirs(self.obj_dir, exist_ok=True)
            jobs = jobs or int(os.environ.get("GX_BUILD_JOBS", "0")) or min(len(self.sources), os.cpu_count() or 1)
            with ThreadPoolExecutor(max_workers=jobs) as ex:
                list(ex.map(lambda src: self._compile(src, bid, force, verbose), self.sources))
            cmd = [_hipcc(), "-shared", "-fPIC", "--offload-arch=gfx950", "-o", tmp] + [self._obj(s) for s in self.sources]
        _run(cmd, verbose)
        os.replace(tmp, self.lib)
        with open(self.build_id_file + ".tmp", "w") as f:
            f.write(bid + "\n")
        os.replace(self.build_id_file + ".tmp", self.build_id_file)
        return self.lib


def _hipcc():
    return os.environ.get("HIPCC", "hipcc")


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


# libguardx_hip.so: the engine.  Its hash covers the per-source flags as well; the others' covers FLAGS alone.
MAIN = Library("hip", "GX_BUILD_ID", SOURCES, HEADERS, "BUILD_ID", obj_dir=os.path.join(LIB_DIR, "obj"),
               per_source_flags=PER_SOURCE_FLAGS)
LIB = MAIN.lib
source_hash, built_id, needs_build = MAIN.source_hash, MAIN.built_id, MAIN.needs_build

# The other libraries, one translation unit each: the batched cost critic, the state-wise (SCPO), the safety-layer, the
# USL, the LPG and the one-episode policy step; the math probe, which only the tests call (the fp32 primitives of
# gx_device.h and gx_policy.h one by one, tests/test_gpu_math64.py); and epstats (the learners' EpRet / EpCost / EpLen
# bookkeeping, guardx_amd/epstats.py), which includes none of the project's device headers.
# Each is a library of its own with its own build identity, so that it leaves the sources, the flags and the build id of
# libguardx_hip.so -- and the profiles taken on that build -- alone.
_SIDE_HEADERS = ["gx_device.h", "gx_policy.h"]
# what the five step libraries share (sizes, the transpose kernel, the MFMA chain, the sample / log-prob block, the host
# side's checks, dispatch and launches): not the critic library's, whose build id does not cover it
_STEP_HEADERS = _SIDE_HEADERS + ["gx_step.h"]
# c_net's device code and the front end of its step and probe kernels, shared by the two learners that correct the action
# with a Q critic (and by them alone: the other libraries' build ids do not cover them)
_Q_HEADERS = _STEP_HEADERS + ["gx_qcritic.h", "gx_qstep.h"]


def _side(key, macro, headers):
    return Library(key, macro, ["gx_%s.hip" % key], headers + [os.path.join("..", "..", "include", "guardx_%s.h" % key)],
                   key.upper() + "_BUILD_ID")


# in build order, after MAIN
LIBRARIES = {lib.key: lib for lib in (
    _side("critic", "GXC_BUILD_ID", _SIDE_HEADERS),
    _side("statewise", "GXS_BUILD_ID", _STEP_HEADERS),
    _side("safelayer", "GXL_BUILD_ID", _STEP_HEADERS),
    _side("usl", "GXU_BUILD_ID", _Q_HEADERS),
    _side("lpg", "GXP_BUILD_ID", _Q_HEADERS),
    _side("episode", "GXE_BUILD_ID", _STEP_HEADERS),
    _side("mathprobe", "GXM_BUILD_ID", _SIDE_HEADERS),
    _side("epstats", "GXT_BUILD_ID", []),
)}

# What works on the learner's batch after collection: fisher (the TRPO family's Fisher-vector product and cg,
# guardx_amd/fisher.py).  The same Library class, built after LIBRARIES and looked up beside it
# (guardx_amd/_sidelib.py).  A mapping of its own only because tests/test_build_identity.py pins list(LIBRARIES) to the
# nine libraries it records: folding the two mappings together waits for a pull request that may touch that test.
# The same holds one step on: tests/test_fisher_host.py pins list(LEARNER_LIBRARIES) to fisher and every_library() to
# MAIN and these two mappings, so what came after it -- linesearch (the TRPO family's backtracking line search,
# guardx_amd/linesearch.py) -- is a third mapping, UPDATE_LIBRARIES, reached through all_libraries().
# And once more: tests/test_linesearch_host.py pins list(UPDATE_LIBRARIES) to linesearch and all_libraries() to the eleven
# libraries up to it, so vfit (the critics' Adam fit, guardx_amd/vfit.py) is a fourth mapping, FIT_LIBRARIES, built last and
# reached through fit_libraries().
# And a fourth time: tests/test_vfit_host.py pins list(FIT_LIBRARIES) to vfit and fit_libraries() to the twelve libraries up
# to it, so pgrad (the surrogate gradients g and b and CPO's step direction, guardx_amd/pgrad.py) is a fifth mapping,
# GRAD_LIBRARIES, built last and reached through grad_libraries().
# And a fifth time: tests/test_pgrad_host.py pins list(GRAD_LIBRARIES) to pgrad and grad_libraries() to the thirteen libraries up
# to it, so pifit (the PPO family's Adam fit of the actor on the clipped surrogate, guardx_amd/pifit.py) is a sixth mapping,
# ACTOR_LIBRARIES, built last and reached through actor_libraries().
# And a sixth time: tests/test_pifit_host.py pins list(ACTOR_LIBRARIES) to pifit and actor_libraries() to the fourteen libraries
# up to it, so cfit (the safety critics' Adam fit under row weights, guardx_amd/cfit.py) is a seventh mapping, SAFETY_LIBRARIES,
# built last and reached through safety_libraries(): that is the list build() builds and the bindings look up.
LEARNER_LIBRARIES = {lib.key: lib for lib in (
    _side("fisher", "GXF_BUILD_ID", _SIDE_HEADERS),
)}

UPDATE_LIBRARIES = {lib.key: lib for lib in (
    _side("linesearch", "GXB_BUILD_ID", _SIDE_HEADERS),
)}

FIT_LIBRARIES = {lib.key: lib for lib in (
    _side("vfit", "GXV_BUILD_ID", _SIDE_HEADERS),
)}


GRAD_LIBRARIES = {lib.key: lib for lib in (
    _side("pgrad", "GXG_BUILD_ID", _SIDE_HEADERS),
)}


ACTOR_LIBRARIES = {lib.key: lib for lib in (
    _side("pifit", "GXA_BUILD_ID", _SIDE_HEADERS),
)}


SAFETY_LIBRARIES = {lib.key: lib for lib in (
    _side("cfit", "GXQ_BUILD_ID", _SIDE_HEADERS),
)}


def every_library():
    """in build order"""
    return [MAIN] + list(LIBRARIES.values()) + list(LEARNER_LIBRARIES.values())


def all_libraries():
    """every_library() and UPDATE_LIBRARIES, in build order"""
    return every_library() + list(UPDATE_LIBRARIES.values())


def fit_libraries():
    """all_libraries() and FIT_LIBRARIES, in build order"""
    return all_libraries() + list(FIT_LIBRARIES.values())


def grad_libraries():
    """fit_libraries() and GRAD_LIBRARIES, in build order"""
    return fit_libraries() + list(GRAD_LIBRARIES.values())


def actor_libraries():
    """grad_libraries() and ACTOR_LIBRARIES, in build order"""
    return grad_libraries() + list(ACTOR_LIBRARIES.values())


def safety_libraries():
    """actor_libraries() and SAFETY_LIBRARIES, in build order: every library there is; what build() builds and the bindings
    look up"""
    return actor_libraries() + list(SAFETY_LIBRARIES.values())


def build(force=False, verbose=False, jobs=None):
    """Build what needs building under an inter-process lock (several ranks importing at once build once).  Every
    library of safety_libraries(); returns the path of libguardx_hip.so."""
    import fcntl
    os.makedirs(LIB_DIR, exist_ok=True)
    with open(LOCK_FILE, "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            for lib in safety_libraries():
                if force or lib.needs_build():
                    lib.build(verbose, jobs, force)
            return LIB
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print("build id", built_id())
    for side in safety_libraries()[1:]:
        print(side.key, "build id", side.built_id())
