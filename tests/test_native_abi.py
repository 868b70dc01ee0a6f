"""The C-ABI library loads on a CPU-only host and exports every symbol that
include/guardx.h declares (no compute calls without a GPU)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "guardx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gx_[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def native():
    from guardx_amd import build, _native
    build.build()
    return _native


def test_every_declared_symbol_is_exported_and_bound(native):
    lib = native.load()
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in guardx.h but not exported"
        assert n in native.SYMBOLS, f"{n} has no ctypes prototype"
    assert sorted(native.SYMBOLS) == names


def test_abi_version_and_struct_size(native):
    lib = native.load()
    assert lib.gx_abi_version() == 2
    from guardx_amd import build as gx_build
    assert lib.gx_build_id().decode() == gx_build.source_hash() == gx_build.built_id()   # the library is this tree's
    cfg = native.GxConfig()
    h = C.c_void_p()
    cfg.struct_size = 4                       # wrong size is rejected before any HIP call
    assert lib.gx_create(C.byref(cfg), C.byref(h)) == native.GX_ERR_ARG
    assert b"struct_size" in lib.gx_last_error()
    # the right size passes the ABI check (and then fails on the arguments / missing device)
    cfg.struct_size = C.sizeof(native.GxConfig)
    rc = lib.gx_create(C.byref(cfg), C.byref(h))
    assert rc != native.GX_OK and b"struct_size" not in lib.gx_last_error()


def test_oracle_and_product_config_structs_have_the_same_layout(native):
    from oracle import gxo
    a = [(n, t) for n, t in native.GxConfig._fields_]
    b = [(n, t) for n, t in gxo.Config._fields_]
    assert [t for _, t in a] == [t for _, t in b]
    assert C.sizeof(native.GxConfig) == C.sizeof(gxo.Config)


def test_null_arguments_are_errors_not_crashes(native):
    lib = native.load()
    assert lib.gx_create(None, None) == native.GX_ERR_ARG
    assert lib.gx_reset(None, None, None) == native.GX_ERR_ARG
    assert lib.gx_step(None, None, None, None, None, None, None, None) == native.GX_ERR_ARG
    assert lib.gx_reset_done(None, None, None, None) == native.GX_ERR_ARG
    assert lib.gx_obs_dim(None) == -1
    assert lib.gx_tape_floats(None, 1, None, None, None) == native.GX_ERR_ARG
    assert lib.gx_rollout_tape(None, 1, None, None, None, None) == native.GX_ERR_ARG
    assert lib.gx_expand_tape(None, 1, None, 0, None, None) == native.GX_ERR_ARG
    assert lib.gx_destroy(None) == native.GX_OK


def test_integration_stub_matches_the_header():
    """the ctypes structure printed in INTEGRATION.md (what a reference maintainer would paste) has the
    fields of include/guardx.h:gx_config, in order, and the size the library checks"""
    import ctypes as C
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    block = doc[doc.index("class gx_config(C.Structure):"):]
    block = block[:block.index("\n\n")]
    ns = {"C": C}
    exec(block, ns)
    stub = ns["gx_config"]
    from guardx_amd import _native
    assert [f[0] for f in stub._fields_] == [f[0] for f in _native.GxConfig._fields_]
    assert C.sizeof(stub) == C.sizeof(_native.GxConfig)
    hdr = open(os.path.join(root, "include", "guardx.h")).read()
    body = hdr[hdr.index("typedef struct gx_config {"):hdr.index("} gx_config;")]
    names = re.findall(r"^\s+(?:const\s+)?(?:int32_t|uint32_t|float|double)\*?\s+(\w+)", body, re.M)
    flat = []
    for f in stub._fields_:
        flat.append(f[0])
    assert names == flat, (names, flat)


def test_no_kernel_reads_the_aql_packet():
    """A kernel whose descriptor enables the dispatch / queue pointer reads workgroup sizes from the AQL packet
    (host memory) at run time -- what AMDGPUPromoteAlloca makes of a private array it moves to LDS.  That scalar
    load cost every launch of the round-1 lane-group kernels ~12 us (profiles/history/r02_stamps_*.log)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_descriptors as kd
    from guardx_amd import _native
    _native.load()
    ks = kd.library_kernels(_native.LIB_PATH)
    assert len(ks) > 150 and any("group_rollout_kernel" in k for k in ks)
    bad = [k for k, v in ks.items() if v["dispatch_ptr"] or v["queue_ptr"]]
    assert not bad, bad[:3]
    # the Point / Swimmer lane-group kernels keep their state in registers: no scratch
    for k, v in ks.items():
        if "group_rollout_kernel" in k and ("PointRobot" in k or "SwimmerRobot" in k) and k.endswith("ELi0EEEvNS_6ParamsENS_11RolloutArgsENS_10PolicyArgsEP15HIP_vector_typeIfLj4EES8_S8_"):
            assert v["scratch"] == 0, (k, v)


def test_lane_group_steps_contain_no_call():
    """The Ant's and the Walker's lane-group steps are inlined into group_rollout_kernel: no s_swappc_b64 in any
    open-loop lane-group kernel.  History: with the step as a noinline callee, LLVM's
    inter-procedural register allocation let the callee use the VGPR lanes in which the caller parks spilled exec
    masks -- masked-off lanes then stored through garbage addresses after an in-kernel reset_done (rounds 1-2, two call
    sites; round 3 again with ONE call site as soon as the Walker's callee grew).  Rounds 1-2 could not inline the
    Walker's step (hipcc 7.2 miscompiled the 15k-instruction body); the round-3 form, a third shorter, inlines and
    passes every parity test and the soak.  A compiler that outlines a step again shows up here, before it can show up
    as a wrong number on the GPU; the compiler's version is part of the library's identity (gx_build_compiler)."""
    import shutil
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_descriptors as kd
    from guardx_amd import _native, build as gx_build
    lib = _native.load()
    assert lib.gx_build_compiler().decode() == gx_build.compiler_id()
    objdump = shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        import torch
        if torch.cuda.is_available():      # on a GPU box this check guards a known compiler hazard: never silently skipped
            pytest.fail("llvm-objdump not found (looked on PATH and in /opt/rocm/lib/llvm/bin)")
        pytest.skip("llvm-objdump not available")
    calls = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (triple, data) in enumerate(kd.code_objects(_native.LIB_PATH)):
            if "gfx950" not in triple or data[:4] != b"\x7fELF":
                continue
            names = [k for k in kd.descriptors(data)
                     if "group_rollout_kernel" in k and ("WalkerRobot" in k or "AntRobot" in k) and "ELi0EEEvNS_6Params" in k]
            if not names:
                continue
            path = os.path.join(tmp, f"co{i}.elf")
            with open(path, "wb") as f:
                f.write(data)
            for n in names:
                asm = subprocess.run([objdump, "-d", "--mcpu=gfx950", "--disassemble-symbols=" + n, path],
                                     capture_output=True, text=True, check=True).stdout
                assert asm.count("s_endpgm") >= 1, n
                calls[n] = asm.count("s_swappc_b64")
    assert sum("WalkerRobot" in n for n in calls) >= 4 and sum("AntRobot" in n for n in calls) >= 4, sorted(calls)
    assert set(calls.values()) == {0}, {k: v for k, v in calls.items() if v}


# ---------------------------------------------------------------------------------------------------------------------
# libguardx_mathprobe.so (include/guardx_mathprobe.h): the tests' own library, held to what the side libraries are held to
# (its build identity and ABI: tests/test_build_identity.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mathprobe_lib():
    from guardx_amd import build, _mathprobe_native
    build.build()                       # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    return _mathprobe_native.load()     # refuses a library whose build id is not the tree's


def test_mathprobe_bad_arguments_are_errors_not_crashes(mathprobe_lib):
    from guardx_amd import _mathprobe_native as n
    lib = mathprobe_lib
    fake = 4096                         # never dereferenced: every call below returns before any HIP call
    for fn in range(n.GXM_FN_COUNT):
        assert lib.gxm_eval(fn, -1, fake, fake, fake, fake, None) == n.GXM_ERR_ARG
        assert lib.gxm_eval(fn, 4, None, fake, fake, fake, None) == n.GXM_ERR_ARG
        assert lib.gxm_eval(fn, 4, fake, fake, None, fake, None) == n.GXM_ERR_ARG and b"null pointer" in lib.gxm_last_error()
        assert lib.gxm_eval(fn, 0, fake, fake, fake, fake, None) == n.GXM_OK                  # n == 0: nothing to do
        needs_y, needs_o1 = fn in (n.GXM_FN_ATAN2, n.GXM_FN_DIV), fn in (n.GXM_FN_SINCOS, n.GXM_FN_SINCOS_FINITE)
        assert lib.gxm_eval(fn, 0, fake, None, fake, fake, None) == (n.GXM_ERR_ARG if needs_y else n.GXM_OK)
        assert lib.gxm_eval(fn, 0, fake, fake, fake, None, None) == (n.GXM_ERR_ARG if needs_o1 else n.GXM_OK)
    for fn in (-1, n.GXM_FN_COUNT, 1 << 20):
        assert lib.gxm_eval(fn, 4, fake, fake, fake, fake, None) == n.GXM_ERR_ARG and b"unknown fn" in lib.gxm_last_error()
    assert lib.gxm_normal_pair(1, 2, -1, fake, fake, fake, fake, None) == n.GXM_ERR_ARG
    for i in range(4):
        p = [fake] * 4
        p[i] = None
        assert lib.gxm_normal_pair(1, 2, 4, *p, None) == n.GXM_ERR_ARG, i
    assert lib.gxm_normal_pair(0xFFFFFFFF, 0, 0, fake, fake, fake, fake, None) == n.GXM_OK
    for pair in (-1, n.GXM_PAIR_COUNT):
        assert lib.gxm_sweep(pair, 0, 4, fake, None) == n.GXM_ERR_ARG and b"unknown pair" in lib.gxm_last_error()
    for pair in range(n.GXM_PAIR_COUNT):
        assert lib.gxm_sweep(pair, 0, 4, None, None) == n.GXM_ERR_ARG
        assert lib.gxm_sweep(pair, 1, 1 << 32, fake, None) == n.GXM_ERR_ARG and b"2^32" in lib.gxm_last_error()
        assert lib.gxm_sweep(pair, 0xFFFFFFFF, 2, fake, None) == n.GXM_ERR_ARG
        assert lib.gxm_sweep(pair, 0, (1 << 32) + 1, fake, None) == n.GXM_ERR_ARG
        assert lib.gxm_sweep(pair, 0xFFFFFFFF, 0, fake, None) == n.GXM_OK                      # count == 0: nothing to do
