"""Build libcozk.so (all HIP kernels + the C ABI) for gfx950 with hipcc, the test-only primitive harness
tests/native/libcozk_prims.so (build_prims) and the test-only host programs of HOST_PROGRAMS (build_host_program).
Cross-compiles without a GPU."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libcozk.so")
PRIMS_SRC = os.path.join(os.path.dirname(HERE), "tests", "native", "prims.hip")
PRIMS_OUT = os.path.join(os.path.dirname(HERE), "tests", "native", "libcozk_prims.so")
NATIVE = os.path.join(os.path.dirname(HERE), "tests", "native")
# stand-alone host programs (their own main, no device code, no project library), each driven by one CPU test: command-line flag -> name
#   layer_tail_check     csrc/host/layer_tail.hpp, the host tail of the dense layer rounds (tests/test_layer_tail_host.py)
#   bytecode_leaf_check  csrc/bytecode_arith.hip.hpp, the word arithmetic of the bytecode leaf kernels (tests/test_bytecode_leaf_host.py)
#   msm_schedule_check   csrc/host/msm_schedule.hpp, the launch schedule of the batched MSM (tests/test_msm_schedule_host.py)
HOST_PROGRAMS = {"--layer-tail": "layer_tail_check", "--bytecode-leaf-check": "bytecode_leaf_check", "--msm-schedule-check": "msm_schedule_check"}
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
SOURCES = ["capi.hip", "msm.hip", "poly.hip", "harness.hip", "shm_hub.hip", "ring.hip", "shamir.hip", "lasso_witness.hip", "rw_memory_witness.hip", "rw_memory_leaves.hip", "ts_range_witness.hip", "bytecode_leaves.hip"]
HEADERS = ["bytecode_arith.hip.hpp", os.path.join("host", "layer_tail.hpp"), os.path.join("host", "msm_schedule.hpp"), os.path.join("host", "spartan_pub_workers.hpp"), "fr9.hip.hpp", "fr9_consts.inc", os.path.join("host", "memcheck_steps.hpp"), os.path.join("host", "flow_harness.hpp"), os.path.join("host", "ts_range_proof.hpp"), os.path.join("host", "rw_memory_proof.hpp"), os.path.join("host", "rw_memory_proof_rep3.hpp"), os.path.join("host", "bytecode_proof.hpp"), os.path.join("host", "jolt_r1cs.hpp"), os.path.join("host", "spartan_jolt.hpp"), "spartan_inner.inc", "ff.hip.hpp", "prf.hip.hpp", "ff_macc.inc", "ff_mul2.inc", "ec.hip.hpp", "fq9.hip.hpp", "fq9_consts.inc", "fq9_mac.inc", "fq9_mul.inc", "common.hpp", "lasso_walk.hip.hpp", "radix_pass.hip.hpp", "poly.hip.hpp", "toggle_layer.inc", "spartan_group.inc", "sparse_layer.inc", "primary_sumcheck.inc", "primary_group.inc", "shamir_deal.hip.hpp", "spartan_outer.inc", "outer_group.inc", "logup.inc", "compact_open.inc", "output_check.inc", os.path.join("host", "memory_proof.hpp"), os.path.join("host", "memory_proof_rep3.hpp"), os.path.join("host", "wire.hpp"), os.path.join("host", "net.hpp"), os.path.join("host", "prover.hpp"), os.path.join("host", "sparse_rule.hpp"), os.path.join("host", "split.hpp"), os.path.join("host", "split_harness.hpp"), os.path.join("host", "spartan_harness.hpp"), os.path.join("host", "lookups_harness.hpp"), os.path.join("host", "outer_harness.hpp"), os.path.join("host", "runner.hpp"), os.path.join("host", "shamir_gp.hpp"), os.path.join("host", "shamir_harness.hpp"), os.path.join("host", "shamir_spartan.hpp"), os.path.join("host", "shamir_jolt_spartan.hpp"), os.path.join("host", "shamir_primary.hpp"), os.path.join("..", "..", "include", "cozk.h")]


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in HEADERS]
    objs = []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    procs = []
    for s in srcs:
        o = os.path.join(HERE, "build", os.path.basename(s) + ".o")
        objs.append(o)
        if force or _newer(o, deps):
            cmd = ["hipcc"] + HIPCC_FLAGS + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
    if force or procs or _newer(OUT, objs):
        cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs + ["-ldl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    build_prims(force, verbose)
    for name in HOST_PROGRAMS.values():
        build_host_program(name, force, verbose)
    return OUT


def build_prims(force=False, verbose=True):
    """the test-only harness that puts the headers' field, curve and 9 x 29 operations behind element-wise kernels and host
    wrappers (tests/test_gpu_prims.py, tests/test_host_prims.py); rebuilt when it or any header changes"""
    if force or _newer(PRIMS_OUT, [PRIMS_SRC] + [os.path.join(CSRC, h) for h in HEADERS]):
        tmp = PRIMS_OUT[:-3] + ".tmp.so"
        cmd = ["hipcc"] + HIPCC_FLAGS + ["-shared", PRIMS_SRC, "-o", tmp]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        os.replace(tmp, PRIMS_OUT)  # a killed compile leaves no library that looks fresh
    return PRIMS_OUT


def build_host_program(name, force=False, verbose=True, extra_flags=(), out=None):
    """tests/native/<name>.hip -> tests/native/<name>, one of HOST_PROGRAMS; rebuilt when it or any header changes.  extra_flags / out:
    another build of the same program, e.g. one with host sanitizers (-Xarch_host -fsanitize=address,undefined)"""
    src = os.path.join(NATIVE, name + ".hip")
    out = out or os.path.join(NATIVE, name)
    if force or _newer(out, [src] + [os.path.join(CSRC, h) for h in HEADERS]):
        tmp = out + ".tmp"
        cmd = ["hipcc"] + HIPCC_FLAGS + list(extra_flags) + [src, "-o", tmp]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        os.replace(tmp, out)
    return out


if __name__ == "__main__":
    if "--prims" in sys.argv:
        build_prims(force="--force" in sys.argv)
    elif any(flag in sys.argv for flag in HOST_PROGRAMS):
        for flag, name in HOST_PROGRAMS.items():
            if flag in sys.argv:
                build_host_program(name, force="--force" in sys.argv)
    else:
        build(force="--force" in sys.argv)
