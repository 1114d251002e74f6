"""CPU test of the one stand-alone host helper of the sparse pair layers, the storage rule and the hand-over decision of
co-zkvms_amd/csrc/host/sparse_rule.hpp: tests/native/sparse_rule_check.cpp is compiled as a host program (no device code, no
project library) into a temporary directory and run; it checks the rule against the byte counts it stands for and that every
sparse layer hands over after at least one round with at least one dense round left."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_storage_rule_and_handover_hold_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "sparse_rule_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "sparse_rule_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "sparse_rule_check: ok" in out.stdout, out.stdout + out.stderr
