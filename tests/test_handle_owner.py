"""The owner of the tracer library's streams, events and inter-process mappings (DevHandle in
polaris_amd/csrc/device_mem.h) destroys every handle exactly once: tests/tools/handle_check.cpp
instantiates the template with counting fake destroy functions and runs, in an AddressSanitizer +
UBSan build (CPU only, no HIP runtime), through construction, reset, moves, a vector of owners and
an array member."""
import os
import subprocess

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "handle_check.cpp")
CSRC = os.path.join(ROOT, "polaris_amd", "csrc")
BIN = os.path.join(BUILD, "handle_check")


def test_handle_owner_destroys_each_handle_exactly_once():
    os.makedirs(BUILD, exist_ok=True)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC, SRC, "-o", BIN])
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.strip() == "handle_check: ok"
