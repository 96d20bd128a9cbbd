"""Independent evidence for include/polaris_math.h -- the ONE definition of the OpenCL built-ins that the HIP
kernels, the CPU oracle and the compiled reference kernels (oracle/_ref) share.  Bit-equality between those three
says nothing about the built-ins themselves (a wrong pm_acos would be reproduced by all of them), so
tests/tools/builtin_sweep.cpp measures every function against double-precision glibc:

* unary functions over binary32 bit patterns (every 16th here; ALL 2^32 in the `gpu`-marked test, which needs the
  GPU box's core count, and in the committed profiles/r02_builtins_sweep.json), over the argument ranges the kernels
  use, held to the OpenCL 1.2 full-profile ULP bounds (section 7.4);
* binary / ternary functions on 1e8 random inputs plus a 24^3 grid of edge values (zeros, subnormals, 1 +- ulp,
  FLT_MAX, infinities, NaNs);
* exp on [-87, 88.72] and log over every positive finite input, held to what polaris_math.h promises (1.5 / 1.0 ulp), and
  exp's flush to 0 on (-104, -87) to an absolute error below 2^-125;
* every built-in whose result the specification fixes (fabs, floor, sign, min, max, fmin, fmax, clamp, mix,
  uint -> float conversion; sqrt, reciprocal and division, which are correctly rounded in this build) must equal an
  independent formulation bit for bit.
"""
import json
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "tools", "builtin_sweep.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "builtin_sweep")

ULP = ("sin", "cos", "atan", "acos", "pow_gamma", "atan2", "pow", "exp", "log")
EXACT = ("sqrt", "recip", "divide", "fabs", "floor", "sign", "min", "max", "fmin", "fmax", "clamp", "mix", "convert_float_uint")


@pytest.fixture(scope="module")
def sweep_exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "polaris_math.h"), os.path.join(ROOT, "polaris_amd", "csrc", "builtin_probe.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fopenmp", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "polaris_amd", "csrc"), SRC, "-o", EXE])
    return EXE


def check(d, exhaustive):
    for k in ULP:
        assert d[k]["max_ulp"] <= d[k]["opencl_bound_ulp"], (k, d[k])
        assert d[k]["inputs"] > 500_000, (k, d[k])
    # tighter than the OpenCL bounds: what polaris_math.h promises about itself
    for k, bound in (("sin", 2.0), ("cos", 2.0), ("atan", 3.0), ("acos", 2.0), ("exp", 1.5), ("log", 1.0)):
        assert d[k]["max_ulp"] <= bound, (k, d[k])
    # below -87 pm_exp flushes to 0 where exp(x) is still a (sub)normal float: an absolute error below 2^-125 (the denoiser's
    # weights take exp of (-inf, 0], exp_denoise; a weight that small is 0 beside the centre tap's 9/64 either way)
    assert d["exp_underflow"]["max_abs_err"] < 2.0 ** -125 and d["exp_underflow"]["inputs"] > 500, d["exp_underflow"]
    assert d["exp_denoise"]["inputs"] > 500_000, d["exp_denoise"]
    # near a zero crossing the ulp of the result shrinks without bound; there the absolute error is what matters (and the reference
    # only calls native_sin / native_cos, whose accuracy OpenCL leaves to the implementation): < 2^-23 everywhere on [-2pi, 2pi]
    for k in ("sin_all", "cos_all"):
        assert d[k]["max_abs_err"] < 2.0 ** -23, (k, d[k])
    for k in EXACT:
        assert d[k]["mismatches"] == 0 and d[k]["inputs"] > 1_000_000, (k, d[k])
    if exhaustive:
        assert d["stride"] == 1 and d["atan"]["inputs"] == 2 * 0x7F800000  # every finite binary32 value
        assert d["log"]["inputs"] == 0x7F7FFFFF  # every positive finite binary32 value, subnormals included
        assert d["sqrt"]["inputs"] == 2 ** 32 and d["recip"]["inputs"] == 2 ** 32 and d["convert_float_uint"]["inputs"] == 2 ** 32


def test_builtins_strided_sweep(sweep_exe):
    out = subprocess.run([sweep_exe, "16", "100000000"], capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-2000:]
    check(json.loads(out.stdout), exhaustive=False)


def test_committed_exhaustive_sweep_record():
    """profiles/r02_builtins_sweep.json: `builtin_sweep 1 100000000` (all 2^32 patterns) run in the build container."""
    check(json.load(open(os.path.join(ROOT, "profiles", "r02_builtins_sweep.json"))), exhaustive=True)


@pytest.mark.gpu
def test_builtins_exhaustive_sweep_on_the_gpu_box(sweep_exe):
    """All 2^32 inputs of every unary function.  No GPU involved: marked `gpu` because it wants the GPU box's host cores
    (~25 core-minutes; seconds on 256 threads, too long for the 8-CPU container's suite)."""
    if (os.cpu_count() or 1) < 32 and not os.environ.get("POLARIS_FULL_SWEEP"):
        pytest.skip("fewer than 32 host threads: the strided sweep and the committed record cover this machine")
    out = subprocess.run([sweep_exe, "1", "100000000"], capture_output=True, text=True, timeout=3000)
    assert out.returncode == 0, out.stderr[-2000:]
    check(json.loads(out.stdout), exhaustive=True)


def test_oracle_fingerprints_equal_a_plain_loop(sweep_exe, oracle):
    """The CPU side of the device self-test (polaris_oracle_builtins; tests/test_gpu_builtins_device.py compares the device with
    it) against `builtin_sweep fp`, which calls the same pm_* functions in a plain loop: a wrong entry of builtin_probe.h's
    table, chunking or summation -- which the device shares, and which would agree with itself -- fails here.  Every 256th
    chunk: 16 per unary function, the edge-grid chunk and the partial last chunk of the others."""
    from polaris_amd import ctypes_api as T

    out = subprocess.run([sweep_exe, "fp", "256"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    plain = json.loads(out.stdout)
    assert sorted(plain) == sorted(T.BUILTINS)
    for name, fn in T.BUILTINS.items():
        n = T.builtin_inputs(fn)
        assert sorted(int(c) for c in plain[name]) == list(range(0, -(-n // T.BUILTIN_CHUNK), 256)), name
        for c, want in plain[name].items():
            first = int(c) * T.BUILTIN_CHUNK
            got = oracle.builtins(fn, first, min(T.BUILTIN_CHUNK, n - first))
            assert got.shape == (1, 2)
            assert (int(got[0, 0]) + int(got[0, 1])) % 2 ** 64 == want, (name, c)
        fps = set(plain[name].values())
        assert 0 not in fps and len(fps) == len(plain[name]), name   # no two chunks of a function alike
