"""include/polaris_math.h as the product's build compiled it for gfx950, against the same header compiled by the oracle's build for
the host: every built-in the kernels call, over every binary32 input (unary) or the edge grid and 2^28 draws (binary / ternary),
must give the same bits on both sides (polaris_hip_selftest_builtins vs polaris_oracle_builtins, polaris_amd/csrc/builtin_probe.h).

The libm sweep (tests/test_builtins_sweep.py) ties the host side to double-precision glibc; this file ties the device side to the
host side, so a compiler upgrade or a dropped flag of polaris_amd/csrc/Makefile (-ffp-contract=off,
-fhip-fp32-correctly-rounded-divide-sqrt, -fno-gpu-flush-denormals-to-zero) that changes a device result on inputs no test scene
produces is still caught.  Both sides fingerprint each chunk of 2^20 inputs; a chunk that differs is fetched in full from both, and
the failure names its first differing input.

Outside a function's domain (builtin_probe.h pb_in_domain) C++ leaves some conversions undefined; the fingerprints keep those
inputs apart, so a failure says on which side of the domain it lies.  Both builds agree there too today, and are held to it."""
import time

import numpy as np
import pytest

from conftest import make_hip_tracer
from polaris_amd import ctypes_api as T

pytestmark = pytest.mark.gpu

F = np.float32
CH = T.BUILTIN_CHUNK
BATCH = T.SELFTEST_MAX_RESULTS // CH   # chunks per raw fetch


@pytest.fixture(scope="module")
def tracer(built):
    from polaris_amd import scenes

    tr = make_hip_tracer(scenes.SCENES["cornell-diffuse"](), 8, 8)
    yield tr
    tr.Close()


def _raw_mismatches(tracer, oracle, fn, chunks):
    """(indices, inputs (k, 3), device bits, host bits) of every input of the given chunks whose results differ."""
    idx, xyz, dev_bits, host_bits = [], [], [], []
    chunks = sorted(chunks)
    n = T.builtin_inputs(fn)
    k = 0
    while k < len(chunks):   # runs of consecutive chunks, BATCH at a time
        j = k
        while j + 1 < len(chunks) and chunks[j + 1] == chunks[j] + 1 and j + 1 - k < BATCH:
            j += 1
        first = chunks[k] * CH
        count = min(n, (chunks[j] + 1) * CH) - first
        dev = tracer.selftest_builtins(fn, first, count, results=True)
        host, inputs = oracle.builtins(fn, first, count, results=True)
        bad = np.nonzero(dev != host)[0]
        idx.append(first + bad)
        xyz.append(inputs[bad])
        dev_bits.append(dev[bad])
        host_bits.append(host[bad])
        k = j + 1
    cat = lambda a, dt: np.concatenate(a) if a else np.zeros(0, dt)  # noqa: E731
    return cat(idx, np.int64), (np.concatenate(xyz) if xyz else np.zeros((0, 3), F)), cat(dev_bits, np.uint32), cat(host_bits, np.uint32)


@pytest.mark.parametrize("name", list(T.BUILTINS))
def test_device_build_equals_host_build(tracer, oracle, name):
    fn = T.BUILTINS[name]
    t0 = time.perf_counter()
    dev = tracer.selftest_builtins(fn)
    t1 = time.perf_counter()
    host = oracle.builtins(fn)
    t2 = time.perf_counter()
    print(f"\nbuiltins {name}: {T.builtin_inputs(fn)} inputs, device {t1 - t0:.3f} s, host {t2 - t1:.3f} s")
    assert dev.shape == host.shape == (-(-T.builtin_inputs(fn) // CH), 2)
    assert (host[:, 0] | host[:, 1]).all()   # (every chunk has results: a fingerprint of 0 would mean nothing was summed)

    inside = np.nonzero(dev[:, 0] != host[:, 0])[0]
    if inside.size:
        i, xyz, d, h = _raw_mismatches(tracer, oracle, fn, inside[:1])
        assert i.size, f"{name}: chunk {inside[0]}'s in-domain fingerprints differ but no result does"
        x, y, z = (float(v) for v in xyz[0])
        pytest.fail(f"{name}: {inside.size} chunks differ inside the domain; first differing input #{i[0]} (x={x!r}, y={y!r}, z={z!r}, "
                    f"bits 0x{xyz[0:1].view(np.uint32)[0, 0]:08x}): device 0x{d[0]:08x}, host 0x{h[0]:08x} ({i.size} in that chunk)")

    # Outside the domain C++ leaves some conversions undefined (pm__reduce_pio4's uint32_t of |x| * 4 / pi from ~3.4e9 on and of
    # NaN, pm_exp's int32_t of NaN, the tone-map byte of NaN), yet on this toolchain both builds agree on every such input too:
    # a difference here is a change of compiler behaviour to look at (and to confine to its region here), not noise.
    outside = np.nonzero(dev[:, 1] != host[:, 1])[0]
    if outside.size:
        i, xyz, d, h = _raw_mismatches(tracer, oracle, fn, outside[:1])
        pytest.fail(f"{name}: host and device differ outside the domain in {outside.size} chunks; first: input #{i[0]} {xyz[0].tolist()}: "
                    f"device 0x{d[0]:08x}, host 0x{h[0]:08x}")


def test_selftest_entry_refuses_bad_arguments(tracer):
    from polaris_amd.tracer import TracerError

    for fn, first, count in ((len(T.BUILTINS), 0, CH), (0, 1, CH), (0, 2 ** 32 - CH, 2 * CH), (T.BUILTINS["pow"], 0, 2 ** 30)):
        with pytest.raises(TracerError):
            tracer.selftest_builtins(fn, first, count)
    with pytest.raises(TracerError):
        tracer.selftest_builtins(0, 0, T.SELFTEST_MAX_RESULTS + 1, results=True)
    # a partial last chunk and a raw window agree with the fingerprints' own chunking
    fn = T.BUILTINS["mix"]
    last = T.builtin_inputs(fn) // CH * CH
    assert tracer.selftest_builtins(fn, last).shape == (1, 2)
    assert tracer.selftest_builtins(fn, last, results=True).size == T.builtin_inputs(fn) - last
