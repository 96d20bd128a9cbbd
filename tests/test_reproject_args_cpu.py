"""The argument rules of the four CPU reprojection entries (polaris_amd/host/temporal.cpp: polaris_host_reproject, _reproject_moments,
_reproject_motion, _reproject_deform), which all go through check_reproject of polaris_amd/csrc/reproject_io.h -- the function the
device entries refuse with too (tests/test_gpu_reproject_entries.py walks the same table).

Bars: a valid call succeeds on every entry, and every single violation of tests/reproject_args.py that applies to an entry returns
POLARIS_E_BAD_ARGUMENT -- before anything behind a plane pointer is touched: the frame rows pass pointers nothing may dereference --
which polaris_amd.host_api raises as ValueError; the values at the bounds are accepted."""
import numpy as np
import pytest

import reproject_args as RA
from conftest import bits

ENTRIES = list(RA.ORDER)
# (entry, with the moments group): the plain entry has none, polaris_host_reproject_moments demands it, the other two take it or not
CALLS = [("reproject", False), ("reproject_moments", True), ("reproject_motion", False), ("reproject_motion", True),
         ("reproject_deform", False), ("reproject_deform", True)]


@pytest.fixture(scope="module")
def host(built):
    from polaris_amd import host_api

    host_api.load()
    return host_api


def call(host, entry, d):
    return RA.raw(getattr(host.load(), "polaris_host_" + entry), entry, d)


def wrapper_args(entry, d):
    """The call as polaris_amd.host_api's wrapper of the entry takes it: (positional, keyword)."""
    names = [k for k in RA.ORDER[entry] if k not in ("W", "H", "n", "nt", "p", "prior", "prior2") and (k != "hvar" or entry == "reproject_moments")]
    kw = dict(max_history=d["p"].max_history, normal_threshold=d["p"].normal_threshold, depth_threshold=d["p"].depth_threshold)
    if "hvar" in RA.ORDER[entry] and entry != "reproject_moments":
        kw["history_variance"] = d["hvar"]
    return [d[k] for k in names], kw


@pytest.mark.parametrize("entry,moments", CALLS)
def test_a_valid_call_succeeds(host, entry, moments):
    d = RA.valid(entry, moments)
    assert call(host, entry, d) == 0
    assert (d["prior"][..., 3] > 0).sum() >= 8, "the engineered frame finds history"
    args, kw = wrapper_args(entry, d)
    got = getattr(host, entry)(*args, **kw)       # the wrapper marshals the same call
    got = got if isinstance(got, tuple) else (got,)
    want = (d["prior"], d["prior2"]) if moments else (d["prior"],)
    assert len(got) == len(want) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, want))


@pytest.mark.parametrize("entry,moments", CALLS)
def test_every_single_violation_is_refused(host, entry, moments):
    rows = RA.rows(entry)
    assert len(rows) >= 23
    for name, change in rows:
        d = RA.violated(entry, change, moments)
        assert call(host, entry, d) == RA.BAD_ARGUMENT, f"{entry} (moments {moments}): {name}"
        for k in ("prior", "prior2"):             # a refused call writes nothing
            assert not isinstance(d.get(k), np.ndarray) or not d[k].any(), f"{entry}: {name} wrote {k}"


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_bounds_themselves_are_accepted(host, entry):
    for name, change in RA.ACCEPTED:
        assert call(host, entry, RA.violated(entry, change)) == 0, f"{entry}: {name}"


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_wrapper_raises_value_error(host, entry):
    """Where the wrapper can state the violation -- the params, empty tables, null or empty vertices -- the library's refusal reaches
    the caller as ValueError."""
    fn = getattr(host, entry)
    args, kw = wrapper_args(entry, RA.valid(entry))
    fn(*args, **kw)
    for bad in (dict(max_history=4097), dict(normal_threshold=float("nan")), dict(depth_threshold=2e6)):
        with pytest.raises(ValueError):
            fn(*args, **{**kw, **bad})
    if entry in ("reproject_motion", "reproject_deform"):
        empty = list(args)
        empty[11], empty[12] = args[11][:0], args[12][:0]                      # n_instances = 0
        with pytest.raises(ValueError):
            fn(*empty, **kw)
    if entry == "reproject_deform":
        for v, pv in ((args[14][:0], args[15][:0]), (None, args[15]), (args[14], None)):
            with pytest.raises(ValueError):
                fn(*args[:14], v, pv, **kw)
