"""CPU test of the transition behind a change of the option "guide_specular" (polaris_amd/csrc/frame_sync.h,
SyncState::guide_rule_changed): the G-buffer and the history go, the instance table stays, nothing is swapped."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "tools", "guide_rule_check.cpp")
LIB = os.path.join(BUILD, "libguide_rule_check.so")
GBUFFER, PRIOR, HAVE_HISTORY, HISTORY_M2, TEMPORAL_SYNCED, VARIANCE_SYNCED = 1, 2, 4, 8, 16, 32


def test_guide_rule_changed_drops_the_gbuffer_and_the_history_and_keeps_the_instance_table():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "polaris_amd", "csrc", "frame_sync.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "polaris_amd", "csrc"), SRC, "-o", LIB])
    out = (C.c_int64 * 7)()
    C.CDLL(LIB).guide_rule_check(out)
    before, after, prior_refused, table_kept, swaps, recompute_prior, from_history = list(out)
    assert before == GBUFFER | PRIOR | HAVE_HISTORY | HISTORY_M2 | TEMPORAL_SYNCED | VARIANCE_SYNCED
    assert after == 0
    assert prior_refused == 1 and table_kept == 1
    assert recompute_prior == 1 and from_history == 0      # the next temporal sync clears PRIOR: m = 0 everywhere
    assert swaps == 0                                       # nothing was synced under the new rule: nothing joins the history
