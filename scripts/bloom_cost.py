"""What bloom (polaris_hip_set_bloom) costs a displayed sync (profiles/bloom_cost.txt).

    python scripts/bloom_cost.py [--reps 31] [--no-resources | --no-timing]

Resources (needs hipcc, no GPU): registers, LDS, scratch and the waves a SIMD holds of every k_bloom_* and k_display_bloom variant, from
the .amdhsa_ fields of the device listing of polaris_hip.hip compiled with the Makefile's flags.

Timing (needs the GPU): the Cornell box traced once at 1 spp at 512 x 512 and 1024 x 1024, then --reps plain syncs of the whole frame per
setting on a tracer with time_kernels = 1; per setting the median over the syncs of each timer.  Settings, all ACES with sRGB and
auto-exposure: bloom off ("display": k_display), bloom's defaults with "bloom_fused" 0 (one launch per level) and 1 (k_bloom_tail), each twice;
"bloom" is one bracket around every pyramid launch of a sync, "display" with bloom on is k_display_bloom.
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TIMERS = ("meter", "expose", "bloom", "display")


def resources():
    """One line per bloom kernel from the device listing."""
    csrc = os.path.join(ROOT, "polaris_amd", "csrc")
    flags = subprocess.check_output(["make", "-s", "-C", csrc, "-pn"], text=True)
    flags = re.search(r"^FLAGS := (.*)$", flags, re.M).group(1).replace("-shared", "").split()
    listing = subprocess.check_output([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "--cuda-device-only", "-S", "-o", "-",
                                       os.path.join(csrc, "polaris_hip.hip")], text=True)
    names, rows = [], []
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", listing, re.S):
        if re.search(r"k_(bloom_|display_bloom)", m.group(1)):
            names.append(m.group(1))
            rows.append({k: int(re.search(r"\.amdhsa_" + k + r" (\d+)", m.group(2)).group(1))
                         for k in ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size", "accum_offset")})
    pretty = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    lines = []
    for name, r in sorted(zip(pretty, rows)):
        vgpr = -(-r["next_free_vgpr"] // 8) * 8                                  # gfx950 allocates unified VGPRs in blocks of 8, 512 a SIMD lane
        lines.append(f"{name.split('(')[0].replace('void ', '')}: {r['next_free_vgpr']} VGPRs (ArchVGPRs {r['accum_offset']}), {r['next_free_sgpr']} SGPRs, "
                     f"LDS {r['group_segment_fixed_size']} B, scratch {r['private_segment_fixed_size']} B, {min(8, 512 // max(vgpr, 8))} waves/SIMD")
    return lines


def timing(reps):
    from conftest import make_hip_tracer
    from polaris_amd import ctypes_api as T
    from polaris_amd import scenes
    from test_gpu_denoise import sync, trace

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    display = dict(tone_operator=T.TONE_ACES, srgb=1, auto_exposure=1)
    lines = []
    for W in (512, 1024):
        tr = make_hip_tracer(scenes.cornell_box(), W, W, time_kernels=1)
        try:
            trace(tr, W, W, 1)
            tr.set_display(1, **display)
            for label, fused in (("bloom off", None), ("bloom on, bloom_fused 0", 0), ("bloom on, bloom_fused 1", 1), ("bloom on, bloom_fused 0 again", 0),
                                 ("bloom on, bloom_fused 1 again", 1)):
                if fused is None:
                    tr.set_bloom(0)
                else:
                    tr.set_bloom(1, **T.BLOOM_DEFAULTS)
                    tr.set_option("bloom_fused", fused)
                for _ in range(3):                                               # warm-up: the pyramid's allocation, first launches
                    sync(tr, W, W, 1)
                for t in TIMERS:
                    tr.kernel_ms(t)                                              # (reading a timer resets it)
                ms = {t: [] for t in TIMERS}
                for _ in range(reps):
                    sync(tr, W, W, 1)
                    for t in TIMERS:
                        ms[t].append(tr.kernel_ms(t)[0])
                m = {t: med(ms[t]) for t in TIMERS}
                lines.append(f"{W}x{W}, {label}: " + ", ".join(f"{t} {m[t] * 1e3:.1f} us" for t in TIMERS if m[t] > 0) +
                             f"; sum {sum(m.values()) * 1e3:.1f} us (medians of {reps} syncs; display is {tr.kernel_symbol('display')})")
                print(lines[-1], flush=True)
        finally:
            tr.Close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bloom_cost.txt"))
    a = ap.parse_args()
    lines = []
    if not a.no_resources:
        lines += resources()
        print("\n".join(lines), flush=True)
    if not a.no_timing:
        lines += timing(a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
