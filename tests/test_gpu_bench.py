"""bench.py end to end on the GPU box: the single-GPU line carries the contract's fields, and the
N>1 flow (row blocks, the primary's peer-read merge through HIP IPC mappings, tonemap) completes under
torch.distributed -- two, three and FOUR processes sharing the one GPU (the box admits six), which exercises
the code path the driver runs on 8 GPUs (the mapping is then a peer mapping over xGMI instead of a second
mapping of local memory); the handle / mapping / merge count of an 8-GPU frame is exercised by one primary
that maps SEVEN peer rings owned by three other processes (test_primary_maps_seven_peer_rings).  The
strip-transfer fallback is covered too (over gloo), for a failed open and a failed export.  Everything
runs as subprocesses under a timeout so a collective mismatch cannot hang the suite."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


SMALL = ["--width", "128", "--height", "97", "--spp", "8", "--steps", "2", "--warmup", "1"]  # 97 rows: uneven blocks [49, 48]


def test_bench_single_gpu_line(built):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", *SMALL], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["config"]["workload"]
    # the line says which physical GPU it was measured on (polaris_hip_device_identity) and what its merges were
    (dev,) = d["config"]["devices"]
    assert d["config"]["distinct_gpus"] == 1 and dev["rank"] == 0 and dev["hip_index"] == 0 and dev["device_chosen_by"] == "LOCAL_RANK"
    assert len(dev["pci_bus_id"]) >= 7 and ":" in dev["pci_bus_id"] and len(dev["uuid"]) == 32 and dev["cus"] > 0 and "gfx950" in dev["gcn_arch"]
    mc = d["config"]["exchange_detail"]["merge_counts"]
    assert mc["local"] > 0 and sum(mc.values()) == mc["local"]      # MergeOutput(self) only
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    # ONE kernel symbol, the one with the largest isolated time; every stream-moving symbol has the same object
    assert r["kernel"].startswith("pol::k_") and r["kernel"] in d["roofline_per_kernel"]
    assert r["ms_per_frame"] == max(e["ms_per_frame"] for e in d["roofline_per_kernel"].values())
    syms = set(d["roofline_per_kernel"])
    assert any(s.startswith("pol::k_shade<") and s.endswith(", true>") for s in syms)          # k_shade<.., FIRST>
    assert "pol::k_generate" in syms and any(s.startswith("pol::k_trace<true") for s in syms)
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["value"] > 0
    # the PMC counters are collected live, by rocprofv3 child runs of the same workload at the end of the run: HBM traffic per launch,
    # live lanes and the issue roofline come from THIS build on THIS machine (the committed profiles are only the fallback)
    assert "THIS run" in r["counters_source"], r["counters_source"]
    assert r["traffic"] > 0 and 0.0 < r["lane_util"] <= 1.0 and 0.0 < d["roofline_issue"]["frac"] < 1.0
    assert all(e["roofline_issue"] and e["traffic"] for e in d["roofline_per_kernel"].values())


def test_bench_plain_line_and_dumped_outputs(built, tmp_path):
    """A plain run (no --full) times exactly --steps frames and measures nothing else; --dump-outputs writes the last timed frame's
    results in float32, and a second run with the same arguments writes the same results bit for bit (exact_accumulate=1); on one GPU
    the frame accumulator holds the last frame's one block: its rows equal the trace accumulator's."""
    import numpy as np

    runs = []
    for i in range(2):
        d_out = tmp_path / f"out{i}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, "--steps", "3", "--opt", "exact_accumulate=1", "--dump-outputs", str(d_out)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        d = json.loads(out.stdout.strip().splitlines()[-1])
        assert d["full"] is False and d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["roofline"] is None and d["cpu_baseline"] is None and "roofline_per_kernel" not in d and "kernels_isolated_ms_per_frame" not in d
        assert d["config"]["rays_per_frame"] > 0
        got = {p.stem: np.load(p) for p in d_out.glob("*.npy")}
        assert sorted(got) == ["frame_accumulator", "framebuffer", "trace_accumulator"]
        assert all(a.dtype == np.float32 and a.shape == (97, 128, 4) for a in got.values())
        runs.append(got)
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    trace, frame = runs[0]["trace_accumulator"], runs[0]["frame_accumulator"]
    assert trace[..., :3].mean() > 0 and runs[0]["framebuffer"][..., :3].max() > 0
    assert np.array_equal(frame[..., :3], trace[..., :3])      # the frame's one block, merged into the frame accumulator


def _two_rank_frame_matches_the_oracle(d, acc_path):
    """rank 0's frame accumulator of the last frame == the oracle run block by block, bit for bit
    (exact_accumulate=1), like test_row_blocks_merge_to_the_full_frame does in-process."""
    import numpy as np

    from oracle import pybind as ob
    from polaris_amd import scenes
    from polaris_amd.distributed import block_of, naive_rows

    W, H, spp, B = 128, 97, 8, 5
    frame = np.load(acc_path)
    assert frame.shape == (H, W, 4)
    sc = scenes.SCENES["cornell"](W / H)
    seeds = scenes.make_seeds(spp, B)
    rows = naive_rows(2, H)
    orc = ob.Oracle("oracle")
    expect = np.zeros((H, W, 3), np.float32)
    rays = 0
    for r in range(2):
        by, bh = block_of(r, rows)
        a, st, _ = orc.trace(sc, ob.make_request(W, H, spp=spp, bounces=B, rr=3, block_y=by, block_h=bh), seeds)
        expect[by:by + bh] = a[by:by + bh, :, :3]
        rays += st.total_rays()
    assert np.array_equal(frame[..., :3].view(np.uint32), expect.view(np.uint32))
    assert d["config"]["rays_per_frame"] == rays


def test_bench_two_ranks_bare_launch_and_frame(built, tmp_path):
    """`python bench.py --gpus 2` with NO launcher: bench.py starts its own ranks (two ranks share the one
    GPU over gloo -- the same frame loop the driver runs over RCCL on 8 GPUs), reports n_gpus == 2, and the
    frame the primary assembled from the gathered strips equals the per-block oracle bit for bit."""
    acc = str(tmp_path / "frame.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", *SMALL, "--same-device", "--no-cpu-baseline",
           "--opt", "exact_accumulate=1", "--save-accumulator", acc]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len(out.stdout.splitlines()) == 1, out.stdout[:600]     # ONE line on stdout, whatever gloo / the runtime print (they go to stderr)
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["config"]["ranks"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    assert d["config"]["exchange"].startswith("hip-ipc"), d["config"]["exchange"]      # the default: peer reads, no fallback
    # ... and the line proves where it ran: two ranks, ONE physical GPU (--same-device), every block read through a mapping of LOCAL memory
    _one_gpu_shared_by(d, 2, "--same-device")
    assert d["config"]["scheduler"] == "naive" and "row blocks [49, 48]" in d["config"]["workload"]   # what `polaris render` passes
    ps = d["config"]["perfect_scheduler"]                                                 # the second timed region of the same run
    assert ps["scheduler"] == "perfect" and ps["value"] > 0 and sum(ps["rows_last_frame"]) == 97
    _two_rank_frame_matches_the_oracle(d, acc)


def _one_gpu_shared_by(d, ranks, chosen_by, branch="ipc-local"):
    """config.devices / distinct_gpus / exchange_detail of a run whose `ranks` ranks all sit on the box's one GPU."""
    cfg = d["config"]
    assert d["n_gpus"] == ranks and cfg["distinct_gpus"] == 1 and len(cfg["devices"]) == ranks
    assert [e["rank"] for e in cfg["devices"]] == list(range(ranks))
    assert len({(e["pci_bus_id"], e["uuid"]) for e in cfg["devices"]}) == 1 and len({e["pid"] for e in cfg["devices"]}) == ranks
    # (under a per-rank mask rank 0's LOCAL_RANK 0 IS the one visible device: it says "LOCAL_RANK", the others say why they took index 0)
    assert all(e["hip_index"] == 0 and (chosen_by in e["device_chosen_by"] or (e["local_rank"] == 0 and e["device_chosen_by"] == "LOCAL_RANK"))
               for e in cfg["devices"]), [(e["local_rank"], e["device_chosen_by"]) for e in cfg["devices"]]
    x = cfg["exchange_detail"]
    # the exchange proves itself: every rank's own rows, gathered over gloo after the timed regions, equal the primary's frame accumulator
    pr = x["proof"]
    assert pr.get("all_equal") is True and pr["blocks_equal"] == [True] * ranks and pr["covered_rows"] == sum(pr["rows"]) == cfg["frame"][1], pr
    if x["mode"] == "hip-ipc":
        assert x["control"] == "shm"     # the ranks of one box: the per-frame message goes through the shared-memory mailbox
        assert [p["rank"] for p in x["peers"]] == list(range(1, ranks))
        assert all(p["branch"] == branch and p["same_device"] == 1 and p["pci_bus_id"] == cfg["devices"][0]["pci_bus_id"] for p in x["peers"]), x["peers"]
        mc = x["merge_counts"]
        assert mc[branch] > 0 and mc["local"] > 0 and sum(mc.values()) == mc[branch] + mc["local"], mc     # every peer block by that branch, its own block by merge_slot
        assert mc[branch] == (ranks - 1) * mc["local"], mc
    else:
        assert x["mode"] == "strips-gloo" and all(p["branch"] == "strips-gloo" for p in x["peers"]) and x["merge_counts"]["device-strip"] > 0, x


def test_bench_two_ranks_strip_fallback(built, tmp_path):
    """`--exchange strips`: the path bench.py falls back to when an IPC mapping cannot be opened -- point-to-point transfers of
    the strips (here over gloo, staged through the host; RCCL needs two GPUs), merged with polaris_hip_merge_device."""
    acc = str(tmp_path / "frame.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", *SMALL, "--exchange", "strips", "--backend", "gloo", "--same-device", "--no-cpu-baseline",
           "--no-second-scheduler", "--opt", "exact_accumulate=1", "--save-accumulator", acc]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["config"]["exchange"].startswith("gloo point-to-point")
    _one_gpu_shared_by(d, 2, "--same-device")
    _two_rank_frame_matches_the_oracle(d, acc)


def test_bench_falls_back_inside_the_same_processes_when_a_mapping_cannot_be_opened(built, tmp_path):
    """The default exchange with rank 0 refusing to map the peers' rings (what a failing hipIpcOpenMemHandle looks like to
    PeerExchange.setup): every rank must switch to the strip transfers without a re-launch -- here over gloo, since RCCL needs two
    GPUs -- say so in config.exchange, and still assemble the right frame."""
    acc = str(tmp_path / "frame.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", *SMALL, "--test-ipc-failure", "--backend", "gloo", "--same-device", "--no-cpu-baseline",
           "--no-second-scheduler", "--opt", "exact_accumulate=1", "--save-accumulator", acc]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "falling back to strip transfers" in out.stderr
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["exchange"].startswith("fallback after a failed IPC mapping") and "gloo point-to-point" in d["config"]["exchange"]
    _one_gpu_shared_by(d, 2, "--same-device")      # the silent-fallback case: exchange_detail.mode names the transport that really ran
    _two_rank_frame_matches_the_oracle(d, acc)


def test_an_ipc_export_that_cannot_be_mapped_is_refused_cleanly(built):
    """polaris_hip_ipc_open on handles the runtime will not open (here: this process's own export with another pid written into
    it -- HIP cannot open its own IPC handle) returns POLARIS_E_UNSUPPORTED with the runtime's message and leaves nothing
    half-mapped: the tracer keeps working, a merge from an own ring slot still adds up."""
    import numpy as np

    from conftest import make_hip_tracer
    from oracle import pybind as ob
    from polaris_amd import ctypes_api as T
    from polaris_amd import scenes
    from polaris_amd.tracer import TracerError

    sc = scenes.SCENES["cubes"]()
    W, H, spp, B = 32, 24, 1, 2
    tr = make_hip_tracer(sc, W, H, exact_accumulate=1)
    try:
        x = T.IpcExport.from_buffer_copy(tr.ipc_export(3))
        x.pid += 1
        with pytest.raises(TracerError) as e:
            tr.ipc_open(bytes(x))
        assert e.value.code == 6 and "hipIpcOpenMemHandle" in str(e.value)      # POLARIS_E_UNSUPPORTED
        x.frame_w += 1
        with pytest.raises(TracerError, match="does not match"):
            tr.ipc_open(bytes(x))
        seeds = scenes.make_seeds(spp, B)
        tr.Trace(ob.make_request(W, H, spp=spp, bounces=B), seeds)
        tr.reset_frame()
        tr.merge_slot(tr, tr.trace_slot(), ob.make_request(W, H, spp=spp, bounces=B))
        tr.SyncFramebuffer(ob.make_request(W, H, spp=spp, bounces=B))
        assert np.array_equal(tr.read_accumulator(1), tr.read_accumulator(0)) and tr.read_accumulator(0)[..., :3].sum() > 0
    finally:
        tr.Close()


def test_bench_two_ranks_perfect_scheduler(built, tmp_path):
    """`--scheduler perfect`: the reference's perfect scheduler (tracer/scheduler.go:50-80) fed by all-gathered (rows, time)
    pairs -- every rank must arrive at the same rows every frame, or the blocks would not fit together.  The last frame, with
    whatever rows the scheduler had settled on, must be the per-block oracle result bit for bit."""
    import numpy as np

    from oracle import pybind as ob
    from polaris_amd import scenes

    acc = str(tmp_path / "frame.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    small = ["--width", "128", "--height", "97", "--spp", "8", "--steps", "4", "--warmup", "3"]
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", *small, "--same-device", "--no-cpu-baseline", "--no-kernel-timers",
           "--scheduler", "perfect", "--no-second-scheduler", "--opt", "exact_accumulate=1", "--save-accumulator", acc,
           "--control", "gloo"]    # (the per-frame message as a gloo all_gather: what ranks that cannot map a common /dev/shm file fall back to)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.splitlines()[-1])["config"]["exchange_detail"]["control"] == "gloo"
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    rows = d["config"]["rows_last_frame"]
    assert d["config"]["scheduler"] == "perfect" and "perfect scheduler" in d["config"]["workload"] and sum(rows) == 97 and min(rows) >= 1
    assert d["config"]["exchange"].startswith("hip-ipc"), d["config"]["exchange"]
    W, H, spp, B = 128, 97, 8, 5
    sc = scenes.SCENES["cornell"](W / H)
    seeds = scenes.make_seeds(spp, B)
    orc = ob.Oracle("oracle")
    expect = np.zeros((H, W, 3), np.float32)
    y = 0
    for r in range(2):
        a, _, _ = orc.trace(sc, ob.make_request(W, H, spp=spp, bounces=B, rr=3, block_y=y, block_h=rows[r]), seeds)
        expect[y:y + rows[r]] = a[y:y + rows[r], :, :3]
        y += rows[r]
    assert np.array_equal(np.load(acc)[..., :3].view(np.uint32), expect.view(np.uint32))


def test_bench_two_ranks_with_a_different_frame_every_step(built, tmp_path):
    """The exchange runs one frame behind the tracing (polaris_amd/distributed.py) and every rank's trace accumulator is a ring
    of three: with the same seeds every frame a block read from the wrong ring slot, or merged into the wrong frame, would go
    unnoticed.  --test-seeds gives every frame its own seed list; the frame rank 0 assembled LAST (through the IPC mappings)
    must be the per-block oracle result of the last frame's seeds."""
    import numpy as np

    from oracle import pybind as ob
    from polaris_amd import scenes
    from polaris_amd.distributed import block_of, naive_rows

    acc = str(tmp_path / "frame.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    steps, warmup = 5, 2
    small = ["--width", "128", "--height", "97", "--spp", "8", "--steps", str(steps), "--warmup", str(warmup)]
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", *small, "--same-device", "--no-cpu-baseline",
           "--no-kernel-timers", "--no-second-scheduler", "--opt", "exact_accumulate=1", "--save-accumulator", acc, "--test-seeds"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["exchange"].startswith("hip-ipc"), d["config"]["exchange"]
    W, H, spp, B = 128, 97, 8, 5
    frame = np.load(acc)
    sc = scenes.SCENES["cornell"](W / H)
    seeds = scenes.make_seeds(spp, B, base=0xC0FFEE + steps + warmup - 1)   # the last frame's list
    rows = naive_rows(2, H)
    orc = ob.Oracle("oracle")
    expect = np.zeros((H, W, 3), np.float32)
    for r in range(2):
        by, bh = block_of(r, rows)
        a, _, _ = orc.trace(sc, ob.make_request(W, H, spp=spp, bounces=B, rr=3, block_y=by, block_h=bh), seeds)
        expect[by:by + bh] = a[by:by + bh, :, :3]
    assert np.array_equal(frame[..., :3].view(np.uint32), expect.view(np.uint32))


def _frame_matches_the_oracle_block_by_block(acc_path, W, H, spp, B, rows, seeds):
    import numpy as np

    from oracle import pybind as ob
    from polaris_amd import scenes

    frame = np.load(acc_path)
    assert frame.shape == (H, W, 4) and sum(rows) == H and min(rows) >= 1
    sc = scenes.SCENES["cornell"](W / H)
    orc = ob.Oracle("oracle")
    expect = np.zeros((H, W, 3), np.float32)
    y = rays = 0
    for bh in rows:
        a, st, _ = orc.trace(sc, ob.make_request(W, H, spp=spp, bounces=B, rr=3, block_y=y, block_h=bh), seeds)
        expect[y:y + bh] = a[y:y + bh, :, :3]
        y += bh
        rays += st.total_rays()
    assert np.array_equal(frame[..., :3].view(np.uint32), expect.view(np.uint32))
    return rays


def test_bench_four_ranks_bare_launch_headline_blocks_one_rank_held_back(built, tmp_path):
    """`python bench.py --gpus 4`, the first command a multi-GPU node runs (here: four PROCESSES sharing the one GPU -- the box
    admits six -- through the real HIP-IPC path: three peer rings mapped by rank 0, twelve memory and twelve event handles, four
    merges per frame).  64 rows per rank, the block an 8-GPU headline frame gives a rank; a different seed list every frame;
    rank 3 sleeps 60 ms after every Trace so that the three others run as far ahead of it as the ring's depth-3 argument lets
    them (renderer/default.go:127-136,188-191).  The frame rank 0 assembled last == the per-block oracle of the last frame's
    seeds, bit for bit; the same run then times the perfect scheduler (tracer/scheduler.go:50-80) over four (rows, ns) pairs."""
    from polaris_amd import scenes

    acc = str(tmp_path / "frame.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    W, H, spp, B, steps, warmup = 128, 256, 4, 5, 4, 1
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "4", "--width", str(W), "--height", str(H), "--spp", str(spp), "--steps", str(steps),
           "--warmup", str(warmup), "--same-device", "--no-cpu-baseline", "--no-kernel-timers", "--opt", "exact_accumulate=1", "--save-accumulator", acc,
           "--test-seeds", "--test-delay-rank", "3:60"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 4 and d["config"]["ranks"] == 4 and d["config"]["exchange"].startswith("hip-ipc"), d["config"]["exchange"]
    _one_gpu_shared_by(d, 4, "--same-device")
    assert d["config"]["rows_last_frame"] == [64, 64, 64, 64] and d["config"]["scheduler"] == "naive"
    ps = d["config"]["perfect_scheduler"]
    assert ps["scheduler"] == "perfect" and ps["value"] > 0 and sum(ps["rows_last_frame"]) == H and min(ps["rows_last_frame"]) >= 1
    # the rank that is held back reports the longest frames: the perfect scheduler must have taken rows AWAY from it, and rank 0's
    # block must not have withered (round 4 billed the primary the wait for the slowest rank: ADVICE r4)
    assert ps["rows_last_frame"][3] < 64 and ps["rows_last_frame"][0] >= 16, ps
    _frame_matches_the_oracle_block_by_block(acc, W, H, spp, B, [64] * 4, scenes.make_seeds(spp, B, base=0xC0FFEE + steps + warmup - 1))


def test_bench_four_ranks_under_the_drivers_launcher_c4_blocks_perfect_scheduler(built, tmp_path):
    """The driver's launch line (`python -m torch.distributed.run --nproc-per-node 4 ... bench.py --gpus 4`) on a C4-shaped
    frame: 541 rows -> [136, 135, 135, 135] (135 rows = a rank's block of the 1080-row frame on 8 GPUs; the odd row goes to
    tracer 0, scheduler.go:98-104), `--scheduler perfect`: the rows change from frame to frame with the ranks' measured times
    and every rank must arrive at the same ones.  Last frame == per-block oracle for whatever rows it ended on."""
    from polaris_amd import scenes

    acc = str(tmp_path / "frame.npy")
    W, H, spp, B, steps, warmup = 96, 541, 2, 5, 4, 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "4", "--width", str(W), "--height", str(H), "--spp", str(spp),
           "--steps", str(steps), "--warmup", str(warmup), "--same-device", "--no-cpu-baseline", "--no-kernel-timers", "--no-second-scheduler",
           "--scheduler", "perfect", "--opt", "exact_accumulate=1", "--save-accumulator", acc, "--test-seeds"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 4 and d["config"]["exchange"].startswith("hip-ipc"), d["config"]["exchange"]
    assert d["config"]["rows_first_timed_frame"] is not None and d["config"]["scheduler"] == "perfect"
    rows = d["config"]["rows_last_frame"]
    rays = _frame_matches_the_oracle_block_by_block(acc, W, H, spp, B, rows, scenes.make_seeds(spp, B, base=0xC0FFEE + steps + warmup - 1))
    assert rays > 0


def test_bench_three_ranks_fall_back_together_when_an_export_fails(built, tmp_path):
    """`--test-ipc-failure export`: the LAST rank's polaris_hip_ipc_export raises.  PeerExchange.setup() must not leave the
    others hanging in its collective: every rank learns of it and all switch to the strip transfers together (here over gloo)."""
    from polaris_amd import scenes

    acc = str(tmp_path / "frame.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    W, H, spp, B = 128, 97, 8, 5
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "3", *SMALL, "--test-ipc-failure", "export", "--backend", "gloo", "--same-device",
           "--no-cpu-baseline", "--no-kernel-timers", "--no-second-scheduler", "--opt", "exact_accumulate=1", "--save-accumulator", acc]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "falling back to strip transfers" in out.stderr and "rank 2: export failed" in out.stderr
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 3 and d["config"]["exchange"].startswith("fallback after a failed IPC mapping") and "gloo point-to-point" in d["config"]["exchange"]
    _frame_matches_the_oracle_block_by_block(acc, W, H, spp, B, [33, 32, 32], scenes.make_seeds(spp, B))


def _ring_owner(conn, ranks, W, H, spp, B, frames, rows):
    """Child process of test_primary_maps_seven_peer_rings: owns the tracers of `ranks`, exports their rings, traces every
    frame's blocks and names the slots.  Before Trace f it waits for the primary's "merged f - 3" (the frame that lived in the
    slot Trace f overwrites) -- the rule PeerExchange's depth-3 argument guarantees."""
    sys.path.insert(0, ROOT)
    from conftest import make_hip_tracer
    from oracle import pybind as ob
    from polaris_amd import scenes
    from polaris_amd.distributed import block_of

    try:
        sc = scenes.SCENES["cornell"](W / H)
        trs = {r: make_hip_tracer(sc, W, H, exact_accumulate=1) for r in ranks}
        conn.send({r: trs[r].ipc_export(3) for r in ranks})
        merged = -1
        for f in range(frames):
            while merged < f - 3:
                merged = conn.recv()
            slots = {}
            for r in ranks:
                by, bh = block_of(r, rows)
                trs[r].Trace(ob.make_request(W, H, spp=spp, bounces=B, block_y=by, block_h=bh), scenes.make_seeds(spp, B, base=500 + f))
                slots[r] = trs[r].trace_slot()
            conn.send((f, slots))
        while merged < frames - 1:      # the rings stay mapped until the primary has read the last frame and closed its mappings
            merged = conn.recv()
        assert conn.recv() == "closed"
        for t in trs.values():
            t.Close()
        conn.send("bye")
    except Exception as e:  # noqa: BLE001 -- report instead of leaving the parent in recv()
        conn.send(("error", repr(e)))


def test_primary_maps_seven_peer_rings(built, oracle):
    """An 8-rank frame's worth of IPC on the one GPU of the box, which admits six processes: the primary (this process) maps the
    rings of SEVEN tracers living in three other processes (3 + 2 + 2) -- 21 hipIpcOpenMemHandle mappings and 21 inter-process
    events, one per ring slot -- and assembles every frame from eight blocks (61 rows -> [12, 7, 7, 7, 7, 7, 7, 7]), one frame
    behind the tracing, a different seed list every frame, the owners running ahead as far as the ring allows.  Every frame ==
    the per-block oracle bit for bit.  (renderer/default.go:127-136,188-191; what bench.py --gpus 8 does with one tracer per
    process.)"""
    import multiprocessing as mp

    import numpy as np

    from conftest import bits, make_hip_tracer
    from oracle import pybind as ob
    from polaris_amd import scenes
    from polaris_amd.distributed import block_of, naive_rows

    W, H, spp, B, frames = 64, 61, 2, 4, 6
    rows = naive_rows(8, H)
    assert rows == [12, 7, 7, 7, 7, 7, 7, 7]
    ctx = mp.get_context("spawn")
    groups = [(1, 2, 3), (4, 5), (6, 7)]
    conns, procs = [], []
    for g in groups:
        a, b = ctx.Pipe()
        p = ctx.Process(target=_ring_owner, args=(b, g, W, H, spp, B, frames, rows), daemon=True)
        p.start()
        conns.append(a)
        procs.append(p)

    def recv(c):
        assert c.poll(300), "a ring owner went silent"
        m = c.recv()
        assert not (isinstance(m, tuple) and m[0] == "error"), m
        return m

    sc = scenes.SCENES["cornell"](W / H)
    prim = make_hip_tracer(sc, W, H, exact_accumulate=1)
    peers = {}
    try:
        prim.ipc_export(3)
        for c in conns:
            for r, blob in recv(c).items():
                peers[r] = prim.ipc_open(blob)
        assert sorted(peers) == [1, 2, 3, 4, 5, 6, 7]
        full = ob.make_request(W, H, spp=spp, bounces=B)
        own_slots = {}

        def merge(f):
            slots = {0: own_slots[f]}
            for c in conns:
                ff, s = recv(c)
                assert ff == f
                slots.update(s)
            prim.reset_frame()
            for r in range(8):
                by, bh = block_of(r, rows)
                req = ob.make_request(W, H, spp=spp, bounces=B, block_y=by, block_h=bh)
                if r == 0:
                    prim.merge_slot(prim, slots[0], req)
                else:
                    prim.merge_ipc(peers[r], slots[r], req)
            prim.SyncFramebuffer(full)
            got = prim.read_accumulator(1)[..., :3]
            seeds = scenes.make_seeds(spp, B, base=500 + f)
            expect = np.zeros((H, W, 3), np.float32)
            for r in range(8):
                by, bh = block_of(r, rows)
                a = oracle.trace(sc, ob.make_request(W, H, spp=spp, bounces=B, block_y=by, block_h=bh), seeds)[0]
                expect[by:by + bh] = a[by:by + bh, :, :3]
            assert np.array_equal(bits(got), bits(expect)), f
            for c in conns:
                c.send(f)

        for f in range(frames):
            by, bh = block_of(0, rows)
            prim.Trace(ob.make_request(W, H, spp=spp, bounces=B, block_y=by, block_h=bh), scenes.make_seeds(spp, B, base=500 + f))
            own_slots[f] = prim.trace_slot()
            if f >= 1:
                merge(f - 1)          # one frame behind the tracing, like PeerExchange
        merge(frames - 1)
        for r in list(peers):
            prim.ipc_close(peers.pop(r))
        for c in conns:
            c.send("closed")
        for c in conns:
            assert recv(c) == "bye"
    finally:
        for r in list(peers):
            prim.ipc_close(peers.pop(r))
        prim.Close()
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()


@pytest.mark.parametrize("scheduler", ["naive", "perfect"])
def test_bench_inproc_three_tracers_on_one_gpu(built, tmp_path, scheduler):
    """`bench.py --gpus 3 --inproc --devices 0,0,0`: ONE process, the C++ frame loop (worker thread per tracer), the blocks
    merged into the primary through polaris_hip_merge on its merge stream -- the reference renderer's own model
    (renderer/default.go:106-196), no torch.distributed.  The last frame must be the per-block oracle result for the rows the
    scheduler handed out, bit for bit."""
    import numpy as np

    from oracle import pybind as ob
    from polaris_amd import scenes

    acc = str(tmp_path / "frame.npy")
    W, H, spp, B, steps = 96, 90, 4, 5, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--inproc", "--devices", "0,0,0", "--scheduler", scheduler, "--width", str(W),
           "--height", str(H), "--spp", str(spp), "--steps", str(steps), "--warmup", "0", "--opt", "exact_accumulate=1", "--test-seeds",
           "--save-accumulator", acc]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    rows = d["config"]["rows_last_frame"]
    assert d["config"]["tracers"] == 3 and sum(rows) == H and min(rows) >= 1 and d["value"] > 0
    assert d["config"]["rows_first_timed_frame"] == [30, 30, 30]      # both schedulers start from the naive split (scheduler.go:52-56)
    assert scheduler in d["config"]["workload"] and str(rows) in d["config"]["workload"]
    sc = scenes.SCENES["cornell"](W / H)
    orc = ob.Oracle("oracle")
    expect = np.zeros((H, W, 3), np.float32)
    y, rays = 0, 0
    for t in range(3):
        a, st, _ = orc.trace(sc, ob.make_request(W, H, spp=spp, bounces=B, rr=3, block_y=y, block_h=rows[t]), scenes.make_seeds(spp, B, base=1000 * (steps - 1) + 17 * t))
        expect[y:y + rows[t]] = a[y:y + rows[t], :, :3]
        y += rows[t]
    frame = np.load(acc)
    assert np.array_equal(frame[..., :3].view(np.uint32), expect.view(np.uint32))


def test_bench_inproc_refuses_more_gpus_than_visible(built):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--inproc", *SMALL], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode != 0 and "only" in (out.stderr + out.stdout) and "{" not in out.stdout


def test_bench_refuses_more_gpus_than_visible(built):
    """--gpus 64 on this box must fail loudly, never print a 1-GPU line."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", *SMALL], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode != 0 and "only" in (out.stderr + out.stdout) and "{" not in out.stdout


def test_bench_two_ranks_under_the_drivers_launcher(built):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", *SMALL, "--same-device",
           "--no-cpu-baseline"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    assert "row blocks [49, 48]" in d["config"]["workload"] and d["config"]["exchange"].startswith("hip-ipc")


def test_bench_four_ranks_masked_to_one_visible_device_each(built, tmp_path):
    """The launch shape VERDICT round 5 found untested: a launcher that MASKS every rank to one visible device
    (HIP_VISIBLE_DEVICES per rank) -- here all four to GPU 0, the only one of the box -- and hands out LOCAL_RANK 0..3.  Round 5
    indexed the device by LOCAL_RANK and would have failed on every rank but 0; now a rank whose LOCAL_RANK is beyond the visible
    devices takes the one it sees (polaris_amd.distributed.device_for_rank), and the line says what happened: four ranks, one
    distinct GPU, every mapping a local one.  No --same-device: this is the product's own device choice
    (renderer/default.go:204-256, tracer/opencl/tracer.go:279-286)."""
    from polaris_amd import scenes

    acc = str(tmp_path / "frame.npy")
    W, H, spp, B, steps, warmup = 96, 128, 2, 5, 3, 1
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "4", "--width", str(W), "--height", str(H), "--spp", str(spp),
           "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-kernel-timers", "--no-second-scheduler",
           "--opt", "exact_accumulate=1", "--save-accumulator", acc, "--test-seeds"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["exchange"].startswith("hip-ipc"), d["config"]["exchange"]
    _one_gpu_shared_by(d, 4, "one visible device")
    assert d["config"]["devices"][0]["device_chosen_by"] == "LOCAL_RANK" and d["config"]["devices"][3]["local_rank"] == 3
    assert all(e["visible_devices"] == 1 and e["HIP_VISIBLE_DEVICES"] == "0" for e in d["config"]["devices"])
    assert d["config"]["exchange_detail"]["can_access_peer_from_primary"] == {"0": None}     # rank 0 sees its own device only
    _frame_matches_the_oracle_block_by_block(acc, W, H, spp, B, [32] * 4, scenes.make_seeds(spp, B, base=0xC0FFEE + steps + warmup - 1))


def test_bench_four_ranks_sixty_frames_under_random_delays(built, tmp_path):
    """The randomised schedule of the CPU protocol test, through the REAL exchange: four processes, HIP-IPC mappings of three rings of
    depth 3, per-slot inter-process events, 60 frames with a different seed list each, every rank sleeping a seeded random time after
    every Trace -- who runs ahead and who lags changes from frame to frame -- under the perfect scheduler, whose rows follow the
    measured times.  The frame rank 0 assembled LAST must be the per-block oracle of the last frame's seeds for the rows it ended on
    (a slot reused too early, a merge from the wrong slot or ranks disagreeing about rows would break it)."""
    from polaris_amd import scenes

    acc = str(tmp_path / "frame.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    W, H, spp, B, steps, warmup = 96, 122, 2, 4, 60, 2
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "4", "--width", str(W), "--height", str(H), "--spp", str(spp), "--bounces", str(B),
           "--steps", str(steps), "--warmup", str(warmup), "--same-device", "--no-cpu-baseline", "--no-kernel-timers", "--no-second-scheduler",
           "--scheduler", "perfect", "--opt", "exact_accumulate=1", "--save-accumulator", acc, "--test-seeds", "--test-random-delays", "11"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["exchange"].startswith("hip-ipc") and d["config"]["exchange_detail"]["mode"] == "hip-ipc"
    mc = d["config"]["exchange_detail"]["merge_counts"]
    assert mc["ipc-local"] == 3 * (steps + warmup) and mc["local"] == steps + warmup, mc        # every frame: three peer blocks + its own, nothing else
    rows = d["config"]["rows_last_frame"]
    assert sum(rows) == H and min(rows) >= 1
    _frame_matches_the_oracle_block_by_block(acc, W, H, spp, B, rows, scenes.make_seeds(spp, B, base=0xC0FFEE + steps + warmup - 1))


def test_merge_ipc_through_the_staging_strip(built, tmp_path):
    """A ring on a GPU the primary has no peer access to must never be read by a kernel (a fault there can take a node down): the
    runtime copies the rows into a staging strip (hipMemcpyAsync) and k_aggregate adds from there.  Every pair of GPUs of an MI355X
    node has peer access, so the path is exercised by forcing it (option ipc_staged = 1) on the one GPU: the line says `ipc-staged`
    for every peer, the library counted every peer merge under that branch, and the frame is the per-block oracle's, bit for bit."""
    acc = str(tmp_path / "frame.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "3", *SMALL, "--same-device", "--no-cpu-baseline", "--no-kernel-timers", "--no-second-scheduler",
           "--opt", "exact_accumulate=1", "--opt", "ipc_staged=1", "--save-accumulator", acc]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["exchange"].startswith("hip-ipc"), d["config"]["exchange"]
    _one_gpu_shared_by(d, 3, "--same-device", branch="ipc-staged")
    from polaris_amd import scenes

    _frame_matches_the_oracle_block_by_block(acc, 128, 97, 8, 5, [33, 32, 32], scenes.make_seeds(8, 5))


def test_a_rank_that_fails_during_setup_reaches_every_rank(built):
    """--test-setup-failure 2: rank 2 of 3 cannot bring its tracer up.  Before round 6 the others would have sat in the first
    collective until its timeout; now every rank's set-up verdict is gathered over the (120 s-bounded) gloo group before any
    other collective, rank 0 names the failed rank, every rank exits non-zero, and no bench line is printed."""
    import time

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    t = time.time()
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", *SMALL, "--same-device", "--no-cpu-baseline", "--test-setup-failure", "2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode != 0 and "{" not in out.stdout
    assert "set-up failed" in out.stderr and "rank 2: RuntimeError: injected set-up failure" in out.stderr, out.stderr[-1500:]
    assert time.time() - t < 120
