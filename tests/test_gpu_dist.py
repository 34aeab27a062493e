"""The multi-process sharded paths on the MI355X at world = 1: RCCL process
group + IPC peer buffers + cfmm_set_peers, launched exactly as the driver
launches bench.py (torch.distributed.run, 127.0.0.1 rendezvous).  The log is kept under
gpurun_out/ and copied to profiles/ (r02_dist_world1.json)."""
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _torchrun(args, timeout=600):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port())] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT)


def test_sharded_paths_world1_rccl_and_peer():
    r = _torchrun([os.path.join(ROOT, "tests", "dist_world1_worker.py")])
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    line = [l for l in r.stdout.splitlines() if l.startswith("DIST_WORLD1 ")][-1]
    out = json.loads(line[len("DIST_WORLD1 "):])
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "gpurun_out", "dist_world1.json"), "w"), indent=1)
    assert out["backend"] == "nccl" and out["world"] == 1
    assert out["peer"]["in_library_collective"] and not out["rccl"]["in_library_collective"]
    assert out["lib_rccl"]["in_library_collective"] and "cfmm_rccl_init_rank" in out["lib_rccl"]["collective"]
    for path in ("peer", "lib_rccl", "rccl"):
        rec = out[path]
        assert rec["fixed_v_netflow_equal"] and rec["trades_equal"]   # world 1: the all-reduce is the identity
        assert rec["route_native_netflow_rel_diff"] <= 1e-9 and rec["route_scipy_netflow_rel_diff"] <= 1e-9
        assert rec["route_native_evaluations"] >= 5


@pytest.mark.parametrize("extra", [[], ["--rccl"]])
def test_bench_under_torchrun_world1(extra):
    """bench.py exactly as the driver launches it for N > 1, at N = 1: RCCL init, the collective in the
    timed step, the self-check against a plain all-reduce, the sharded route! leg."""
    r = _torchrun([os.path.join(ROOT, "bench.py"), "--full", "--gpus", "1", "--steps", "20", "--warmup", "3",
                   "--workload", "config4shard"] + extra)
    print(r.stdout[-2000:], r.stderr[-3000:])
    assert r.returncode == 0
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["collective_check_rel_err"] <= 1e-12
    assert ("RCCL" in line["config"]["sharding"]) == bool(extra)
    rs = line["route_sharded"]
    assert "error" not in rs and rs["ranks_agree_on_v"] and rs["evaluations"] >= 5
    # one line carries the step under ALL three all-reduces, whichever is the headline
    assert line["collective"]["headline"] == ("rccl_library" if extra else "peer")
    col = line["collectives"]
    for mode in ("peer", "rccl_library", "rccl_torch"):
        assert col[mode]["ok"], (mode, col[mode])
        assert col[mode]["ms_per_step"] > 0 and col[mode]["check_rel_err"] <= 1e-12
        assert 0 < col[mode]["kernel_ms_min"] <= col[mode]["kernel_ms_max"]
    assert col["rccl_library"]["rccl_ranks"] == 1 and "cfmm_rccl_init_rank" in col["rccl_library"]["sharding"]
    # N = 1 under torchrun costs what the plain N = 1 step costs (same process, same clocks)
    assert line["plain_n1"]["ratio_torchrun_over_plain"] <= (1.10 if extra else 1.05), line["plain_n1"]
    tag = "rccl" if extra else "peer"
    json.dump(line, open(os.path.join(ROOT, "gpurun_out", f"bench_torchrun_world1_{tag}.json"), "w"), indent=1)


def test_bench_single_process_multi_device_and_cold_only():
    """bench.py --full --single-process (cfmm_ctx_create_multi, here 3 shards on the one GPU) and --cold-only."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "3", "--single-process",
                        "--devices", "0,0,0", "--steps", "10", "--warmup", "2", "--workload", "config4shard"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout[-1500:], r.stderr[-2000:])
    assert r.returncode == 0
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 3 and line["config"]["pools_total"] == 1_500_000
    assert "cfmm_ctx_create_multi" in line["config"]["sharding"] and line["route"]["evaluations"] >= 5
    json.dump(line, open(os.path.join(ROOT, "gpurun_out", "bench_single_process_3shards.json"), "w"), indent=1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "12", "--warmup", "6",
                        "--cold-only", "--no-cpu", "--workload", "product1m"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout[-1500:], r.stderr[-2000:])
    assert r.returncode == 0
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["roofline"]["residency"].startswith("hbm-resident") and line["roofline"]["warm"] is None
    assert 0.2 < line["roofline"]["frac"] < 1.0


def test_bench_plain_run_is_the_headline_only(tmp_path):
    """The driver's command without --full: set-up, warm-up, the timed steps, --dump-outputs and the headline line -- none of
    the legs --full adds, and at most 30 s of the run's wall-clock outside its warm-up and timed steps."""
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    wall = time.perf_counter() - t0
    print(r.stdout[-1500:], r.stderr[-2000:])
    assert r.returncode == 0
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["metric"].startswith("find_arb! pools/sec") and line["unit"] == "pools/s" and line["higher_is_better"]
    assert line["dtype"] == "f64" and (line["steps"], line["warmup"], line["n_gpus"]) == (20, 5, 1)
    assert line["config"]["workload"].startswith("config3") and not line["config"]["full"]
    m = line["config"]["pools_total"]
    assert m == 1_000_000 and line["value"] == pytest.approx(m / (line["ms_per_step"] * 1e-3), rel=1e-9)
    moved = {"roofline", "route", "cpu_baseline", "parity", "host_boundary", "configs", "value_hbm_resident",
             "collective_check_rel_err", "collectives", "strong_scaling", "route_sharded", "plain_n1"}
    assert not moved & set(line), moved & set(line)
    psi, acc = np.load(tmp_path / "netflows.npy"), np.load(tmp_path / "dual_value.npy")
    D, L = np.load(tmp_path / "trades_delta.npy"), np.load(tmp_path / "trades_lambda.npy")
    assert psi.shape == (256,) and acc.shape == (1,) and D.shape == L.shape == (m, 2)
    assert np.isfinite(psi).all() and np.isfinite(acc).all() and np.abs(psi).max() > 0
    outside = wall - (line["steps"] + line["warmup"]) * line["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.1f} s wall, {outside:.1f} s outside the steps")
    assert outside <= 30.0


def test_bench_default_line_and_reference_grid():
    """The driver's command with --full (N = 1, config3) carries the round-4 fields -- parity by convergence, the fraction of
    the bus from live PMC bytes (or the committed fall-back), an HBM-resident step without kernel events -- and
    `--workload scaling --full` reproduces the reference's own benchmark grid (benchmark/scaling.jl:8-38): 30 points."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "20", "--warmup", "5"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    print(r.stdout[-1500:], r.stderr[-2000:])
    assert r.returncode == 0
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    roof, par = line["roofline"], line["parity"]
    assert line["n_gpus"] == 1 and line["config"]["workload"].startswith("config3")
    assert roof["bound"] == "hbm" and 0.2 < roof["frac"] < 1.0 and roof["cold"]["ms_per_step"] > 0
    assert roof["cold"]["ms_per_step"] <= roof["cold"]["ms_per_step_with_kernel_events"]
    if roof["traffic"]:
        assert 0.1 < roof["bus_frac"] < 1.0 and roof["frac_bus"] == roof["bus_frac"]
    # round 6: the kernel span on rocprofv3's clock (what profiles/ holds) with the hipEvent figure beside it (within 10 %),
    # and what producing the reference's 32-byte rows costs (expand kernel / plain-rows sweep)
    assert "kernel_ms_source" in roof and abs(roof["kernel_ms"] - roof["kernel_ms_hip_events"]) <= 0.1 * roof["kernel_ms"]
    ex = roof["expanded"]
    assert ex["expanded"]["ms_per_step"] >= ex["expanded"]["ms_per_step_compact_only"] and 0 < ex["plain_rows"]["frac"] < 1.0
    c4 = line["configs"]["config4_full"]
    assert c4["pools"] == 4_000_000 and c4["shards"] == 8 and c4["parity"]["all_trade_rows_bit_equal"]
    assert c4["parity"]["netflow_rel_err_at_fixed_v"] <= 1e-12 and c4["parity"]["route_native_vs_fortran_netflow_rel_err"] <= 1e-6
    assert par["netflow_rel_err_at_fixed_v"] <= 1e-12 and par["route_native_netflow_rel_err"] <= 1e-6
    assert par["route_converged_netflow_rel_err"] <= 1e-8
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["value"] > 0
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--workload", "scaling"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    print(r.stdout[-800:], r.stderr[-2000:])
    assert r.returncode == 0
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    grid = line["grid"]
    assert len(grid) == 30 and [g["m"] for g in grid[::3]] == [100, 167, 278, 464, 774, 1292, 2154, 3594, 5995, 10000]
    assert (grid[0]["n_tokens"], grid[1]["n_tokens"], grid[2]["n_tokens"]) == (10, 20, 40)
    for g in grid:
        assert g["netflow_rel_err"] <= 1e-6 and g["native_evaluations"] >= 2 and 0 < g["native_ms"] < 50
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    json.dump(line, open(os.path.join(ROOT, "gpurun_out", "bench_scaling_grid.json"), "w"), indent=1)


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_route_across_processes_sharing_one_gpu(world):
    """A real multi-process run of the N > 1 path on the 1-GPU box: `world` processes (gloo rendezvous; RCCL
    does not allow two ranks on one device) each own a shard, exchange the library's IPC buffer handles,
    and every sweep's fold launch gathers the other processes' {Ψ, acc} from their mapped buffers."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "ipc_ranks_worker.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", CFMM_AMD_PEER_TIMEOUT_S="20")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("IPC_RANKS ")][-1][len("IPC_RANKS "):])
    json.dump(out, open(os.path.join(ROOT, "gpurun_out", f"ipc_ranks_world{world}.json"), "w"), indent=1)
    assert out["world"] == world and out["in_library_collective"] and out["buffers"] == "IpcPeers"
    assert out["guard"] and "checked against torch.distributed" in out["collective"] and out["collective_retries"] == 0
    assert out["ranks_bit_identical"] and out["pools_total"] == 460_000
    assert out["fixed_v_rel_diff"] <= 1e-13
    assert out["route_native_rel_diff"] <= 1e-6 and out["route_scipy_rel_diff"] <= 1e-6 and out["evaluations"] >= 5


def test_config4_at_full_size_across_four_processes_sharing_one_gpu():
    """VERDICT r5 item 2 / BASELINE config 4 AT ITS STATED SIZE: 4M ProductTwoCoin pools, 512 tokens -- here 4 PROCESSES of
    1M pools each on the one GPU (gloo rendezvous, the library's IPC peer buffers, fold + gather in one launch: the N > 1
    path minus the xGMI links).  Four, not eight: the ranks and this process all hold the GPU, and a shared GPU takes at
    most six such processes at once (the 8-shard split of the same market runs in one process in
    test_gpu_multi.py::test_config4_at_full_size_eight_shards).  Every rank: all 1M trade rows of its shard bit-equal to the
    CPU restatement at fixed prices; rank 0: the global Ψ <= 1e-12 of the serial pool-order sum, ranks bit-identical, and
    route! within north_star's 1e-6 of the Fortran L-BFGS-B 3.0 run on the restatement of the SAME 4M-pool market
    (tests/golden/route_fortran.npz: full_config4; that run's own pool-order slack is 8e-7)."""
    world = 4
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "ipc_ranks_worker.py"), "--config4"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", CFMM_AMD_PEER_TIMEOUT_S="30")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, cwd=ROOT, env=env)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("IPC_RANKS ")][-1][len("IPC_RANKS "):])
    assert out["world"] == world and out["pools_total"] == 4_000_000 and out["in_library_collective"]
    assert out["all_trade_rows_bit_equal"] and out["ranks_bit_identical"]
    assert out["fixed_v_rel_err_vs_oracle"] <= 1e-12
    assert out["route_native_vs_fortran"] <= 1e-6 and out["route_scipy_vs_fortran"] <= 1e-6 and out["evaluations"] >= 5


@pytest.mark.parametrize("mode", ["selftest-fail", "fail-route-once"])
def test_sharded_router_guard_across_processes(mode):
    """VERDICT r3 item 3, in the LIBRARY path (dist.py::ShardedRouter), two processes on the one GPU:
    selftest-fail   -- the start-up check of the in-library exchange against torch.distributed is made to disagree on ONE
                       rank: the vote is collective, so BOTH ranks drop the exchange and route through the
                       torch.distributed all-reduce -- same results;
    fail-route-once -- one rank's native route! fails before it publishes: the other rank runs into the peer time-out, both
                       vote, re-align the exchange, switch pre-arming off and repeat the route -- same results."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "ipc_ranks_worker.py"), "--" + mode]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", CFMM_AMD_PEER_TIMEOUT_S="3")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("IPC_RANKS ")][-1][len("IPC_RANKS "):])
    if mode == "selftest-fail":
        assert not out["in_library_collective"] and "torch.distributed" in out["collective"] and not out["guard"]
    else:
        assert out["in_library_collective"] and out["guard"] and out["collective_retries"] == 1
    assert out["ranks_bit_identical"] and out["pools_total"] == 460_000
    assert out["fixed_v_rel_diff"] <= 1e-13
    assert out["route_native_rel_diff"] <= 1e-6 and out["route_scipy_rel_diff"] <= 1e-6 and out["evaluations"] >= 5


def test_bench_rehearsal_world2_on_one_gpu():
    """The N > 1 orchestration of bench.py at world = 2 on the ONE GPU of this box (CFMM_BENCH_SHARE_GPU=1: both ranks on
    device 0, rendezvous over gloo because RCCL does not share a device): shard indexing, the in-library peer exchange
    between two PROCESSES, the start-up collective check, global-market oracle parity on rank 0, the sharded route! and
    the strong-scaling leg (config 4 divided among the ranks).  Timings of such a run mean nothing (`config.rehearsal`);
    what is asserted is that the line exists and that its parity figures are those of an N = 1 run."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "10",
           "--warmup", "2", "--opt", "armed=0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT,
                       env=dict(os.environ, CFMM_BENCH_SHARE_GPU="1"))
    print(r.stdout[-2000:], r.stderr[-3000:])
    assert r.returncode == 0
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and "rehearsal" in line["config"]
    assert line["config"]["pools_total"] == 2 * line["config"]["pools_per_gpu"]
    assert line["collective_check_rel_err"] <= 1e-12
    par = line["parity"]
    assert par["netflow_rel_err_at_fixed_v"] <= 1e-12 and par["dual_rel_err"] <= 1e-12
    assert par["route_sharded_netflow_rel_err"] <= 1e-6
    rs = line["route_sharded"]
    assert "error" not in rs and rs["ranks_agree_on_v"] and rs["pools_total"] == line["config"]["pools_total"]
    ss = line["strong_scaling"]
    assert ss["pools_total"] == 4_000_000 and ss["pools_per_gpu"] == 2_000_000 and ss["collective_check_rel_err"] <= 1e-12
    # the `collectives` block: all three keys on the weak and the strong leg; two processes on one GPU can
    # run the peer exchange and torch.distributed (gloo here), not RCCL -- which says so instead of hanging
    for col in (line["collectives"], ss["collectives"]):
        assert set(col) == {"peer", "rccl_library", "rccl_torch"}
        assert col["peer"]["ok"] and col["peer"]["check_rel_err"] <= 1e-12 and col["peer"]["peer_ranks"] == 2
        assert col["rccl_torch"]["ok"] and col["rccl_torch"]["check_rel_err"] <= 1e-12
        assert not col["rccl_library"]["ok"] and "one device per rank" in col["rccl_library"]["why_not"]
    assert line["collective"]["headline"] == "peer"
    assert line["cpu_baseline"]["value"] > 0
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    json.dump(line, open(os.path.join(ROOT, "gpurun_out", "bench_rehearsal_world2.json"), "w"), indent=1)

