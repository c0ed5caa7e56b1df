"""bench.py on the GPU box: the contract line, and the distributed path with a real RCCL communicator on one rank
(DABGPU_FORCE_DIST=1) -- what the driver's N = 2, 4, 8 launches initialise, exercised where only one GPU is leased."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def run_bench(extra_args, extra_env, timeout=600):
    env = dict(os.environ, **extra_env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--frames", "64", "--no-extra", "--no-cpu-baseline"] + extra_args,
                       env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout                       # ONE JSON line on stdout, nothing else (RCCL's banner goes to stderr)
    return json.loads(lines[0])


def test_bench_line_single_process():
    d = run_bench([], {})
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["unit"] == "frames/s" and d["value"] > 0
    assert d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] < 1
    assert d["config"]["frames_per_step_per_gpu"] == 64


def test_plain_bench_times_the_headline_only_and_dumps_what_its_last_step_computed(tmp_path):
    """A plain run (no --full) prints the line without the secondary figures; --dump-outputs writes a seeded sample of whole
    frames of the IQ its timed path returned -- the same in two runs, and the oracle's chain on the same input bits (drawn on
    the device from a generator seeded with 42 on rank 0)."""
    import numpy as np
    import torch
    import oracle as O
    dumps = []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        line = run_bench(["--steps", "3", "--dump-outputs", d], {})
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
        assert not {"other_workloads", "cpu_baseline"} & set(line) and "peak_measured_GBps" not in line["roofline"]
        dumps.append((np.load(os.path.join(d, "iq.npy")), np.load(os.path.join(d, "iq_frames.npy"))))
    (iq, idx), (iq2, idx2) = dumps
    assert iq.dtype == np.float32 and iq.shape == (32, 196608, 2) and iq.nbytes + idx.nbytes <= 64 << 20
    assert idx.dtype == np.float64 and len(set(idx.tolist())) == 32 and 0 <= idx.min() and idx.max() < 64
    assert np.array_equal(idx, idx2) and np.array_equal(iq, iq2)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(42)
    bits = torch.randint(0, 256, (64, 28800), dtype=torch.uint8, device="cuda:0", generator=gen).cpu().numpy()
    ref = O.Chain(mode=1, stages=3, gain_mode=2, normalise=1.0 / 50000.0).process(bits[idx.astype(np.int64)])
    y = iq[..., 0] + 1j * iq[..., 1]
    for f in range(len(idx)):
        assert np.linalg.norm(y[f] - ref[f]) / np.linalg.norm(ref[f]) < 1e-6, f


def test_bench_with_a_real_rccl_communicator_on_one_rank():
    """torch.distributed over RCCL initialised for WORLD_SIZE = 1: barrier, all_reduce(MAX) and the optional IQ
    gather run through the same code as on N ranks."""
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    env = {"DABGPU_FORCE_DIST": "1", "RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1", "MASTER_ADDR": "127.0.0.1",
           "MASTER_PORT": str(port), "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    d = run_bench(["--gather", "8"], env)
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["scaling"] == "weak"
    g = d["iq_gather"]
    assert g["frames_per_rank"] == 8 and g["bytes_per_rank"] == 8 * 196608 * 8 and g["ranks"] == 1 and g["ms"] > 0


def test_bench_gpus_2_launches_two_ranks():
    """`python bench.py --gpus 2` with no launcher around it starts two ranks itself.  One GPU is leased here, so both
    ranks drive device 0 (DABGPU_BENCH_DEVICES) and talk over gloo; the line must say n_gpus = 2 and its value must be
    both ranks' frames over the slower rank's time."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(DABGPU_BENCH_DEVICES="0,0", DABGPU_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
                        "--frames", "256", "--no-extra", "--no-cpu-baseline"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["config"]["frames_per_step_per_gpu"] == 256
    assert abs(d["value"] - 2 * 256 * 4 / (d["ms_per_step"] * 4e-3)) / d["value"] < 1e-3
    one = run_bench([], {})                       # the one-rank line is what it was
    assert one["n_gpus"] == 1


def test_bench_gpus_2_on_the_full_chain_of_config_5():
    """BASELINE config 5 says "full chain": two ranks of `bench.py --gpus 2 --workload cfg4` (frame kernel -> x4 resampler
    with the polynomial predistorter), both on the one leased GPU over gloo -- the cfg 4 allocations (native-rate
    intermediate, 4x output) and the per-rank resampler state under the launcher."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(DABGPU_BENCH_DEVICES="0,0", DABGPU_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "cfg4", "--steps", "3",
                        "--warmup", "1", "--frames", "128", "--no-extra", "--no-cpu-baseline"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["frames_per_step_per_gpu"] == 128 and "config 4" in d["config"]["workload"]
    assert d["roofline"]["algorithmic_bytes_per_frame"] == 28800 + 6291456 and d["value"] > 0
    assert abs(d["value"] - 2 * 128 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-3


def test_bench_gpus_2_with_the_iq_gather_at_world_size_2():
    """The optional final IQ gather (north_star; StreamGroup.gather_to_root) at world size 2 UNDER THE LAUNCHER: two ranks
    on the one leased GPU, gloo (which gathers host tensors: the harness stages them), 8 frames per rank to rank 0 -- the
    line carries iq_gather with ranks = 2 and the bytes of one rank's piece."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(DABGPU_BENCH_DEVICES="0,0", DABGPU_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--frames", "64", "--gather", "8", "--no-extra", "--no-cpu-baseline"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0
    g = d["iq_gather"]
    assert g["ranks"] == 2 and g["frames_per_rank"] == 8 and g["bytes_per_rank"] == 8 * 196608 * 8
    assert g["ms"] > 0 and g["GBps_into_rank0"] > 0


def test_bench_gpus_8_ranks_with_real_kernels_on_the_one_gpu():
    """The driver's largest scan point with REAL kernels: eight ranks of `bench.py --gpus 8`, all on the one leased GPU
    (DABGPU_BENCH_DEVICES, gloo) -- eight processes importing torch, creating contexts and modulating side by side, the barrier and
    the MAX-reduce at world size 8, one line.  Small batches: the eight share 288 GB and one set of CUs."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(DABGPU_BENCH_DEVICES="0,0,0,0,0,0,0,0", DABGPU_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "3", "--warmup", "1",
                        "--frames", "256", "--no-extra", "--no-cpu-baseline"], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["steps"] == 3 and d["config"]["frames_per_step_per_gpu"] == 256
    assert d["config"]["devices"] == [0] * 8 if "devices" in d["config"] else True
    assert abs(d["value"] - 8 * 256 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-3
    assert d["scaling"] == "weak" and d["roofline"]["frac"] > 0


def test_bench_gpus_beyond_the_node_fails_loudly():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "DABGPU_BENCH_DEVICES")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--steps", "1"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "needs devices" in r.stderr and not r.stdout.strip()


@pytest.mark.parametrize("fmt", [None, "s16"])
def test_streaming_host_path_is_not_slower_than_the_synchronous_call(tmp_path, fmt):
    """VERDICT r05 item 7 (profiles/r06_hostpath_bisect.txt: not a source regression -- four source states, one box, the
    same rates; the halved figures came from a single short repetition right behind a five-call warm-up).  Measured the
    robust way (tools/time_host_path.py: warm-up by time, median of five repetitions), submit / collect at 32 frames per
    batch must reach 95 % of the synchronous call at the same batch size and 92 % of it at its best batch size (256 frames per
    call, which sits on the PCIe link as well), and its median must not be a slow-start artefact (spread of the repetitions
    within 40 %)."""
    out = str(tmp_path / "host_path.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "time_host_path.py")] + ([fmt] if fmt else []) +
                       ["--json", out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.load(open(out))
    a32 = d["async"]["32"]
    best_sync = max(v["frames_per_s"] for v in d["sync"].values())
    # (measured on eight boxes of round 6: 1.02 ... 1.03 x the best synchronous batch for complexf, 0.995 ... 1.04 x for s16, which
    #  sits on the link at 256 frames per synchronous call too; 1.08 ... 1.11 x the synchronous call at the same 32 frames)
    assert a32["frames_per_s"] >= 0.95 * d["sync"]["32"]["frames_per_s"], (a32, d["sync"]["32"])      # the verdict's criterion
    assert a32["frames_per_s"] >= 0.92 * best_sync, (a32, best_sync)
    assert a32["min"] >= 0.6 * a32["max"], a32
    for B in ("1", "8"):
        assert d["async"][B]["frames_per_s"] >= 0.95 * d["sync"][B]["frames_per_s"], (B, d["async"][B], d["sync"][B])


def test_bench_falls_back_to_a_batch_that_fits_the_free_memory():
    """A rank that cannot get the buffers of --frames (another tenant on the GPU; here: an absurd request, 400 000 frames =
    640 GB) halves the batch until they fit and says so on the line -- the driver's 8-GPU run must not die of one rank's
    hipErrorOutOfMemory."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--frames", "400000", "--no-extra", "--no-cpu-baseline", "--counters", "off"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
    b = d["config"]["frames_per_step_per_gpu"]
    assert b < 400000 and b in (200000, 100000, 50000, 25000, 12500) and "did not fit" in d["config"]["frames_note"]
    assert d["value"] > 0 and 0 < d["roofline"]["frac"] < 1
