"""bench.py's N-rank flow on real hardware: three processes share cuda:0 (gloo backend instead of RCCL, which
refuses two ranks on one device) -- pixel tiles round-robin, deferred submission, one film reduce onto rank 0,
MAX-over-ranks timing, JSON as the last stdout line -- and the reduced film equals the 1-process render
byte for byte (as PNG)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cmd, env_extra, tmp_path, tag):
    env = dict(os.environ)
    env.update(env_extra)
    out = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    last = out.stdout.decode().strip().splitlines()[-1]
    return json.loads(last)


def free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_three_ranks_on_one_device_equal_one_process(gpu_ctx_ok, tmp_path):
    common = ["--steps", "3", "--warmup", "1", "--frames-per-step", "4", "--size", "320", "--ntri", "20000",
              "--tile-size", "1024", "--no-cpu-baseline", "--no-roofline"]
    one = run([sys.executable, "bench.py"] + common + ["--save-png", str(tmp_path / "one.png")], {}, tmp_path, "one")
    three = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
                 "--master-port", str(free_port()), "bench.py", "--gpus", "3"] + common + ["--save-png", str(tmp_path / "three.png")],
                {"TIRT_BENCH_ONE_DEVICE": "1", "TIRT_BENCH_BACKEND": "gloo"}, tmp_path, "three")
    assert three["n_gpus"] == 3 and one["n_gpus"] == 1 and three["scaling"] == "strong"
    assert three["rays"] == one["rays"]                       # every pixel-sample traced exactly once across the ranks
    assert (tmp_path / "one.png").read_bytes() == (tmp_path / "three.png").read_bytes()


def test_gpus_3_typed_without_a_launcher(gpu_ctx_ok, tmp_path):
    """`python bench.py --gpus 3 ...` exactly as typed (no torch.distributed.run in front, no WORLD_SIZE): bench.py starts its own
    ranks; same rays and the same PNG as one process."""
    common = ["--steps", "2", "--warmup", "1", "--frames-per-step", "4", "--size", "320", "--ntri", "20000",
              "--tile-size", "1024", "--no-cpu-baseline", "--no-roofline"]
    one = run([sys.executable, "bench.py"] + common + ["--save-png", str(tmp_path / "one.png")], {}, tmp_path, "one")
    env = {"TIRT_BENCH_ONE_DEVICE": "1", "TIRT_BENCH_BACKEND": "gloo"}
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        assert k not in os.environ
    three = run([sys.executable, "bench.py", "--gpus", "3"] + common + ["--save-png", str(tmp_path / "three.png")], env, tmp_path, "three")
    assert three["n_gpus"] == 3 and three["rays"] == one["rays"]
    assert (tmp_path / "one.png").read_bytes() == (tmp_path / "three.png").read_bytes()


def test_force_dist_one_rank_rccl(gpu_ctx_ok, tmp_path):
    """The N > 1 code path through RCCL itself with the one rank a 1-GPU box allows: communicator set-up, hash all-gather, film reduce."""
    r = run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames-per-step", "4", "--size", "256",
             "--ntri", "20000", "--no-cpu-baseline", "--no-roofline"], {"TIRT_FORCE_DIST": "1"}, tmp_path, "force")
    assert r["n_gpus"] == 1 and r["distributed"]["rccl_ranks"] == 1 and r["distributed"]["backend"] == "nccl"


def test_bench_line_carries_the_contract_fields(gpu_ctx_ok, tmp_path):
    """One JSON line, last on stdout, with the driver's fields, a `roofline` object measured in this run (HIP-event launch duration, rocprofv3 --pmc child
    passes for the traffic) and a `cpu_baseline` object (the CPU oracle on a bounded sample); small sizes, same code path as the --full run."""
    r = run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--frames-per-step", "16", "--size", "512", "--ntri", "20000",
             "--full", "--no-configs", "--cpu-target-s", "1.5"], {}, tmp_path, "contract")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in r, k
    assert r["unit"] == "Mrays/s" and r["n_gpus"] == 1 and r["steps"] == 2 and r["dtype"] == "f32" and r["vs_baseline"] is None and "workload" in r["config"]
    roof = r["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "fractions", "bound_evidence"):
        assert k in roof, k
    # (round 5 ran this at 256^2 x 8 frames -- launches of half a million rays, mostly launch latency: frac 0.048 -- and lowered the bound to 0.01 when 0.05 failed
    # once; the run is now 512^2 x 16 frames, 4 Mi paths per batch, where the fraction is a property of the kernel: 0.05 again)
    assert roof["bound"] == "gather" and 0.05 < roof["frac"] < 1.5 and roof["traffic"] and roof["traffic"] > 0
    assert roof["bound_by_largest_fraction_of_this_run"]["bound"] in roof["fractions"]
    # everything a render pays for is inside the clock: the candidate lists are made again in the timed region (batches of 16 frames use them)
    pb = r["primary_beams"]
    assert pb["list_builds_in_timed_region"] == 1 and pb["prepare_ms_in_timed_region"] > 0.0 and pb["camera_rays_through_lists"] == 2 * 16 * 512 * 512
    assert r["value_cold_256spp"] > 0 and r["cold_256spp"]["list_builds"] == 1
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    cb = r["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb


def test_plain_run_is_the_headline_only_and_dumps_a_reproducible_film(gpu_ctx_ok, tmp_path):
    """Without --full the line carries the headline and nothing measured beside it; --dump-outputs writes the film the timed steps left,
    the same bits from run to run (seeded inputs), and --steps sets the number of timed steps."""
    import numpy as np
    common = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--frames-per-step", "4", "--size", "256", "--ntri", "20000"]
    films = []
    for tag in ("a", "b"):
        r = run([sys.executable, "bench.py"] + common + ["--dump-outputs", str(tmp_path / tag)], {}, tmp_path, tag)
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in r, k
        assert r["steps"] == 3 and r["value"] > 0 and r["ms_per_step"] > 0 and r["unit"] == "Mrays/s"
        assert r["rays"]["paths"] == 3 * 4 * 256 * 256
        for k in ("roofline", "cpu_baseline", "configs", "value_cold_256spp", "oracle_sample_identical", "build_detail"):
            assert k not in r, k
        films.append(np.load(str(tmp_path / tag / "film_hdr.npy")))
    assert films[0].dtype == np.float32 and films[0].shape == (256, 256, 3) and np.isfinite(films[0]).any() and films[0].any()
    assert np.array_equal(films[0], films[1], equal_nan=True)
