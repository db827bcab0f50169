"""`python bench.py --gpus N` is the N-rank job: without a launcher around it the file starts its own ranks under
torch.distributed.run, one per GPU; with fewer GPUs than ranks it fails at once instead of printing a 1-GPU line for an N-GPU request.
Everything here runs on a box without a GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH, *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def gpu_count():
    import torch
    return torch.cuda.device_count()


def test_more_gpus_asked_for_than_present_fails_at_once_and_prints_no_line():
    n = gpu_count() + 2
    r = run(["--gpus", str(n), "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert f"needs {n} GPUs, found {gpu_count()}" in r.stderr
    assert '"n_gpus"' not in r.stdout, "no measurement line for a request that cannot be served"


def test_launch_check_starts_one_rank_per_requested_gpu_without_touching_one():
    r = run(["--gpus", "2", "--launch-check"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["launch_check"] == "ok" and line["n_ranks"] == 2
    ranks = sorted(line["ranks"], key=lambda e: e["rank"])
    assert [e["rank"] for e in ranks] == [0, 1] and [e["local_rank"] for e in ranks] == [0, 1]
    assert all(e["world_size"] == 2 and e["env"]["WORLD_SIZE"] == "2" and e["env"]["MASTER_ADDR"] == "127.0.0.1" for e in ranks)
    assert ranks[0]["pid"] != ranks[1]["pid"], "one process per GPU"


def test_a_launcher_with_another_world_size_than_gpus_is_refused():
    """WORLD_SIZE from a launcher that disagrees with --gpus: never an n_gpus line for another N than the one asked for"""
    r = run(["--gpus", "4", "--launch-check"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "--gpus 4 but WORLD_SIZE=1" in r.stderr
    r = run(["--gpus", "1", "--launch-check"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "--gpus 1 but WORLD_SIZE=2" in r.stderr


def test_config4_takes_the_same_launcher():
    n = gpu_count() + 2
    r = run(["--gpus", str(n), "--config", "4", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0 and f"needs {n} GPUs" in r.stderr and '"n_gpus"' not in r.stdout


def test_summary_is_the_last_key_and_names_every_secondary_row():
    sys.path.insert(0, ROOT)
    import bench
    line = {"ms_per_step": 0.78, "roofline": {"frac": 0.6, "whole_path_frac": 0.5}, "cpu_baseline": {"value": 2700.0},
            "extra": {"config3_cell_errors": {"ms_per_step": 0.85}, "config4_n1": {"value": 2e5, "without_solve": {"frames_per_s": 6e5}},
                      "config5_extract_4096": {"captures_per_s": 45000.0}, "single_frame": {"ms_per_frame": 0.19}, "mode66": {"threshold_hbm_frac": 0.52},
                      "ingest": {"error": "x"}}}
    s = bench.summary(line)
    assert s["configs2_ms_per_step"] == 0.85 and s["configs3_n1_without_solve"] == 6e5 and s["configs4_captures_per_s"]["4096"] == 45000.0
    assert s["single_frame_ms"] == 0.19 and s["mode_k1_frac"]["66"] == 0.52 and s["mode_k1_frac"]["67"] is None
    assert len(json.dumps(s)) < 1500, "must fit the tail of the line the driver records"


def test_bad_step_counts_and_dump_outside_the_default_workload_are_refused():
    for args in (["--steps", "0"], ["--reps", "0"], ["--warmup", "-1"], ["--config", "4", "--dump-outputs", "out"]):
        r = run(args)
        assert r.returncode != 0 and "error:" in r.stderr and '"n_gpus"' not in r.stdout, args


@pytest.mark.gpu
def test_steps_is_the_timed_region_and_the_dump_holds_the_last_step(tmp_path):
    import numpy as np
    from libcimbar_amd import framegen, modeb
    if gpu_count() == 0:
        pytest.skip("no GPU")
    n = 64
    r = run(["--steps", "3", "--warmup", "1", "--frames", str(n), "--no-cpu-baseline", "--no-extras", "--dump-outputs", str(tmp_path)], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["timed_region"]["repetitions"] == 1 and line["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path)) == ["chunks.npy", "masks.npy"]
    chunks, masks = np.load(tmp_path / "chunks.npy"), np.load(tmp_path / "masks.npy")
    assert chunks.dtype == masks.dtype == np.float32 and chunks.shape == (n, modeb.FRAME_BYTES) and masks.shape == (n,)
    assert (masks == 0xFFF).all()
    # the last timed step decoded one of the rotated input batches (rank 0: seed 1234 + 7919 b), bit for bit
    assert any((chunks == framegen.synth_payload(n, seed=1234 + 7919 * b).numpy()).all() for b in range(16))


@pytest.mark.gpu
def test_a_plain_run_prints_the_headline_alone_and_full_adds_the_rest():
    """a plain run sets up, warms up, times its steps and prints the headline; per-kernel figures and secondary rows come with --full"""
    if gpu_count() == 0:
        pytest.skip("no GPU")
    moved = ("roofline", "stage_ms", "no_pipeline", "cpu_baseline", "payload_sha_match", "extra", "summary")
    r = run(["--steps", "3", "--warmup", "1", "--frames", "64"], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["metric"] == "decoded cimbar frames/s (1024x1024 mode-B)" and line["unit"] == "frames/s" and line["dtype"] == "u8"
    assert line["higher_is_better"] is True and line["steps"] == 3 and line["ms_per_step"] > 0
    assert abs(line["value"] - 64 * 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]
    assert not [k for k in moved if k in line], "a plain run measures the headline alone"
    r = run(["--steps", "3", "--warmup", "1", "--frames", "64", "--full", "--no-cpu-baseline", "--no-extras"], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["stage_ms"]["threshold"] > 0 and line["roofline"]["bound"] == "hbm" and line["no_pipeline"]["ms_per_step"] > 0
    assert "cpu_baseline" not in line and "extra" not in line and list(line)[-1] == "summary"
