"""CPU suite: `bench.py --gpus N` really starts N ranks, its end-to-end leg (root scatter -> decode -> root gather, with
--full) moves the right bytes, and a plain run is the headline alone.  Runs the benchmark's own code on gloo with the
oracle as the block codec (--dry-gloo)."""
import importlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("gpus", [2, 3])
def test_bench_gpus_n_spawns_n_ranks(gpus, oracle):
    env = dict(os.environ, RCX_BENCH_DRY_CODEC="_dry_codec", PYTHONPATH=os.path.join(ROOT, "tests") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--dry-gloo", "--full", "--nblocks", "5", "--steps", "2", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == gpus and res["steps"] == 2 and res["scaling"] == "weak"
    e = res["end_to_end"]
    assert e["verified"] is True and e["bytes_gathered"] == (gpus - 1) * 5 * 65536 and e["bytes_scattered"] > 0
    assert e["scatter_ms"] > 0 and e["gather_ms"] > 0 and "gloo" in e["transport"]
    # BASELINE config 5's sharding: ONE stream's RCXQ container split by block ranges, scattered, decoded per rank, gathered ==
    # the source; and raw ranges scattered, encoded per rank, the containers gathered and joined == what one device writes
    c5 = [o for o in res["other_configs"] if o.get("config") == 5][0]
    assert c5["n_gpus"] == gpus and c5["sharded_container_verified"] is True and c5["joined_equals_single_device"] is True
    assert sum(c5["block_ranges"]) == c5["blocks"] == 11 and len(c5["block_ranges"]) == gpus and min(c5["block_ranges"]) >= 1


@pytest.mark.parametrize("gpus", [2, 3])
def test_bench_line_survives_a_rank_failing_inside_the_scatter(gpus, oracle):
    """A side leg that dies on ONE rank in the middle of a collective exchange (here: rank 1 raises inside the end-to-end leg's
    scatter, its peers are left waiting) must not cost the headline: rank 0 still prints exactly one line, with the value,
    and the failed leg reported as {"error": ...}."""
    env = dict(os.environ, RCX_BENCH_DRY_CODEC="_dry_codec_faulty", RCX_DRY_FAULT_RANK="1", RCX_BENCH_PG_TIMEOUT="6", RCX_BENCH_SIDE_TIMEOUT="120",
               PYTHONPATH=os.path.join(ROOT, "tests") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--dry-gloo", "--full", "--nblocks", "5", "--steps", "2", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:] + p.stderr[-3000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == gpus and res["value"] > 0 and res["ms_per_step"] > 0 and res["roofline"]["frac"] > 0
    assert "error" in res["end_to_end"] and "end_to_end" in res["side_legs_failed"]
    # what came after the failed leg and needs the process group is skipped, not attempted on a group in an unknown state
    assert all("error" in o for o in res["other_configs"])


def test_bench_watchdog_prints_the_line_when_a_leg_hangs(oracle):
    """The same with the process group's own timeout far away (what RCCL looks like: a stuck collective never raises): the
    watchdog ends the legs and rank 0's line is still there."""
    env = dict(os.environ, RCX_BENCH_DRY_CODEC="_dry_codec_faulty", RCX_DRY_FAULT_RANK="1", RCX_BENCH_PG_TIMEOUT="600", RCX_BENCH_SIDE_TIMEOUT="12",
               PYTHONPATH=os.path.join(ROOT, "tests") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-gloo", "--full", "--nblocks", "5", "--steps", "2", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:] + p.stderr[-3000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["value"] > 0 and "side_legs_note" in res


def test_bench_single_rank_dry(oracle):
    env = dict(os.environ, RCX_BENCH_DRY_CODEC="_dry_codec", PYTHONPATH=os.path.join(ROOT, "tests") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-gloo", "--full", "--nblocks", "4", "--steps", "2", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert res["n_gpus"] == 1 and res["end_to_end"]["verified"] is True and res["end_to_end"]["bytes_gathered"] == 0
    assert res["other_configs"][0]["sharded_container_verified"] is True


@pytest.mark.parametrize("gpus", [1, 2])
def test_bench_plain_run_is_the_headline_alone(gpus, oracle):
    """Without --full the line is the headline and nothing more: no side leg runs, on one rank or several.  The faulty codec
    would make rank 1's end-to-end leg raise, so a plain run at world 2 that reached it would report a failed leg."""
    env = dict(os.environ, RCX_BENCH_DRY_CODEC="_dry_codec_faulty", RCX_DRY_FAULT_RANK="1",
               PYTHONPATH=os.path.join(ROOT, "tests") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--dry-gloo", "--nblocks", "4", "--steps", "3", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["metric"] == "GiB/s decoded output (batched blocks)" and res["unit"] == "GiB/s" and res["higher_is_better"] is True
    assert res["dtype"] == "u8" and res["value"] > 0 and res["ms_per_step"] > 0 and res["steps"] == 3 and res["warmup"] == 1
    assert res["n_gpus"] == gpus and res["end_to_end"] is None and list(res["per_distribution"]) == ["G-text"]
    side = ("other_configs", "sustained", "host_path", "cpu_baseline", "single_stream", "hbm_ceiling_measured", "extras",
            "rccl_self_sendrecv", "side_legs_failed", "side_legs_note")
    assert not [k for k in side if k in res]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-gloo", "--extras"], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 2 and "--full" in p.stderr


def test_container_split_join(oracle):
    """pipeline.split_container / join_containers: every shard is a valid container of its block range, and the shards joined
    in rank order are the stream again, byte for byte (the container one device writes)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import _dry_codec as D
    from rust_compress_amd import pipeline as P, dist, synth
    data = synth.gen("text", 9 * 2048 + 77, 3).tobytes()
    whole = D.pipe_encode(data, 2048)
    bs, parts, lens, praw, clen, p = P.parse_container(whole)
    assert bs == 2048 and parts == 16 and lens.tolist() == [2048] * 9 + [77]
    for world in (1, 2, 3, 7, 12):
        bounds = dist.partition(lens, world)
        shards = P.split_container(whole, bounds)
        assert len(shards) == world and P.join_containers(shards) == whole
        assert b"".join(D.pipe_decode(x) for x in shards) == data
    with pytest.raises(P.ContainerError):
        P.parse_container(whole[:40])
    with pytest.raises(P.ContainerError):
        P.join_containers([whole, D.pipe_encode(data[:100], 1024)])


def test_bench_dump_outputs_is_the_last_steps_result_and_repeats(oracle, tmp_path):
    """--dump-outputs DIR: float arrays of what the timed decode returned, within 64 MB, the same from run to run; --steps is
    the number of timed steps and the line carries ms_per_step."""
    env = dict(os.environ, RCX_BENCH_DRY_CODEC="_dry_codec", PYTHONPATH=os.path.join(ROOT, "tests") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    dumps = []
    for run in range(2):
        d = tmp_path / ("dump%d" % run)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-gloo", "--nblocks", "3", "--steps", "3", "--warmup", "1",
                            "--no-e2e", "--no-others", "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        assert res["steps"] == 3 and res["ms_per_step"] > 0
        files = sorted(os.listdir(d))
        assert files == ["block_crc32.npy", "block_out_len.npy", "block_status.npy", "sample_block_index.npy", "sample_decoded_bytes.npy"]
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        dumps.append({f[:-4]: np.load(d / f) for f in files})
    a, b = dumps
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert (a["block_status"] == 0).all() and (a["block_out_len"] == 65536).all() and a["sample_block_index"].tolist() == [0, 1, 2]
    raw = a["sample_decoded_bytes"].astype(np.uint8)
    assert [zlib.crc32(r.tobytes()) for r in raw] == a["block_crc32"].astype(np.int64).tolist()
    _, raws = importlib.import_module("_dry_codec").make_blocks("text", 3, 65536, 0x4C5A3401)
    assert [r.tobytes() for r in raw] == raws
