"""-m gpu: the N > 1 code path of bench.py (RCCL process group, StepPipeline with an asynchronous all-gather per lane) executed
on hardware with ONE rank.  It claims nothing about scaling — the driver's SCALE run owns that — but the collective path, its
stream ordering and the lane reuse logic run on a real MI355X in the driver's pytest."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_rccl_one_rank_step_pipeline(dev):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_rccl_worker.py")
    env = {**os.environ, "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    r = subprocess.run([sys.executable, worker, str(port)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RCCL_SMOKE_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_rccl_one_rank_bench_c5_sharded_retrieval(dev):
    """`bench.py --workload c5` on its N > 1 path with ONE rank (--force-dist: RCCL group, the embeddings all-gather, the sharded
    retrieval = local exact top-k + all-gather of the [C, k] candidates + merge): the line carries a retrieval object whose result
    equals the unsharded retrieve_topk over the gathered embeddings.  A 2-layer tower (--c5-layers 2) keeps the host-side weight
    generation short; the collective path does not depend on the depth."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {**os.environ, "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c5", "--force-dist", "--c5-layers", "2", "--batch", "16",
                        "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-second-precision"], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["retrieval"]["equals_unsharded_on_rank0"] is True and d["retrieval"]["k"] == 16 and d["retrieval"]["categories"] == 919
    assert d["value"] > 0 and "NOT CONFIG 5" in d["config"]["workload"]


def test_rccl_one_rank_bench_headline_force_dist(dev):
    """The headline workload of `bench.py` on its N > 1 path with ONE rank (--force-dist): RCCL group, three lanes, the asynchronous
    all-gather of the low-res logits per step on each lane's stream — the line carries the collective, and the timed lanes' outputs are
    still bitwise an eager step."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {**os.environ, "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--force-dist", "--steps", "6", "--warmup", "3", "--full", "--no-cpu-baseline",
                        "--no-torch-gpu-baseline", "--no-second-precision", "--no-io-rates", "--no-batch1", "--no-configs", "--no-live-traffic"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["timed_outputs_checked"] is True and "all_gather" in d["config"]["collective"] and d["n_gpus"] == 1 and d["value"] > 0
    # the line proves its collective (round-5 review: the gathered buffers were never looked at): every timed step's gather was retired,
    # slice r of lane 0's gathered logits checksums to rank r's payload, and the per-step gather costs (nearly) nothing on one rank —
    # so `value` under --force-dist is the plain N = 1 value within noise (same process, same lanes, with and without the gather)
    c = d["collective"]
    assert c["ranks_in_gather"] == 1 and c["verified"] is True and c["gathers_retired_in_timed_region"] == 6 and c["steps"] == 6
    assert c["bytes_per_rank"] == 32 * 81 * 42 * 42 * 4 and "rccl" in c["backend"] and c["mismatching_slices_on_this_rank"] == []
    assert abs(c["gather_ms_exposed"]) < 0.06 * d["ms_per_step"], c
    assert abs(c["ms_per_step_without_gather"] - d["ms_per_step"]) < 0.06 * d["ms_per_step"], (c, d["ms_per_step"])
    assert c["per_rank_images_per_s"]["min"] <= d["value"] * 1.001 and c["per_rank_images_per_s"]["max"] >= c["per_rank_images_per_s"]["min"]
    assert d["summary"]["coll"]["ok"] is True and d["summary"]["coll"]["ranks"] == 1 and list(d)[-1] == "summary"
