"""CPU: the parts of bench.py that run without a GPU — the entry re-exports what tests / tools use from benchlib/, and the live
counter-pass helper returns THREE values on every path (round-5 advisor: its two early exits returned two and the caller's unpack
raised after the timed run, so the line was never printed)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_entry_reexports_the_parts():
    import bench
    for name in ("build_lanes", "make_launch", "check_timed_outputs", "rank_launch_command", "launch_ranks", "gemm_roofline", "live_pmc_traffic",
                 "c3_model", "c3_parity", "batch1_object", "solver_object", "pseudo_label_object", "c4_object", "c5_object", "main"):
        assert callable(getattr(bench, name)), name
    assert bench.MFMA_F16_DENSE_PEAK_TFLOPS == 2500.0 and bench.PRECISION_DTYPE["exact"].startswith("f16x3")
    n = sum(1 for _ in open(os.path.join(ROOT, "bench.py")))
    assert n < 120, f"bench.py is the entry point only ({n} lines): measurement code belongs in benchlib/"


def test_live_traffic_refuses_nested_profiling_with_three_values(monkeypatch):
    from benchlib import roofline
    monkeypatch.setenv("ROCPROF_FOO", "1")
    traffic, note, per = roofline.live_pmc_traffic(["--precision", "exact"], 1)
    assert traffic is None and per is None and "being profiled" in note
    monkeypatch.delenv("ROCPROF_FOO")
    monkeypatch.setenv("LD_PRELOAD", "/opt/rocm/lib/librocprofiler-sdk-tool.so")
    traffic, note, per = roofline.live_pmc_traffic([], 0)
    assert traffic is None and per is None and "being profiled" in note


def test_live_traffic_without_rocprofv3_returns_three_values(monkeypatch, tmp_path):
    from benchlib import roofline
    for k in [k for k in os.environ if k.startswith(("ROCPROF", "ROCP_"))]:
        monkeypatch.delenv(k)
    monkeypatch.setenv("PATH", str(tmp_path))                       # no rocprofv3 on PATH ...
    monkeypatch.setattr(roofline, "ROCPROFV3_FALLBACK", str(tmp_path / "rocprofv3"))   # ... nor at the ROCm location
    traffic, note, per = roofline.live_pmc_traffic([], 1)
    assert traffic is None and per is None and note == "rocprofv3 not found"


def test_live_traffic_failed_pass_returns_three_values(monkeypatch, tmp_path):
    """A profiler that exits non-zero (refused / crashed): reported, never fatal."""
    from benchlib import roofline
    for k in [k for k in os.environ if k.startswith(("ROCPROF", "ROCP_"))]:
        monkeypatch.delenv(k)
    fake = tmp_path / "rocprofv3"
    fake.write_text("#!/bin/sh\nexit 7\n")
    fake.chmod(0o755)
    monkeypatch.setenv("PATH", str(tmp_path) + os.pathsep + os.environ["PATH"])
    traffic, note, per = roofline.live_pmc_traffic([], 1, timeout_s=30)
    assert traffic is None and per is None and "failed" in note


def test_dump_outputs_float32_within_budget_same_sample_every_run(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 files, at most the budget in all, and an over-budget array is written as the same seeded sample
    of its elements every run (two builds compare element for element)."""
    import numpy as np
    import torch
    from benchlib import common
    monkeypatch.setattr(common, "DUMP_BUDGET_BYTES", 1 << 16)
    labels = torch.arange(12, dtype=torch.int64).reshape(3, 4)
    logits = np.random.default_rng(1).standard_normal(100000)
    for d in ("a", "b"):
        common.dump_outputs(str(tmp_path / d), {"labels": labels, "logits": logits})
    assert sorted(os.listdir(tmp_path / "a")) == ["labels.npy", "logits_sample.npy"]
    lab = np.load(tmp_path / "a" / "labels.npy")
    assert lab.dtype == np.float32 and np.array_equal(lab, labels.numpy())
    s1, s2 = np.load(tmp_path / "a" / "logits_sample.npy"), np.load(tmp_path / "b" / "logits_sample.npy")
    assert s1.dtype == np.float32 and np.array_equal(s1, s2) and np.isin(s1, logits.astype(np.float32)).all()
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= (1 << 16) + 2 * 128
