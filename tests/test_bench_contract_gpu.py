"""-m gpu: the driver's contract with bench.py, checked on hardware with a shortened run: ONE JSON line on stdout (last line), the contract's
keys with the right types; under `--full` the `roofline` and `cpu_baseline` objects, the timed outputs checked, the bounded objects of the
other BASELINE configs, and the compact `summary` as the LAST key (the driver keeps the tail of stdout); a plain run only times, and
`--dump-outputs` writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_workload_line_contract(dev):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--full", "--cpu-sample", "2",
                        "--no-cpu-all-cores", "--no-live-traffic", "--no-io-rates"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    d = json.loads(lines[-1])                                   # the result is the LAST line (RCCL / library banners may precede it)
    assert sum(1 for ln in lines if ln.startswith("{")) == 1
    for k, t in (("metric", str), ("value", (int, float)), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int), ("ms_per_step", (int, float)),
                 ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict)):
        assert isinstance(d[k], t), (k, d[k])
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["scaling"] == "weak" and d["higher_is_better"] is True
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and d["unit"] == "images/s" and "workload" in d["config"]
    assert abs(d["value"] - 32 * 1e3 / d["ms_per_step"]) / d["value"] < 0.01          # whole-job images/s == batch / step time
    roof = d["roofline"]
    assert roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s" and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3 and 0.2 < roof["frac"] < 1.0
    cpu = d["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["sample"]
    # what was timed was checked, and the parity legs look at the timed outputs
    assert d["timed_outputs_checked"] is True and d["parity"]["timed_outputs_bitwise_equal_eager"] is True
    assert d["parity"]["logit_max_abs_err"] < 2e-5 and d["parity"]["unexplained_label_mismatches"] == 0
    sp = d["second_precision"]
    assert sp["mode"] == "fast" and sp["parity"]["timed_outputs_bitwise_equal_eager"] is True and sp["parity"]["logit_max_abs_err"] < 1e-3
    # the other BASELINE configs, bounded, in the same line
    assert d["c4"]["timed_outputs_bitwise_equal_eager"] is True and d["c4"]["parity"]["logit_max_abs_err"] < 2e-5 and d["c4"]["value"] > 0
    assert d["c5"]["precision"] == "fast" and d["c5"]["parity"]["embedding_max_abs_err"] < 1e-3 and d["c5"]["roofline"]["peak"] == 2500.0
    assert d["bilateral_solver"]["batch1"]["ms_per_image"] > 0 and d["pseudo_labels"]["value"] > 0 and d["batch1"]["parity"]["category_list_identical"]
    # the pseudo-label path is measured like the headline (round 6): roofline of its dominant kernel, parity of the final mask against the
    # oracle chain, a bounded CPU baseline
    pl = d["pseudo_labels"]
    assert pl["roofline"]["bound"] == "mfma" and "attn_f16_kernel" in pl["roofline"]["kernel"] and 0.15 < pl["roofline"]["frac"] < 1.0
    assert abs(pl["roofline"]["frac"] - pl["roofline"]["achieved"] / pl["roofline"]["peak"]) < 1e-3
    assert pl["parity"]["differing_pixels_off_the_oracle_contour"] == 0 and pl["parity"]["differing_pixels"] <= 200
    assert pl["parity"]["selected_query_identical"] is True and pl["cpu_baseline"]["kind"] == "port" and pl["cpu_baseline"]["value"] > 0
    assert pl["value_noise_images"] > 0 and "natural" in pl["images"]
    assert list(d)[-1] == "summary" and len(json.dumps(d["summary"])) < 1500
    s = d["summary"]
    assert s["checked"] is True and s["c4"]["ok"] is True and "c5_fast" in s and "solver_ms" in s and "b1_ms" in s and s["pseudo"]["bad_px"] == 0


def test_plain_run_only_times_and_dumps_the_last_step(dev, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: the contract keys, K timed steps, none of the --full objects; and
    `--dump-outputs DIR` writes the last timed step's label maps and low-res logits as float32 — what one eager step of the engine
    computes on bench.py's rank-0 batch, bit for bit."""
    import numpy as np
    import torch
    from zutis_amd import detgen, ops
    from zutis_amd.engine import ZutisEngine
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
    for k, t in (("metric", str), ("value", (int, float)), ("unit", str), ("higher_is_better", bool), ("dtype", str), ("ms_per_step", (int, float))):
        assert isinstance(d[k], t), (k, d[k])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "images/s" and d["dtype"].startswith("f16x3")
    assert abs(d["value"] - 32 * 1e3 / d["ms_per_step"]) / d["value"] < 0.01
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["timed_outputs_checked"] is None
    assert not {"second_precision", "io_inclusive", "torch_gpu_baseline", "batch1", "c4", "c5"} & set(d)
    assert sorted(p.name for p in out.iterdir()) == ["labels.npy", "logits_lowres.npy"]
    lab, lo = np.load(out / "labels.npy"), np.load(out / "logits_lowres.npy")
    assert lab.dtype == np.float32 and lo.dtype == np.float32 and lab.shape == (32, 336, 336) and lo.shape == (32, 81, 42, 42)
    cfg = detgen.VIT_B16
    P = {k: torch.from_numpy(v).to(dev) for k, v in detgen.zutis_state_dict(cfg).items()}
    text = torch.from_numpy(detgen.text_embeddings(81, cfg.embed_dim)).to(dev)
    x = torch.randn((32, 3, 336, 336), generator=torch.Generator(device="cpu").manual_seed(1000)).to(dev)     # bench.py's rank-0 batch
    eng = ZutisEngine(P, cfg.patch, cfg.dec_heads, precision="exact")
    lo_e = eng.semantic_logits_lowres(eng.forward(x)["patch_tokens"], text)
    lab_e = torch.empty((32, 336, 336), dtype=torch.int64, device=dev)
    ops.upsample_argmax(lo_e, lab_e, 32, 81, lo_e.shape[2], lo_e.shape[3], 336, 336)
    assert np.array_equal(lo, lo_e.cpu().numpy()) and np.array_equal(lab, lab_e.cpu().numpy().astype(np.float32))
