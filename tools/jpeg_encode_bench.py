"""Developer tool: the overlays of predict_from_files as JPEG files (overlay_format="jpeg": the writer threads' Pillow, jpeg_encoder="host",
or zh_jpeg_encode, jpeg_encoder="device"; zutis_amd/jpeg_device.py) against the two PNG encoders, on the corpus of tools/png_encode_bench.py.

    python tools/jpeg_encode_bench.py [--setup semantic|instance ...] [--rounds R] [--images N] [--batch B] [--workers W] [--model vitb16|tiny]
                                      [--quality Q] [--subsampling 4:2:0|4:4:4] [--kernel-only] [--corpus DIR] [--out profiles/jpeg_encode_ab.json]

Set-ups (N = 64 coco-like JPEGs of 640 x 480 / 480 x 640, ViT-B/16, 81 classes):
  semantic  predict_from_files(overlay=True): the label map (mode L PNG) and the semantic overlay per image
  instance  tools/instance_paint_bench.py's F1: predict_from_files(semantic=False, instance=True, instance_map=True, instance_overlay=True) —
            the id map (mode L PNG) and the instance overlay per image
Arms png/host, png/device (overlay_format="png" under the two png_encoder values: the parent's arms, the time reference), jpeg/host and
jpeg/device (png_encoder="host"), ALTERNATED in one process (round r runs all four), one untimed pass per arm first, a device synchronise in
every window; medians and min - max over the rounds, every round kept.  Per arm: images/s, the bytes of an overlay file, the bytes the
batch's copy back carries per image (picture_out.Layout.host_bytes at 480 x 640); for jpeg/device the HIP-event time of zh_jpeg_encode's
three launches together, summed over a run, and the pictures that went through the host arm.  The size reference is Pillow's JPEG of the
png/host arm's overlays at the same settings WITHOUT restart markers.  The two JPEG arms' files are compared byte for byte.
--kernel-only: zh_jpeg_encode alone on overlays of the png arm at 480 x 640, B = 1 and 4, both subsamplings, milliseconds per call between
HIP events (median of 20 after 3 untimed) — also the `rocprofv3 --kernel-trace --stats` target that splits the call into its launches."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "zutis_amd", "dropin"))
from eval_files_bench import MEAN, STD, network_of                                 # noqa: E402
from png_encode_bench import corpus_images, files_bytes, timed                     # noqa: E402
from zutis_amd import jpeg_device, ops, picture_out, predict_files                 # noqa: E402

ARMS = {"png/host": dict(png_encoder="host"), "png/device": dict(png_encoder="device"),
        "jpeg/host": dict(overlay_format="jpeg", jpeg_encoder="host"), "jpeg/device": dict(overlay_format="jpeg", jpeg_encoder="device")}


class Probe:
    """Wraps ops.jpeg_encode in HIP events; read() returns and clears what a run gathered."""

    def __init__(self):
        self.events = []
        real = ops.jpeg_encode

        def encode(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = real(*a, **k)
            e1.record()
            self.events.append((e0, e1))
            return r
        ops.jpeg_encode = encode

    def read(self):
        torch.cuda.synchronize()
        out = {"encode_calls": len(self.events), "encode_ms": round(sum(a.elapsed_time(b) for a, b in self.events), 4)}
        self.events = []
        return out


def copy_back_bytes(kinds, arm, batch):
    """Bytes of the batch's copy back per image at 480 x 640 under the arm's encoders."""
    kw = ARMS[arm]
    lay = picture_out.Layout([(480, 640)] * batch, kinds, kw.get("jpeg_encoder", "host"))
    return lay.host_bytes[kw.get("png_encoder", "host")] // batch


def ab(run, rounds, probe, n_images, overlay_key, args):
    rec = {a: {"seconds_rounds": [], "probe_rounds": [], "fallbacks": 0} for a in ARMS}
    results = {}
    for a in ARMS:
        run(a)
        probe.read()
    for r in range(rounds):
        for a in ARMS:
            s, results[a] = run(a)
            rec[a]["seconds_rounds"].append(round(s, 5))
            rec[a]["probe_rounds"].append(probe.read())
            rec[a]["fallbacks"] = results[a].get("jpeg_host_fallbacks", 0)
            print(f"round {r} {a}: {s:.4f} s = {n_images / s:.1f} images/s", flush=True)
    out = {}
    for a in ARMS:
        s, overlays = rec[a]["seconds_rounds"], results[a][overlay_key]
        out[a] = {"seconds": round(statistics.median(s), 5), "seconds_min": min(s), "seconds_max": max(s), "seconds_rounds": s,
                  "images_per_s": round(n_images / statistics.median(s), 1), "images_per_s_min": round(n_images / max(s), 1),
                  "images_per_s_max": round(n_images / min(s), 1), "overlay_files": len(overlays),
                  "bytes_per_overlay": round(files_bytes(overlays) / len(overlays), 1)}
    d = rec["jpeg/device"]
    out["jpeg/device"].update(encode_ms=round(statistics.median(x["encode_ms"] for x in d["probe_rounds"]), 4), encode_calls=d["probe_rounds"][0]["encode_calls"],
                              jpeg_host_fallbacks=d["fallbacks"])
    plain = 0
    for p in results["png/host"][overlay_key]:                              # the size reference: the same pictures, no restart markers
        buf = io.BytesIO()
        with Image.open(p) as im:
            im.save(buf, "JPEG", quality=args.quality, subsampling=jpeg_device.SUBSAMPLINGS[args.subsampling])
        plain += buf.tell()
    out["pillow_no_restart_bytes_per_overlay"] = round(plain / len(results["png/host"][overlay_key]), 1)
    out["jpeg_files_differing"] = sum(open(a, "rb").read() != open(b, "rb").read()
                                      for a, b in zip(results["jpeg/host"][overlay_key], results["jpeg/device"][overlay_key]))
    for a, b in (("jpeg/device", "png/host"), ("jpeg/device", "png/device"), ("jpeg/device", "jpeg/host"), ("jpeg/host", "png/host")):
        overlap = out[a]["seconds_min"] <= out[b]["seconds_max"] and out[b]["seconds_min"] <= out[a]["seconds_max"]
        out[f"{a} over {b}"] = {"speed": round(out[b]["seconds"] / out[a]["seconds"], 3), "ranges_overlap": bool(overlap),
                                "bytes": round(out[a]["bytes_per_overlay"] / out[b]["bytes_per_overlay"], 4)}
    return out


def kernel_only(overlays, dev):
    """zh_jpeg_encode alone: {subsampling: {B: ms per call}} on overlays of 480 x 640."""
    pics = [np.asarray(Image.open(p).convert("RGB")) for p in overlays]
    pics = [a for a in pics if a.shape[:2] == (480, 640)][:4]
    out = {}
    for name, sub in jpeg_device.SUBSAMPLINGS.items():
        out[name] = {}
        for B in (1, 4):
            batch = torch.from_numpy(np.stack(pics[:B])).to(dev)
            H, W, slot = 480, 640, jpeg_device.scan_slot(480, 640)
            hs = 16 if sub == 2 else 8
            off = torch.arange(B, dtype=torch.int64, device=dev)
            scans, lengths = torch.empty(B * slot, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
            hw, quant = torch.tensor([[H, W]] * B, dtype=torch.int32, device=dev), jpeg_device.quant_tensor(90, dev)
            img_off, out_off, mcus = off * (H * W * 3), off * slot, (H // hs) * (W // hs)
            ms = []
            for it in range(23):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.jpeg_encode(batch, img_off, hw, sub, quant, scans, out_off, slot, lengths, mcus)
                e1.record()
                torch.cuda.synchronize()
                if it >= 3:
                    ms.append(e0.elapsed_time(e1))
            out[name][f"B{B}"] = {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                                  "scan_bytes": [int(v) for v in lengths.cpu().tolist()]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setup", nargs="+", default=["semantic", "instance"], choices=["semantic", "instance"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--model", default="vitb16", choices=["vitb16", "tiny"])
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--subsampling", default="4:2:0", choices=sorted(jpeg_device.SUBSAMPLINGS))
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--corpus", default=os.path.join(tempfile.gettempdir(), "zutis_eval_corpus"))
    ap.add_argument("--out", help="also write the result object to this JSON file")
    args = ap.parse_args()
    workers = max(1, min(args.workers, 16))
    dev = torch.device("cuda:0")
    probe = Probe()
    cfg, d, p_images = corpus_images(args, workers)
    net, _ = network_of(args.model, cfg["n"], dev)
    ids = list(range(args.images))
    rng = np.random.default_rng(3)
    palette = rng.integers(0, 256, (cfg["n"], 3)).astype(np.uint8)
    res = {"tool": "jpeg_encode_bench", "model": args.model, "images": args.images, "batch": args.batch, "n_workers": workers, "rounds": args.rounds,
           "quality": args.quality, "subsampling": args.subsampling, "interval_mcus": jpeg_device.ENC_INTERVAL_MCUS, "pillow": Image.__version__,
           "cpus_in_use": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None, "setups": {}}
    common = dict(max_size=cfg["max_size"], mean=MEAN, std=STD, batch_size=args.batch, n_workers=workers, jpeg_quality=args.quality,
                  jpeg_subsampling=args.subsampling)

    def run_semantic(arm):
        return timed(lambda: predict_files.predict_from_files(net, p_images, out_dir=os.path.join(d, "jpeg_s_" + arm.replace("/", "_")), label_format=cfg["fmt"],
                                                              palette=palette, overlay=True, **common, **ARMS[arm]))

    def run_instance(arm):
        return timed(lambda: predict_files.predict_from_files(net, p_images, out_dir=os.path.join(d, "jpeg_i_" + arm.replace("/", "_")), semantic=False, instance=True,
                                                              image_ids=ids, instance_map=True, instance_overlay=True, **common, **ARMS[arm]))
    if args.kernel_only:
        _, r = run_instance("png/host")
        res["kernel_only"] = kernel_only(r["instance_overlay_paths"], dev)
    else:
        for name, run, key, kinds in (("semantic", run_semantic, "overlay_paths", [(1, "P", None)]), ("instance", run_instance, "instance_overlay_paths", [(1, "L", None)])):
            if name in args.setup:
                res["setups"][name] = ab(run, args.rounds, probe, args.images, key, args)
                for arm in ARMS:
                    overlay = (3, "JPEG", None) if arm.startswith("jpeg") else (3, "RGB", None)
                    res["setups"][name][arm]["copy_back_bytes_per_image"] = copy_back_bytes(kinds + [overlay], arm, args.batch)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
