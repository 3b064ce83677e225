"""Developer tool: the device JPEG decoder (decoder="device": zh_jpeg_decode) against the decoding threads' Pillow (decoder="host", the
default and the parent's own path) on the two drivers that start from image files, in one process.

    python tools/jpeg_decode_bench.py [--setup extract|predict ...] [--rounds R] [--images N] [--predict-images M] [--workers W]
                                      [--layers L] [--kernel-only] [--out FILE.json]

Set-ups, per set-up the arms ALTERNATED (round r runs every arm once), medians and every round; an arm is "ahead" only when its slowest
round is above the other's fastest:
  extract  extract_bench.py's corpus (2048 seeded JPEGs, ViT-L/14@336, B = 256, `fast`): extract_image_embeddings with decoder="host" and
           "device", the embeddings compared for equality, beside `encode_image` on a resident batch (E, the ceiling)
  predict  predict_files_bench.py's coco-like corpus (64 files, 640x480 / 480x640, 81 classes, B = 4, semantic label PNGs):
           predict_from_files with decoder="host" and "device", the written files compared byte for byte
Per arm: images/s and the bytes copied host-to-device per image (the staging buffers' sizes, summed over the loader's batches).
--kernel-only: nothing but zh_jpeg_decode on one batch of each set-up (B = 256 of the extraction corpus, B = 4 of the prediction
corpus), 5 launches each — the form to put behind `rocprofv3 --kernel-trace --stats --` for the time per launch of each stage."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "zutis_amd", "dropin"))
from eval_files_bench import CONFIGS, MEAN, STD, network_of, write_pair          # noqa: E402
from extract_corpus import corpus, tower                                        # noqa: E402
from utils import extract_image_embeddings as DROPIN                            # noqa: E402
from zutis_amd import jpeg_device, ops, predict_files, preprocess               # noqa: E402
from zutis_amd.engine import ClipImageEncoder                                   # noqa: E402

ARMS = ("host", "device")


def h2d_bytes(loader):
    """Bytes of the staging buffers of every batch of `loader` (what device_batches copies host-to-device), and the files the host decoded."""
    total = n_host = 0
    for b in loader:
        total += b.staging.numel()
        n_host += len(b.paths) if b.jpeg is None else b.n_host_decoded
    return total, n_host


def summarise(secs, n):
    out = {}
    for a, v in secs.items():
        med = statistics.median(v)
        out[a] = {"images_per_s": round(n / med, 1), "seconds_rounds": [round(x, 3) for x in v], "images_per_s_min": round(n / max(v), 1),
                  "images_per_s_max": round(n / min(v), 1)}
    if all(a in secs for a in ARMS):
        out["device_over_host"] = round(out["device"]["images_per_s"] / out["host"]["images_per_s"], 3)
        out["ahead"] = "device" if max(secs["device"]) < min(secs["host"]) else "host" if max(secs["host"]) < min(secs["device"]) else "neither"
    return out


def predict_corpus(directory, n, workers):
    cfg = CONFIGS["coco"]
    d = os.path.join(directory, "coco")
    os.makedirs(d, exist_ok=True)
    p_images = [os.path.join(d, f"img_{k:05d}.jpg") for k in range(n)]
    p_gts = [os.path.join(d, f"gt_{k:05d}.png") for k in range(n)]
    todo = [k for k in range(n) if not (os.path.exists(p_images[k]) and os.path.exists(p_gts[k]))]
    with ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(lambda k: write_pair(cfg, k, p_images[k], p_gts[k]), todo))
    return cfg, d, p_images


def kernel_only(dev, paths, B, launches=5):
    """zh_jpeg_decode alone on the first B files of `paths`."""
    datas = [open(p, "rb").read() for p in paths[:B]]
    plans = [jpeg_device.parse(d) for d in datas]
    packed = jpeg_device.pack(plans, datas, skip_overflow=True)
    up = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    scan, segments, images, tables = up(packed.scan), up(packed.segments), up(packed.images), up(packed.tables)
    out = torch.empty(packed.out_bytes, dtype=torch.uint8, device=dev)
    status = torch.empty(len(packed.kept), dtype=torch.int32, device=dev)
    for _ in range(launches):
        ops.jpeg_decode(scan, segments, images, tables, packed.n_blocks, packed.max_image_blocks, packed.max_image_pixels, out, status)
    torch.cuda.synchronize()
    assert not bool(status.any())
    return {"B": len(packed.kept), "segments": int(len(packed.segments)), "scan_bytes": int(packed.scan.size), "blocks": int(packed.n_blocks),
            "table_sets": int(packed.tables.shape[0]), "launches": launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setup", action="append", choices=["extract", "predict"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--predict-images", type=int, default=64)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--extract-corpus", default=os.path.join(tempfile.gettempdir(), "zutis_extract_corpus"))
    ap.add_argument("--predict-corpus", default=os.path.join(tempfile.gettempdir(), "zutis_eval_corpus"))
    ap.add_argument("--out", help="also write the result object to this JSON file")
    args = ap.parse_args()
    setups = list(dict.fromkeys(args.setup or ["extract", "predict"]))
    workers = max(1, min(args.workers, 16))
    dev = torch.device("cuda:0")
    res = {"tool": "jpeg_decode_bench", "rounds": args.rounds, "n_workers": workers, "pillow": Image.__version__,
           "cpus_in_use": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None, "setups": {}}
    if "extract" in setups:
        paths = corpus(args.extract_corpus, args.images, workers)
        if args.kernel_only:
            res["setups"]["extract"] = kernel_only(dev, paths, 256)
        else:
            sd, patch = tower(dev, args.layers)
            n_px, B = 336, 256

            def call(decoder, some):
                torch.cuda.synchronize(); t = time.perf_counter()
                out = DROPIN.extract_image_embeddings(some, model_name="ViT-L/14@336px", device=dev, batch_size=B, n_workers=workers, state_dict=sd,
                                                      precision="fast", decoder=decoder)
                torch.cuda.synchronize()
                return time.perf_counter() - t, out

            enc = ClipImageEncoder(sd, patch, prefix="visual.", precision="fast")
            resident = torch.randn((B, 3, n_px, n_px), generator=torch.Generator(device="cpu").manual_seed(2000)).to(dev)
            enc.encode_image(resident)

            def ceiling():
                steps = (len(paths) + B - 1) // B
                torch.cuda.synchronize(); t = time.perf_counter()
                for _ in range(steps):
                    enc.encode_image(resident)
                torch.cuda.synchronize()
                return (time.perf_counter() - t) * len(paths) / (steps * B)

            for a in ARMS:
                call(a, paths[:B])                                        # warm-up
            secs, outs = {a: [] for a in ARMS + ("E",)}, {}
            for r in range(args.rounds):
                for a in ARMS:
                    dt, outs[a] = call(a, paths)
                    secs[a].append(dt)
                    print(f"extract round {r} {a}: {dt:.3f} s = {len(paths) / dt:.1f} images/s", flush=True)
                secs["E"].append(ceiling())
            e = summarise(secs, len(paths))
            e["equal"] = bool(list(outs["host"]) == list(outs["device"]) and all(torch.equal(outs["host"][k], outs["device"][k]) for k in outs["host"]))
            for a in ARMS:
                total, n_host = h2d_bytes(preprocess.BatchLoader(paths, n_px, B, workers, DROPIN.resize_crop_box, pin=False, decoder=a))
                e[a]["h2d_bytes_per_image"] = round(total / len(paths), 1)
                e[a]["host_decoded"] = n_host
            e["file_bytes_per_image"] = round(sum(os.path.getsize(p) for p in paths) / len(paths), 1)
            res["setups"]["extract"] = e
    if "predict" in setups:
        cfg, d, p_images = predict_corpus(args.predict_corpus, args.predict_images, workers)
        if args.kernel_only:
            res["setups"]["predict"] = kernel_only(dev, p_images, 4)
        else:
            net, _ = network_of("vitb16", cfg["n"], dev)
            outs = {a: [os.path.join(d, f"pred_jpeg_{a}", os.path.basename(p)[:-4] + ".png") for p in p_images] for a in ARMS}

            def call(decoder):
                torch.cuda.synchronize(); t = time.perf_counter()
                predict_files.predict_from_files(net, p_images, out_paths=outs[decoder], label_format=cfg["fmt"], max_size=cfg["max_size"], mean=MEAN,
                                                 std=STD, batch_size=4, n_workers=workers, decoder=decoder)
                torch.cuda.synchronize()
                return time.perf_counter() - t

            for a in ARMS:
                call(a)                                                   # warm-up (graph captures, allocator, page cache)
            secs = {a: [] for a in ARMS}
            for r in range(args.rounds):
                for a in ARMS:
                    secs[a].append(call(a))
                    print(f"predict round {r} {a}: {secs[a][-1]:.3f} s = {len(p_images) / secs[a][-1]:.1f} images/s", flush=True)
            e = summarise(secs, len(p_images))
            e["equal"] = all(open(x, "rb").read() == open(y, "rb").read() for x, y in zip(outs["host"], outs["device"]))
            for a in ARMS:
                total, n_host = h2d_bytes(preprocess.PredictBatchLoader(p_images, cfg["max_size"], 4, workers, pin=False, decoder=a))
                e[a]["h2d_bytes_per_image"] = round(total / len(p_images), 1)
                e[a]["host_decoded"] = n_host
            e["file_bytes_per_image"] = round(sum(os.path.getsize(p) for p in p_images) / len(p_images), 1)
            res["setups"]["predict"] = e
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
