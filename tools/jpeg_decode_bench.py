"""Developer tool: the device JPEG decoders (decoder="device": zh_jpeg_decode, one lane per entropy segment; decoder="device-split":
zh_jpeg_decode_split, every segment split among lanes) against the decoding threads' Pillow (decoder="host", the default) on the two
drivers that start from image files, in one process.

    python tools/jpeg_decode_bench.py [--setup extract|predict ...] [--rounds R] [--images N] [--predict-images M] [--workers W]
                                      [--layers L] [--kernel-only] [--chunk-bytes N ...] [--passes P ...] [--out FILE.json]

Set-ups, per set-up the arms ALTERNATED (round r runs every arm once), medians and every round; an arm is "ahead" only when its slowest
round is above the other's fastest:
  extract  extract_bench.py's corpus (2048 seeded JPEGs, ViT-L/14@336, B = 256, `fast`): extract_image_embeddings with every decoder,
           the embeddings compared for equality with the host's, beside `encode_image` on a resident batch (E, the ceiling)
  predict  predict_files_bench.py's coco-like corpus (64 files, 640x480 / 480x640, 81 classes, B = 4, semantic label PNGs):
           predict_from_files with every decoder, the written files compared byte for byte with the host's
Per arm: images/s and the bytes copied host-to-device per image (the staging buffers' sizes, summed over the loader's batches); for
"device-split" also the images of the whole corpus that came back UNSYNCED at the shipped constants (they are decoded by the host).
--kernel-only: nothing but the decoders on one batch of each set-up (B = 256 of the extraction corpus, B = 4 of the prediction corpus),
alternated, `--rounds` launches each between HIP events: Pillow in the worker threads ("host"), zh_jpeg_decode ("device") and
zh_jpeg_decode_split at every --chunk-bytes x --passes asked for (default: the shipped constants), with the images left UNSYNCED; the
outputs of the device arms are compared for equality.  Also the form to put behind `rocprofv3 --kernel-trace --stats --`."""
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

ARMS = ("host", "device", "device-split")


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
    ahead = lambda a, b: a if max(secs[a]) < min(secs[b]) else b if max(secs[b]) < min(secs[a]) else "neither"      # noqa: E731
    if all(a in secs for a in ARMS):
        out["device_over_host"] = round(out["device"]["images_per_s"] / out["host"]["images_per_s"], 3)
        out["ahead"] = ahead("device", "host")
        out["split_over_device"] = round(out["device-split"]["images_per_s"] / out["device"]["images_per_s"], 3)
        out["split_over_host"] = round(out["device-split"]["images_per_s"] / out["host"]["images_per_s"], 3)
        out["ahead_split_device"] = ahead("device-split", "device")
        out["ahead_split_host"] = ahead("device-split", "host")
        out["split_ahead_of_device_in_every_round"] = all(s < d for s, d in zip(secs["device-split"], secs["device"]))
    return out


def unsynced_share(paths, B):
    """(images served, images UNSYNCED) of zh_jpeg_decode_split's host twin at the shipped constants over `paths` in batches of B."""
    served = unsynced = 0
    for k in range(0, len(paths), B):
        datas = [open(p, "rb").read() for p in paths[k:k + B]]
        plans = [jpeg_device.parse(d) for d in datas]
        keep = [i for i, p in enumerate(plans) if p is not None]
        packed = jpeg_device.pack([plans[i] for i in keep], [datas[i] for i in keep], skip_overflow=True, chunk_bytes=jpeg_device.CHUNK_BYTES)
        _, status = jpeg_device.decode_split_host(packed)
        served += len(status)
        unsynced += int(((status & jpeg_device.STATUS["unsynced"]) != 0).sum())
    return served, unsynced


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


def kernel_only(dev, paths, B, launches, workers, chunk_sizes, pass_counts):
    """The three decoders alone on the first B files of `paths`, alternated: milliseconds per batch of every launch."""
    datas = [open(p, "rb").read() for p in paths[:B]]
    plans = [jpeg_device.parse(d) for d in datas]
    packed = jpeg_device.pack(plans, datas, skip_overflow=True)
    up = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    scan, segments, images, tables = up(packed.scan), up(packed.segments), up(packed.images), up(packed.tables)
    outs = {}
    status = torch.empty(len(packed.kept), dtype=torch.int32, device=dev)

    def out_of(arm):
        if arm not in outs:
            outs[arm] = torch.zeros(packed.out_bytes, dtype=torch.uint8, device=dev)
        return outs[arm]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    arms = {"device": lambda: ops.jpeg_decode(scan, segments, images, tables, packed.n_blocks, packed.max_image_blocks, packed.max_image_pixels,
                                              out_of("device"), status)}
    chunks = {cb: up(jpeg_device.chunk_rows(packed, cb)) for cb in chunk_sizes}
    for cb in chunk_sizes:
        for ps in pass_counts:
            arms[f"device-split-{cb}-{ps}"] = lambda cb=cb, ps=ps: ops.jpeg_decode_split(
                scan, segments, chunks[cb], images, tables, packed.n_blocks, packed.max_image_blocks, packed.max_image_pixels,
                out_of(f"device-split-{cb}-{ps}"), status, chunk_bytes=cb, passes=ps)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        def host():
            list(pool.map(lambda p: Image.open(p).convert("RGB").load(), paths[:B]))
        ms, unsynced = {a: [] for a in ("host",) + tuple(arms)}, {}
        for a, fn in arms.items():
            fn()                                                      # warm-up
        torch.cuda.synchronize()
        for _ in range(launches):
            t = time.perf_counter(); host(); ms["host"].append(1e3 * (time.perf_counter() - t))
            for a, fn in arms.items():
                ms[a].append(timed(fn))
                st = status.cpu().numpy()
                if a == "device":
                    assert not st.any()
                else:
                    assert ((st == 0) | ((st & jpeg_device.STATUS["unsynced"]) != 0)).all()      # (an UNSYNCED image may carry error bits too)
                    unsynced[a] = int((st != 0).sum())
    equal = {a: bool(torch.equal(outs[a], outs["device"])) for a in arms if a != "device" and unsynced[a] == 0}
    return {"B": len(packed.kept), "segments": int(len(packed.segments)), "scan_bytes": int(packed.scan.size), "blocks": int(packed.n_blocks),
            "table_sets": int(packed.tables.shape[0]), "launches": launches, "chunks": {str(cb): int(chunks[cb].shape[0]) for cb in chunk_sizes},
            "ms_per_batch_median": {a: round(statistics.median(v), 4) for a, v in ms.items()}, "ms_per_batch_rounds": {a: [round(x, 4) for x in v] for a, v in ms.items()},
            "unsynced_images": unsynced, "equal_to_device": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setup", action="append", choices=["extract", "predict"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--predict-images", type=int, default=64)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--chunk-bytes", type=int, nargs="+", default=[jpeg_device.CHUNK_BYTES], help="--kernel-only: the chunk sizes of the split arm")
    ap.add_argument("--passes", type=int, nargs="+", default=[jpeg_device.SPLIT_PASSES], help="--kernel-only: its synchronising passes")
    ap.add_argument("--extract-corpus", default=os.path.join(tempfile.gettempdir(), "zutis_extract_corpus"))
    ap.add_argument("--predict-corpus", default=os.path.join(tempfile.gettempdir(), "zutis_eval_corpus"))
    ap.add_argument("--out", help="also write the result object to this JSON file")
    args = ap.parse_args()
    setups = list(dict.fromkeys(args.setup or ["extract", "predict"]))
    workers = max(1, min(args.workers, 16))
    dev = torch.device("cuda:0")
    res = {"tool": "jpeg_decode_bench", "rounds": args.rounds, "chunk_bytes": jpeg_device.CHUNK_BYTES, "passes": jpeg_device.SPLIT_PASSES, "n_workers": workers, "pillow": Image.__version__,
           "cpus_in_use": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None, "setups": {}}
    if "extract" in setups:
        paths = corpus(args.extract_corpus, args.images, workers)
        if args.kernel_only:
            res["setups"]["extract"] = kernel_only(dev, paths, 256, args.rounds, workers, args.chunk_bytes, args.passes)
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
            e["equal"] = bool(all(list(outs["host"]) == list(outs[a]) and all(torch.equal(outs["host"][k], outs[a][k]) for k in outs["host"]) for a in ARMS[1:]))
            e["device-split"]["served"], e["device-split"]["unsynced"] = unsynced_share(paths, B)
            for a in ARMS:
                total, n_host = h2d_bytes(preprocess.BatchLoader(paths, n_px, B, workers, DROPIN.resize_crop_box, pin=False, decoder=a))
                e[a]["h2d_bytes_per_image"] = round(total / len(paths), 1)
                e[a]["host_decoded"] = n_host
            e["file_bytes_per_image"] = round(sum(os.path.getsize(p) for p in paths) / len(paths), 1)
            res["setups"]["extract"] = e
    if "predict" in setups:
        cfg, d, p_images = predict_corpus(args.predict_corpus, args.predict_images, workers)
        if args.kernel_only:
            res["setups"]["predict"] = kernel_only(dev, p_images, 4, args.rounds, workers, args.chunk_bytes, args.passes)
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
            e["equal"] = all(open(x, "rb").read() == open(y, "rb").read() for a in ARMS[1:] for x, y in zip(outs["host"], outs[a]))
            e["device-split"]["served"], e["device-split"]["unsynced"] = unsynced_share(p_images, 4)
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
