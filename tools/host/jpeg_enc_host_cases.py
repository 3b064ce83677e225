"""Writes the inputs of tools/host/jpeg_enc_host_check.cpp into a directory: one file per call of zh_jpeg_encode_host.

    python tools/host/jpeg_enc_host_cases.py DIR

The calls are those of tests/test_jpeg_encode_cpu.py and tests/test_jpeg_encode_gpu.py: every picture of tests/_jpeg_enc_case.py at one
quality per case and both subsamplings, in one launch of mixed sizes (`q<quality>_<444|420>`); the picture whose scan is longer than its
slot between two small ones, `out` being exactly three slots (`overflow`); a launch whose second image does not fit — too few MCUs in
max_mcus, a slot that ends one byte behind `out`, pixels that end one byte behind `images` (`refuse_grid`, `refuse_out`,
`refuse_images`).  A case file is little-endian: "ZHE1", int64 x 6 (image bytes, B, subsampling, max_mcus, out bytes, slot bytes), then
images u8, img_off int64 [B], hw int32 [B, 2], quant u16 [2, 64], out_off int64 [B], the expected lengths int32 [B] and the expected
output u8 [out bytes] (jpeg_device.scan_np cut at the slot, 0xA5 everywhere else).  CPU only."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import _jpeg_enc_case as E   # noqa: E402
from zutis_amd import jpeg_device as J  # noqa: E402

FILL = 0xA5


def write_case(path, images, quality, subsampling, slot_bytes=None, image_bytes=None, out_bytes=None, max_mcus=None, img_off=None, refused=()):
    pixels, off, hw, out_off, slot, mcus = J.pack_pictures(images, slot_bytes)
    img_off = off if img_off is None else np.asarray(img_off, np.int64)
    image_bytes = pixels.size if image_bytes is None else image_bytes
    out_bytes = len(images) * slot if out_bytes is None else out_bytes
    want, lengths = np.full(out_bytes, FILL, np.uint8), np.zeros(len(images), np.int32)
    for b, a in enumerate(images):
        if b in refused:
            lengths[b] = -1
            continue
        scan = np.frombuffer(J.scan_np(a, quality, subsampling), np.uint8)
        lengths[b] = scan.size
        n = min(scan.size, slot)
        want[int(out_off[b]):int(out_off[b]) + n] = scan[:n]
    with open(path, "wb") as f:
        f.write(b"ZHE1" + struct.pack("<6q", image_bytes, len(images), J.SUBSAMPLINGS[subsampling], mcus if max_mcus is None else max_mcus, out_bytes, slot))
        for a in (pixels[:image_bytes], img_off, hw, J.quant_tables(quality).astype(np.uint16), out_off, lengths, want):
            f.write(np.ascontiguousarray(a).tobytes())


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    n = 0
    for q in E.QUALITIES:
        for s in E.SUBSAMPLINGS:
            write_case(os.path.join(out_dir, f"q{q}_{s.replace(':', '')}.zhe"), [a for _, a, _ in E.cases(q, s)], q, s)
            n += 1
    big, _ = E.overflow()
    small, _ = E.named(100, "4:4:4", "9x5-smooth")
    write_case(os.path.join(out_dir, "overflow.zhe"), [small, big, small], 100, "4:4:4", slot_bytes=J.scan_slot(64, 64))
    pixels, off, _, _, slot, mcus = J.pack_pictures([small, big])
    write_case(os.path.join(out_dir, "refuse_grid.zhe"), [small, big], 90, "4:4:4", max_mcus=mcus - 1, refused=(1,))
    write_case(os.path.join(out_dir, "refuse_out.zhe"), [small, big], 90, "4:4:4", out_bytes=2 * slot - 1, refused=(1,))
    write_case(os.path.join(out_dir, "refuse_images.zhe"), [small, big], 90, "4:4:4", image_bytes=pixels.size - 1, refused=(1,))
    print(f"{n + 4} cases in {out_dir}")


if __name__ == "__main__":
    main(sys.argv[1])
