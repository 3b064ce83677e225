"""Writes the inputs of tools/host/jpeg_host_check.cpp into a directory: one file per launch of zh_jpeg_decode_host.

    python tools/host/jpeg_host_cases.py DIR

The launches are those of tests/test_jpeg_device_cpu.py and tests/test_jpeg_device_gpu.py: each damaged scan of tests/_jpeg_case.py
(a scan cut at a third, FF 00 repeated, a stray FF C4, all-zero bytes, a DRI that disagrees with the markers) between two good files,
and the two good files alone.  A case file is little-endian: "ZHJ1", int64 x 6 (scan bytes, segments, images, table sets, blocks,
output bytes), then scan u8, segments int32 [S, 4], images int32 [B, 12], tables u8 [n_sets, 3904], damaged int32 [B] (1: a non-zero
status is expected, the pixels are not compared) and the expected output u8 (jpeg_device.decode_np of the good files at their offsets,
0xA5 everywhere else).  CPU only."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import _jpeg_case as C      # noqa: E402
from zutis_amd import jpeg_device as J  # noqa: E402

FILL = 0xA5


def write_case(path, plans, datas, damaged):
    packed = J.pack(plans, datas)
    want = np.full(packed.out_bytes, FILL, np.uint8)
    for b, (plan, data) in enumerate(zip(plans, datas)):
        if not damaged[b]:
            a = J.decode_np(data, plan)
            want[int(packed.out_off[b]):int(packed.out_off[b]) + a.size] = a.reshape(-1)
    with open(path, "wb") as f:
        f.write(b"ZHJ1" + struct.pack("<6q", packed.scan.size, len(packed.segments), len(plans), len(packed.tables), packed.n_blocks, packed.out_bytes))
        for a in (packed.scan, packed.segments, packed.images, packed.tables, np.asarray(damaged, np.int32), want):
            f.write(np.ascontiguousarray(a).tobytes())


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    good = [C.file_bytes(16, 16, "q90-444", "noise"), C.file_bytes(33, 64, "q90-rst", "smooth")]
    plans = [J.parse(d) for d in good]
    write_case(os.path.join(out_dir, "good.zhj"), plans, good, [0, 0])
    for kind in C.DAMAGED:
        plan, data = C.damaged(kind)
        write_case(os.path.join(out_dir, f"{kind}.zhj"), [plans[0], plan, plans[1]], [good[0], data, good[1]], [0, 1, 0])
    print(f"{1 + len(C.DAMAGED)} cases in {out_dir}")


if __name__ == "__main__":
    main(sys.argv[1])
