"""Writes the inputs of tools/host/jpeg_host_check.cpp into a directory: one file per launch of zh_jpeg_decode_host and
zh_jpeg_decode_split_host (the program runs both on every case).

    python tools/host/jpeg_host_cases.py DIR

The launches are those of tests/test_jpeg_device_cpu.py and tests/test_jpeg_device_gpu.py: each damaged scan of tests/_jpeg_case.py
(a scan cut at a third, FF 00 repeated, a stray FF C4, all-zero bytes, a DRI that disagrees with the markers) between two good files,
and the two good files alone — each at 16-byte chunks and as many passes as the launch has sequences, and (`<name>_d`) at the shipped
chunk size and pass count; the split cases of tests/test_jpeg_split_cpu.py: a two-sequence file with ONE pass (`one_pass`: UNSYNCED) and
chunk rows that lie (`lie_*`: an offset, a segment, an unstuffed count, a cleared first flag).  A case file is little-endian: "ZHJ2",
int64 x 9 (scan bytes, segments, images, table sets, blocks, output bytes, chunks, chunk bytes, passes), then scan u8, segments int32
[S, 4], images int32 [B, 12], tables u8 [n_sets, 3904], chunks int32 [C, 4], damaged int32 [B] (bit 0: zh_jpeg_decode_host is expected
to give a non-zero status, bit 1: zh_jpeg_decode_split_host is; such an image's pixels are not compared) and the expected output u8
(jpeg_device.decode_np of the good files at their offsets, 0xA5 everywhere else).  CPU only."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import _jpeg_case as C      # noqa: E402
from zutis_amd import jpeg_device as J  # noqa: E402

FILL = 0xA5


def write_case(path, plans, datas, damaged, chunk_bytes=16, passes=None, lie=None):
    packed = J.pack(plans, datas, chunk_bytes=chunk_bytes)
    chunks = packed.chunks.copy()
    if lie is not None:
        lie(packed, chunks)
    want = np.full(packed.out_bytes, FILL, np.uint8)
    for b, (plan, data) in enumerate(zip(plans, datas)):
        if not damaged[b]:
            a = J.decode_np(data, plan)
            want[int(packed.out_off[b]):int(packed.out_off[b]) + a.size] = a.reshape(-1)
    with open(path, "wb") as f:
        f.write(b"ZHJ2" + struct.pack("<9q", packed.scan.size, len(packed.segments), len(plans), len(packed.tables), packed.n_blocks, packed.out_bytes,
                                      len(chunks), chunk_bytes, J.sequences(packed) if passes is None else passes))
        for a in (packed.scan, packed.segments, packed.images, packed.tables, chunks, np.asarray(damaged, np.int32), want):
            f.write(np.ascontiguousarray(a).tobytes())


def _row_of_image(packed, chunks, b, k):
    """The k-th chunk row of image b."""
    return int(np.flatnonzero(packed.segments[chunks[:, 0], 0] == b)[k])


def _lie(col, delta=None, value=None, k=3):
    def apply(packed, chunks):
        i = _row_of_image(packed, chunks, 1, k)
        chunks[i, col] = value if delta is None else chunks[i, col] + delta
    return apply


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    good = [C.file_bytes(16, 16, "q90-444", "noise"), C.file_bytes(33, 64, "q90-rst", "smooth")]
    plans = [J.parse(d) for d in good]
    n = 0
    for tag, kw in (("", {}), ("_d", dict(chunk_bytes=J.CHUNK_BYTES, passes=J.SPLIT_PASSES))):
        write_case(os.path.join(out_dir, f"good{tag}.zhj"), plans, good, [0, 0], **kw)
        for kind in C.DAMAGED:
            plan, data = C.damaged(kind)
            write_case(os.path.join(out_dir, f"{kind}{tag}.zhj"), [plans[0], plan, plans[1]], [good[0], data, good[1]], [0, 3, 0], **kw)
        n += 1 + len(C.DAMAGED)
    long = C.file_bytes(64, 48, "q90-444", "noise")                    # two sequences at 16-byte chunks
    three = ([plans[0], J.parse(long), plans[1]], [good[0], long, good[1]])
    write_case(os.path.join(out_dir, "one_pass.zhj"), *three, [0, 2, 0], passes=1)
    lies = {"lie_offset": _lie(1, delta=1), "lie_segment": _lie(0, value=1 << 20), "lie_unstuffed": _lie(2, delta=8), "lie_first": _lie(3, value=0, k=0)}
    for name, lie in lies.items():
        write_case(os.path.join(out_dir, f"{name}.zhj"), *three, [0, 2, 0], lie=lie)
    print(f"{n + 1 + len(lies)} cases in {out_dir}")


if __name__ == "__main__":
    main(sys.argv[1])
