"""Cases of the device PNG encoder shared by tests/test_png_device_cpu.py and tests/test_png_device_gpu.py: filtered-byte sequences at the
token edges of zutis_amd/png_device.py, an independent statement of the stream's length, and small images.  Plain helper module."""
import numpy as np

from zutis_amd import png_device as P

S = P.SEGMENT_BYTES
RUN_LENGTHS = (1, 2, 3, 4, 5, 6, 7, 258, 259, 260, 261, 262, 517, 518, 519, 520)


def runs_bytes(lengths, values=None) -> np.ndarray:
    """Runs of the given lengths back to back; neighbouring runs differ (values cycle through bytes below and above 144)."""
    values = values or [5, 200, 143, 144, 0, 255]
    return np.concatenate([np.full(n, values[i % len(values)], np.uint8) for i, n in enumerate(lengths)])


def no_run_bytes(n: int, low: int, seed: int = 0) -> np.ndarray:
    """n bytes in low .. 255 without two equal neighbours."""
    rng = np.random.default_rng(seed)
    d = rng.integers(low, 256, n).astype(np.int64)
    for i in range(1, n):
        if d[i] == d[i - 1]:
            d[i] = low + (d[i] - low + 1) % (256 - low)
    return d.astype(np.uint8)


def edge_sequences() -> dict:
    """name -> filtered bytes u8 [n]."""
    seqs = {f"run{n}": runs_bytes([1, n, 1]) for n in RUN_LENGTHS}
    seqs["runs_all"] = runs_bytes(list(RUN_LENGTHS))
    seqs["literals"] = np.arange(256, dtype=np.uint8)
    seqs["cross"] = runs_bytes([S - 100, 300, 7])                      # a run over the segment boundary: clipped to 100 + 200
    seqs["cross_short"] = runs_bytes([S - 2, 4, 1])                    # clipped to 2 + 2: literals on both sides
    seqs["n_seg"] = no_run_bytes(S, 0, 1)
    seqs["n_seg_minus"] = no_run_bytes(S - 1, 0, 2)
    seqs["n_seg_plus"] = no_run_bytes(S + 1, 0, 3)
    seqs["one_long_run"] = np.full(2 * S + 11, 9, np.uint8)
    seqs["worst"] = no_run_bytes(S + 40, 144, 4)
    return seqs


_LEN_EXTRA_BITS = [(3, 0), (11, 1), (19, 2), (35, 3), (67, 4), (131, 5), (258, 0)]     # RFC 1951 3.2.5: first length of each extra-bit class


def _match_bits(length: int) -> int:
    extra = [e for first, e in _LEN_EXTRA_BITS if first <= length][-1]
    return (8 if length >= 115 else 7) + extra + 5                       # symbols 280 .. 287 (lengths 115 ..) have 8-bit codes


def stream_length(data: np.ndarray) -> int:
    """The stream's length from the greedy rule, run by run in a Python loop (not the closed form of png_device.run_tokens)."""
    d = np.asarray(data, np.uint8)
    total = 2 + 6
    for at in range(0, d.size, S):
        seg = d[at:at + S].tolist()
        bits, i = 3 + 7 + 3, 0
        while i < len(seg):
            j = i
            while j < len(seg) and seg[j] == seg[i]:
                j += 1
            lit = 8 if seg[i] < 144 else 9
            left = j - i - 1
            bits += lit
            while left >= 3:
                take = min(258, left)
                bits += _match_bits(take)
                left -= take
            bits += left * lit
            i = j
        total += (bits + 7) // 8 + 4
    return total


def blocky(h: int, w: int, seed: int = 0, labels: int = 21, cell: int = 16) -> np.ndarray:
    """A label-map-like u8 [h, w]: constant cells."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, labels, (-(-h // cell), -(-w // cell))).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(small, cell, 0), cell, 1)[:h, :w])


def images(c: int) -> list:
    """Small u8 images [h, w] (c = 1) or [h, w, 3] (c = 3): the edge sequences as one-row images (the first row is filtered against
    zeros, so the filtered bytes are 2 followed by the row), and pictures just past one and two segments."""
    rng = np.random.default_rng(7 + c)
    out = []
    for d in edge_sequences().values():
        d = d[:d.size // c * c]
        out.append(d.reshape(1, -1) if c == 1 else d.reshape(1, -1, 3))
    shape = lambda h, w: (h, w) if c == 1 else (h, w, 3)                  # noqa: E731
    h1, h2 = (41, 83) if c == 1 else (14, 28)                             # 401 columns: 16482 / 33366 and 16856 / 33712 filtered bytes
    lab = blocky(h2, 401, 1)
    out.append(lab[:h1] if c == 1 else np.stack([lab[:h1], lab[:h1] // 3, np.zeros_like(lab[:h1])], -1))
    out.append(lab if c == 1 else np.stack([lab, lab // 3, np.zeros_like(lab)], -1))
    out.append(rng.integers(0, 256, shape(h1, 401)).astype(np.uint8))                   # per-pixel noise
    out.append(np.full(shape(h2, 401), 77, np.uint8))                                     # constant
    out.append(np.full(shape(1, 1), 200, np.uint8))
    out.append(rng.integers(0, 3, shape(1, 300)).astype(np.uint8))
    out.append((rng.integers(0, 2, shape(37, 129)) * 255).astype(np.uint8))
    return [np.ascontiguousarray(a) for a in out]
