"""Shared inputs of the COCO RLE tests (tests/test_rle.py on the CPU, tests/test_rle_codec_gpu.py on the device): masks built from
run lengths, and the value list the stand-alone sanitizer program tools/host/rle_host_check.cpp walks too."""
import numpy as np

# the worked examples of test_rle.test_rle_hand_derived_format_vectors' docstring: value -> characters
WORKED = [(9, b"9"), (40, b"X1"), (-1, b"O"), (1000, b"Xo0"), (-997, b"kPO"), (1995, b"[n1"), (31, b"o0"), (16, b"`0"), (0, b"0")]
# the magnitudes on both sides of every character-count boundary that a mask of fewer than 2^31 pixels reaches (csrc/rle_codec.h)
EDGES = [0, 15, 16, 31, 32, (1 << 24) - 1, 1 << 24, (1 << 31) - 1]
RUN_LENGTHS = (1, 9, 16, 31, 40, 1000)


def mask_from_runs(size, runs):
    """The mask [h, w] whose column-major runs, the run of zeros first, are `runs`."""
    h, w = size
    flat = np.zeros(h * w, np.uint8)
    pos, val = 0, 0
    for r in runs:
        flat[pos:pos + r] = val
        pos += r
        val ^= 1
    assert pos == h * w
    return flat.reshape((h, w), order="F")


def count_lists():
    """Run-count lists for zh_rle_counts_to_string_host: every worked and edge value as a plain count, as the positive delta
    counts[3] - counts[1] and as the negative one; and the empty list."""
    out = [[]]
    for v in sorted({abs(v) for v, _ in WORKED} | set(EDGES)):
        out += [[v], [5, 0, 7, v], [5, v, 7, 0], [v, v, v, v, v]]
    return out


def seeded_runs(n_pixels, nc, lead, seed):
    """nc run lengths that sum to n_pixels (the first one 0 when `lead`: pixel 0 is set), drawn from RUN_LENGTHS with a seeded
    generator as far as the pixels left allow, the last run taking the rest: multi-character values, the sign-guard group and negative
    deltas fall on both sides of every boundary."""
    rng = np.random.default_rng(seed)
    runs = [0] if lead else []
    left = n_pixels
    while len(runs) < nc - 1:
        need = nc - len(runs) - 1                                   # runs still to come, one pixel each at least
        fit = [r for r in RUN_LENGTHS if r <= left - need]
        runs.append(int(rng.choice(fit)))
        left -= runs[-1]
    runs.append(left)
    assert len(runs) == nc and sum(runs) == n_pixels and all(r > 0 for r in runs[1:]) and (runs[0] > 0) != bool(lead)
    return runs


def alternating_prefix_runs(n_pixels, nt):
    """nt transitions in the first nt + 1 pixels, the rest one run: the shape of the long-list cases."""
    assert 0 <= nt < n_pixels
    return [1] * nt + [n_pixels - nt]


def transitions(mask):
    """(positions int32, value of pixel 0) of a mask: what zh_mask_runs leaves for it."""
    f = np.asarray(mask).reshape(-1, order="F") != 0
    return (np.flatnonzero(f[1:] != f[:-1]) + 1).astype(np.int32), int(f[0])
