"""Cases and float-free references for the device RLE kernels (csrc/mask_rle.hip: zh_mask_runs, zh_mask_runs_kept, zh_mask_rle_kept,
zh_mask_rle_fused_kept) at their capacity and tile edges.  Plain helper module (no fixtures, no pytest hooks): seeds and shapes in,
masks, kept tables and references out.  tests/test_rle_guard_case_cpu.py proves that the cases have the structure they claim,
tests/test_rle_guard_gpu.py runs them inside tests/_guard.py arenas.

References
  * transition list of a mask: with f = mask.reshape(-1, order="F") != 0, np.nonzero(f[1:] != f[:-1])[0] + 1;
  * box and area: numpy (an empty mask has the box (W, H, -1, -1));
  * string: zutis_amd.rle.encode, the host encoder (tests/test_rle.py holds it to pycocotools' vectors); of a crafted run list,
    zutis_amd.rle._to_string;
  * capacities: restated here from the text of include/zutis_hip.h, not imported from zutis_amd.instances.

The kernels' tile constants are restated as well (the CPU test holds the cases to them, the GPU test holds the kernels to the cases).
"""
import numpy as np

RUNS_PANEL, RUNS_SEG = 64, 4                 # zh_mask_runs*: columns per panel (one workgroup), row segments per column
FRLE_COLS, FRLE_ROWS = 32, 16                # zh_mask_rle_fused_kept: an item is 32 columns by 16 rows
RLE_LDS_RUNS = 8192                          # zh_mask_rle_kept: lists up to this length are copied to LDS, longer ones read in place
RLE_CHUNK = 256                              # ... and values are scanned 256 at a time
FIVE_CHAR_PIXELS = 1 << 24                   # below this many pixels no value takes more than 5 characters
FILL32 = int(np.frombuffer(bytes([0xA5] * 4), np.int32)[0])      # an int32 of an untouched output arena

PANEL_W, PANEL_H = (1, 63, 64, 65, 72, 80, 144), (1, 3, 4, 5, 37)
FUSED_MULTI = ((1040, 1), (520, 33), (640, 480), (640, 427))     # (H, W): more items than threads
FUSED_SINGLE = ((480, 640), (500, 375))                          # the controls: at most one item per thread
FUSED_W, FUSED_H = (1, 31, 32, 33, 63, 64, 65, 1023, 1024), (1, 15, 16, 17, 33)
FUSED_WIDE_H = {1023: (17,), 1024: (33,)}                        # one H at the two widest
NC_EDGES = (1, 2, 255, 256, 257, 512, 513)
BIG_A = (1 << 24) + 2


# ------------------------------------------------------------------------------------------------ references
def flat(mask):
    return np.asarray(mask).reshape(-1, order="F") != 0


def transitions(mask):
    f = flat(mask)
    return (np.nonzero(f[1:] != f[:-1])[0] + 1).astype(np.int64)


def lead_of(mask):
    return int(np.asarray(mask).flat[0] != 0)


def box_area(mask):
    """(xmin, ymin, xmax, ymax, area), inclusive; an empty mask: (W, H, -1, -1, 0)."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    if not m.any():
        return (W, H, -1, -1, 0)
    ys, xs = np.nonzero(m)
    return (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()), int(m.sum()))


def string_of_mask(mask):
    from zutis_amd import rle
    return rle.encode((np.asarray(mask) != 0).astype(np.uint8))["counts"]


def string_of_runs(runs):
    from zutis_amd import rle
    return rle._to_string(np.asarray(runs, np.int64))


def runs_of(positions, lead, HW):
    """The run lengths of a transition list: diff([0, positions..., HW]), an empty run of zeros in front when pixel 0 is set."""
    r = np.diff(np.concatenate(([0], np.asarray(positions, np.int64), [HW]))).tolist()
    return ([0] if lead else []) + [int(x) for x in r]


def stored_values(runs):
    """The values the string stores: run k, from the fourth on minus run k - 2."""
    return [int(r) - (int(runs[k - 2]) if k > 2 else 0) for k, r in enumerate(runs)]


def groups(x):
    """Characters of a value: the smallest n with -2^(5n-1) <= x < 2^(5n-1)."""
    n = 1
    while not -(1 << (5 * n - 1)) <= x < (1 << (5 * n - 1)):
        n += 1
    return n


# ------------------------------------------------------------------------------------------------ capacity arithmetic (zutis_hip.h)
def place(nts, max_runs):
    """Per kept mask, in kept order across the batch: (off, rank, cstart) — off = sum of min(transitions, max_runs) over the kept masks
    in front of it (the start of its list in the packed positions), rank = their number, cstart = 5 * off + 16 * rank."""
    out, off = [], 0
    for rank, nt in enumerate(nts):
        out.append((off, rank, 5 * off + 16 * rank))
        off += min(int(nt), max_runs)
    return out


def packed_total(nts, max_runs):
    return sum(min(int(nt), max_runs) for nt in nts)


def packed_written(off, nt, max_runs, packed_capacity):
    """Number of entries of a mask's list that the packed form writes: those of its min(nt, max_runs) that lie below the capacity."""
    return int(max(0, min(min(nt, max_runs), packed_capacity - off)))


def list_fits(off, nt, max_runs, packed_capacity):
    return nt <= max_runs and off + nt <= packed_capacity


def string_fits(cstart, nt, lead, length, HW, out_capacity):
    """zh_mask_rle_kept writes a string (given that its list fits): below 2^24 pixels when `out` holds 5 characters for each of its
    nc values; from 2^24 on when its true length fits [cstart, min(cstart + 5 nt + 16, out_capacity))."""
    nc = nt + 1 + lead
    if HW < FIVE_CHAR_PIXELS:
        return cstart + 5 * nc <= out_capacity
    return length <= min(5 * nt + 16, out_capacity - cstart)


def expected_strings(lists, max_runs, HW, packed_capacity, out_capacity):
    """lists: per kept mask (positions, lead).  -> (out_len per mask, {cstart: string} of the strings that are written)."""
    lens, written = [], {}
    for (pos, lead), (off, _, cstart) in zip(lists, place([len(p) for p, _ in lists], max_runs)):
        nt = len(pos)
        s = string_of_runs(runs_of(pos, lead, HW))
        ok = list_fits(off, nt, max_runs, packed_capacity) and string_fits(cstart, nt, lead, len(s), HW, out_capacity)
        lens.append(len(s) if ok else -1)
        if ok:
            written[cstart] = s
    return lens, written


# ------------------------------------------------------------------------------------------------ which path a case takes
def panel_staging(W, misalign=0):
    """zh_mask_runs*: a panel is staged with 16-byte loads when W % 16 == 0 and the mask's base is 16-byte aligned (every panel is then
    a multiple of 16 columns wide), else byte by byte."""
    return "vector" if W % 16 == 0 and misalign % 16 == 0 else "scalar"


def list_source(nt):
    return "lds" if nt <= RLE_LDS_RUNS else "global"


def fused_items_threads(H, W):
    return -(-W // FRLE_COLS) * -(-H // FRLE_ROWS), -(-W // 64) * 64


def fused_packing(H, W, misalign=0):
    """zh_mask_rle_fused_kept from bytes: 16-byte loads when H*W % 16 == 0 and the mask's base is aligned, else the byte loop."""
    return "vector" if (H * W) % 16 == 0 and misalign % 16 == 0 else "bytes"


def frle_layout(H, W, max_runs):
    """The LDS layout of the fused kernel: bits (u64 [n64 + 2]), counts (u16 [S][Wp]); the string (5 (max_runs + 2) bytes, rounded to 16)
    is built over the two once they are dead; column offsets (int [Wp]) and the list (int [max_runs]) start behind the larger."""
    n64 = (H * W + 63) >> 6
    Wp, S = -(-W // 64) * 64, -(-H // FRLE_ROWS)
    dead = (n64 + 2) * 8 + S * Wp * 2
    string = (5 * (max_runs + 2) + 15) // 16 * 16
    start = max(dead, string)
    return dict(dead=dead, string=string, branch="string" if string > dead else "bits", total=start + Wp * 4 + max_runs * 4)


# ------------------------------------------------------------------------------------------------ builders
def mask_with_transitions(H, W, n, first=0):
    """Exactly n transitions: the first n + 1 column-major pixels alternate (pixel 0 = first), the rest hold the last value."""
    assert 0 <= n < H * W
    f = np.empty((H * W,), np.uint8)
    f[:n + 1] = (np.arange(n + 1) + first) & 1
    f[n + 1:] = f[n]
    return np.ascontiguousarray(f.reshape((H, W), order="F"))


def mask_first_pixel_set(H, W, seed, density=0.5):
    m = (np.random.default_rng(seed).random((H, W)) < density).astype(np.uint8)
    m[0, 0] = 1
    return m


def list_from_runs(runs):
    """A (positions, lead, HW) triple with no mask at all: runs[0] == 0 is the empty leading run of a set pixel 0."""
    runs = [int(r) for r in runs]
    lead = int(runs[0] == 0)
    body = runs[lead:]
    assert all(r > 0 for r in body)
    edges = np.cumsum(body)
    assert edges[-1] < (1 << 31)
    return edges[:-1].astype(np.int64), lead, int(edges[-1])


# both sides of every group-count edge below 2^24: 15 | 16 and -16 | -17, then the same at 2^9, 2^14 and 2^19
VALUE_EDGES = tuple(x for n in (4, 9, 14, 19) for x in ((1 << n) - 1, -(1 << n), 1 << n, -(1 << n) - 1))


def value_edge_runs():
    """A lead run, a run of 1, then even runs that step by every value of VALUE_EDGES from 600 000 (a positive step, then the negative
    one a little larger: the run stays near its start) between odd runs of 1 (delta 0).  Under 2^24 pixels in all."""
    runs, even = [0, 1, 600000], 600000
    for d in VALUE_EDGES:
        even += d
        runs += [1, even]
    return runs


def big_runs(n):
    """A, A, 1, 1, A, A, 1, 1, ... (n runs) with A = 2^24 + 2: every value from the fourth on is +-(A - 1), six characters."""
    return [BIG_A if k % 4 < 2 else 1 for k in range(n)]


def noise_density(H, W, target=1500):
    """Noise that stays below a few thousand transitions however large the mask is (the fused kernel's list lives in LDS)."""
    return min(0.5, target / (2.0 * H * W))


def mask_set(H, W, seed):
    """name -> u8 [H, W]: the masks every shape is run with."""
    rng = np.random.default_rng(seed)
    z = lambda: np.zeros((H, W), np.uint8)
    m = {"empty": z(), "full": np.ones((H, W), np.uint8), "pixel0": z(), "last_pixel": z(), "last_row": z(), "col_stripes": z(),
         "row_stripes": z(), "noise": (rng.random((H, W)) < noise_density(H, W)).astype(np.uint8), "bytes": z(), "last_col": z()}
    m["pixel0"][0, 0] = 1
    m["last_pixel"][H - 1, W - 1] = 1
    m["last_row"][H - 1, :] = 1                                     # every column ends set and the next starts clear: the H-1 -> 0 wrap
    m["col_stripes"][:, ::2] = 1
    m["row_stripes"][::2, :] = 1                                    # 16 transitions in a 16-row chunk
    pick = rng.random((H, W)) < max(noise_density(H, W), 0.02)
    m["bytes"][pick] = np.array([0x02, 0x80, 0xFF], np.uint8)[rng.integers(0, 3, int(pick.sum()))]
    m["last_col"][:, W - 1] = 1                                     # the row-0 rule across the column boundary
    m["last_col"][H - 1, max(W - 2, 0)] = 1
    return m


def kept_table(B, Q, orders):
    """orders: per image the kept query indices.  -> (kept_index int32 [B, Q], kept_count int32 [B]); entries past the count hold -1."""
    idx = np.full((B, Q), -1, np.int32)
    for b, o in enumerate(orders):
        idx[b, :len(o)] = o
    return idx, np.array([len(o) for o in orders], np.int32)


def kept_orders(Q, seed):
    """Three images: every query in a shuffled order, none (a middle image with count 0), and the first half in reverse."""
    rng = np.random.default_rng(seed)
    return [rng.permutation(Q).tolist(), [], list(range(Q // 2, -1, -1))]


def packed_capacities(nts, max_runs):
    """name -> capacity (> 0): the sum of the lists, one less, the middle of a middle mask's list (every later mask has negative room),
    and 1."""
    lens = [min(int(n), max_runs) for n in nts]
    total, caps = sum(lens), {}
    if total > 0:
        caps["exact"] = total
    if total > 1:
        caps["minus1"] = total - 1
    starts = np.concatenate(([0], np.cumsum(lens)))
    mids = [i for i in range(1, len(lens) - 1) if lens[i] >= 2]
    if mids:
        i = mids[len(mids) // 2]
        caps["inside"] = int(starts[i] + lens[i] // 2)
    if total > 2:
        caps["one"] = 1
    return caps


# ------------------------------------------------------------------------------------------------ the string kernel's mask cases
def nc_edge_case():
    """(H, W, masks, orders, max_runs): nc = nt + 1 + lead in NC_EDGES with alternating values of pixel 0, 256 and 257 with the other
    value as well; three images, the middle one with no kept mask."""
    H = W = 24
    masks = [mask_with_transitions(H, W, nc - 1 - (i % 2 if nc > 1 else 0), i % 2 if nc > 1 else 0) for i, nc in enumerate(NC_EDGES)]
    masks += [mask_with_transitions(H, W, 255, lead) for lead in (0, 1)]
    return H, W, masks, [list(range(len(masks))), [], [8, 3, 0, 6]], 8192


def over_max_runs_case():
    """max_runs = 300 below the transitions of masks in the middle of both images."""
    H = W = 24
    return H, W, [mask_with_transitions(H, W, nt, nt & 1) for nt in (5, 511, 300, 301, 0, 17)], [[0, 1, 2, 3, 4, 5], [5, 3, 0]], 300


def lds_edge_case():
    """Lists of RLE_LDS_RUNS and RLE_LDS_RUNS + 1 entries and a short one, at max_runs = 8200."""
    H = W = 96
    masks = [mask_with_transitions(H, W, RLE_LDS_RUNS, 0), mask_with_transitions(H, W, RLE_LDS_RUNS + 1, 1), mask_first_pixel_set(H, W, 3, 0.02)]
    return H, W, masks, [[0, 1, 2], [1, 0]], 8200


def kept_lists(masks, orders):
    """Per kept mask, image-major in kept order: (transition list, lead)."""
    return [(transitions(masks[q]), lead_of(masks[q])) for o in orders for q in o]


def last_needed(lists, max_runs):
    """`out` up to the last byte the last kept string is checked for (below 2^24 pixels): its cstart + 5 nc."""
    nts = [len(p) for p, _ in lists]
    return place(nts, max_runs)[-1][2] + 5 * (nts[-1] + 1 + lists[-1][1])


def big_case(n_runs):
    """The runs of big_runs(n_runs) between two ordinary lists: (lists, HW)."""
    pos, lead, HW = list_from_runs(big_runs(n_runs))
    return [(np.array([5, 9], np.int64), 0), (pos, lead), (np.array([7], np.int64), 1)], HW


def value_edge_case():
    pos, lead, HW = list_from_runs(value_edge_runs())
    return [(np.array([3, 10], np.int64), 0), (pos, lead), (np.array([1], np.int64), 1)], HW
