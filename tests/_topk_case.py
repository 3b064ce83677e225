"""Reference and case builders for the per-row top-k select (zh_topk_rows, csrc/retrieval.hip).  Host only: numpy, no torch, no GPU —
tests/test_topk_case_cpu.py proves every builder's preconditions, tests/test_topk_edges_gpu.py runs the kernel on the same cases.

`reference` states the CONTRACT without the kernel's key trick: every NaN first (either sign, any payload), then value descending
compared as float64 (so -0.0 ties with +0.0), then column ascending.  It is what torch.sort(descending=True, stable=True) gives.

`value_key` / `keys` restate the kernel's mapping of (float32, column) to one unsigned 64-bit key whose descending order IS the
contract: NaNs canonical (0xFFFFFFFF), zeros canonical (the key of +0.0).  `radix_trace` replays the kernel's eight histogram passes on
those keys and returns the bucket each pass stops in; the builders use it to assert that a case really puts a pass's pivot where it
says (bucket 255: the walk stops at once; bucket 0: it walks all 256 buckets; index bytes 2 and 3: the selection is decided above the
low 16 bits of the column).

A builder returns (x float32 [R, ld], N, k, expected int64 [R, k]).  Where a sort of the row would be slow the expectation is by
construction; test_topk_case_cpu.py checks such expectations against `reference` on a shrunken copy.
"""
import numpy as np

U32 = np.uint32
NAN_POS, NAN_NEG, NAN_SIG = 0x7FC00000, 0xFFC00000, 0x7F800001          # quiet, quiet with the sign bit (x86's 0 * inf), signalling
NAN_PATTERNS = (NAN_POS, NAN_NEG, NAN_SIG, 0xFFA00001, 0x7FFFFFFF, 0xFFFFFFFF)
MAXK = 1024                                                              # TOPK_MAXK of the kernel


def f32_of(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def bits_of(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ reference
def reference(row, k):
    """Columns of the k first entries of `row` (1-D float32) under the contract: NaN first, value descending as float64, column
    ascending."""
    row = np.asarray(row)
    assert row.ndim == 1 and row.dtype == np.float32 and 0 < k <= row.size
    nan = np.isnan(row)
    with np.errstate(invalid="ignore"):                                  # widening a signalling NaN raises the flag
        neg = np.where(nan, 0.0, -row.astype(np.float64))                # -(-0.0) == -(+0.0): a tie; NaNs tie among themselves
    return np.lexsort((np.arange(row.size), neg, ~nan))[:k].astype(np.int64)


def reference_rows(x, N, k):
    return np.stack([reference(r[:N], k) for r in x])


# ------------------------------------------------------------------------------------------------ the kernel's key mapping, restated
def value_key(x):
    """float32 -> uint32 whose unsigned order is the contract's value order: NaN -> 0xFFFFFFFF, +-0.0 -> 0x80000000."""
    u = bits_of(x)
    mag = (u & U32(0x7FFFFFFF)).astype(np.int64)
    key = (1 << 31) + np.where(u & U32(0x80000000), -mag, mag)            # 2^31 +- magnitude: -inf 0x00800000 .. +inf 0xFF800000
    return np.where(mag > 0x7F800000, 0xFFFFFFFF, key).astype(np.uint32)


def value_of_key(key):
    """The float32 whose value_key is `key`, +0.0 for the zeros' (keys outside [-inf, +inf] belong to no value and are refused)."""
    d = np.asarray(key, dtype=np.uint32).astype(np.int64) - (1 << 31)
    x = f32_of((np.abs(d) | np.where(d < 0, 1 << 31, 0)).astype(np.uint32))
    assert np.array_equal(value_key(x), np.asarray(key, dtype=np.uint32)), "not the key of a value"
    return x


def keys(row):
    row = np.asarray(row, dtype=np.float32)
    col = np.arange(row.size, dtype=np.uint64)
    return (value_key(row).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - col)


def radix_trace(row, k):
    """The kernel's radix select replayed on `keys(row)`: (bucket each of the 8 passes stops in, rank still wanted after each pass).
    Asserts that the decided prefix is the k-th largest key."""
    ks = keys(row)
    prefix, need, buckets, needs = np.uint64(0), k, [], []
    for p in range(8):
        shift = np.uint64(56 - 8 * p)
        himask = np.uint64(0) if p == 0 else np.uint64(0xFFFFFFFFFFFFFFFF) << (shift + np.uint64(8))
        live = ks[(ks & himask) == prefix]
        hist = np.bincount(((live >> shift) & np.uint64(255)).astype(np.int64), minlength=256)
        acc, b = 0, 255
        while acc + int(hist[b]) < need:
            acc += int(hist[b])
            b -= 1
            assert b >= 0
        prefix |= np.uint64(b) << shift
        need -= acc
        buckets.append(b)
        needs.append(need)
    assert need == 1 and prefix == np.sort(ks)[ks.size - k]
    return buckets, needs


# ------------------------------------------------------------------------------------------------ builders
RANDOM_BITS_K = (1, 500, 1024)


def random_bits(k, seed=11):
    """Random uint32 patterns as float32: every exponent, denormals, NaNs of both signs (about 1 in 128), and a few planted zeros and
    infinities of both signs."""
    R, N = 4, 5000
    g = np.random.default_rng(seed + k)
    u = g.integers(0, 1 << 32, (R, N), dtype=np.uint64).astype(np.uint32)
    plant = (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, NAN_POS, NAN_NEG, NAN_SIG)
    for r in range(R):
        pos = g.choice(N, 3 * len(plant), replace=False)
        u[r, pos] = np.tile(np.array(plant, dtype=np.uint32), 3)
    x = u.view(np.float32)
    assert all(np.isnan(r).sum() > 3 and np.signbit(r[np.isnan(r)]).any() and not np.signbit(r[np.isnan(r)]).all() for r in x)
    return x, N, k, reference_rows(x, N, k)


def signed_zero():
    """-0.0 and +0.0 are ties: the column decides.  Rows: the two interleaved (both phases), all -0.0, the zeros among negatives (fewer
    and more than k of them), among denormals of both signs, and the five-element example padded with -1."""
    N, k = 300, 40
    g = np.random.default_rng(21)
    nz, pz = np.float32(-0.0), np.float32(0.0)
    rows = []
    a = np.empty(N, np.float32); a[0::2] = nz; a[1::2] = pz; rows.append(a)
    a = np.empty(N, np.float32); a[0::2] = pz; a[1::2] = nz; rows.append(a)
    rows.append(np.full(N, nz, np.float32))
    for nzero in (25, 60):
        a = -(g.random(N, dtype=np.float32) + np.float32(0.5))
        pos = np.sort(g.choice(N, nzero, replace=False))
        a[pos] = np.where(g.integers(0, 2, nzero) == 1, nz, pz)
        a[pos[0]], a[pos[1]] = nz, pz                                   # the first zero is a -0.0, a +0.0 follows it
        rows.append(a)
    a = f32_of(g.integers(1, 1 << 23, N).astype(np.uint32) | (g.integers(0, 2, N).astype(np.uint32) << U32(31))).copy()    # +-denormals
    pos = np.sort(g.choice(N, 30, replace=False))
    a[pos] = np.where(np.arange(30) % 2 == 0, nz, pz)
    rows.append(a)
    a = np.full(N, -1.0, np.float32); a[:4] = (nz, pz, nz, pz); rows.append(a)
    x = np.stack(rows)
    exp = reference_rows(x, N, k)
    assert np.array_equal(exp[0], np.arange(k)) and np.array_equal(exp[1], np.arange(k)) and np.array_equal(exp[2], np.arange(k))
    assert np.array_equal(exp[-1][:4], [0, 1, 2, 3])
    return x, N, k, exp


NAN_SIGNS_COUNT = len(NAN_PATTERNS)
NAN_SIGNS_K = (NAN_SIGNS_COUNT - 2, NAN_SIGNS_COUNT, NAN_SIGNS_COUNT + 3)


def nan_signs(k, seed=31):
    """Six NaNs per row (both signs, quiet and signalling, all-ones payloads), two +inf, one large finite value, the rest standard normal,
    in shuffled positions.  Expectation by construction: the NaN columns ascending, the +inf columns ascending, then the large value."""
    R, N = 5, 200
    g = np.random.default_rng(seed)
    x = g.standard_normal((R, N)).astype(np.float32)
    exp = np.empty((R, NAN_SIGNS_COUNT + 3), np.int64)
    for r in range(R):
        pos = g.choice(N, NAN_SIGNS_COUNT + 3, replace=False)
        u = x[r].view(np.uint32)
        u[pos[:NAN_SIGNS_COUNT]] = np.array(NAN_PATTERNS, dtype=np.uint32)[g.permutation(NAN_SIGNS_COUNT)]
        x[r, pos[NAN_SIGNS_COUNT:NAN_SIGNS_COUNT + 2]] = np.inf
        x[r, pos[-1]] = np.float32(3e38)
        exp[r] = np.concatenate([np.sort(pos[:NAN_SIGNS_COUNT]), np.sort(pos[NAN_SIGNS_COUNT:NAN_SIGNS_COUNT + 2]), pos[-1:]])
    assert k <= exp.shape[1]
    return x, N, k, exp[:, :k].copy()


# one (pass, low) per row of the table in the module docstring of test_topk_edges_gpu.py; pass 4 low and pass 5 low are out of reach of
# a small row: the k-th column would need byte 3 == 0xFF (a 17 GB row) or byte 2 == 0xFF (column >= 0xFF0000: index_byte2_low below)
PIVOT_CASES = [(p, low) for p in range(8) for low in (False, True) if (p, low) not in ((4, True), (5, True))]
_PREFIX = (0xC1, 0x37, 0x5A)                                             # shared top value-key bytes of the passes 1..3 rows


def _tie_window(N, start, width, k, tie, background=-1.0):
    x = np.full((1, N), background, np.float32)
    x[0, start:start + width] = tie
    assert 0 < k <= width and start + width <= N and tie > background
    return x, N, k, np.arange(start, start + k, dtype=np.int64)[None]


def pivot_buckets(p, low, seed=41):
    """One row whose pass-p histogram walk stops in bucket 255 (low=False: at its first step) or in bucket 0 (low=True: after walking
    all 256 buckets).  Passes 0..3 read the value key's bytes, 4..7 the inverted column's.  Asserted with radix_trace."""
    g = np.random.default_rng(seed + 2 * p + int(low))
    t = 0x00 if low else 0xFF
    if p < 4:
        N, n_pivot = 600, 120
        lowbits = 8 * (3 - p)
        if p == 0:
            # top key byte 0xFF: finite values >= 2^127 and +inf; 0x00: values < -2^127 and -inf.  The rest: any finite pattern
            rest = value_key(f32_of(g.integers(0, 0x7F000000, N - n_pivot).astype(np.uint32) | (g.integers(0, 2, N - n_pivot).astype(np.uint32) << U32(31))))
            rest = rest[(rest >> U32(24) != 0xFF) & (rest >> U32(24) != 0x00)]
            piv = (U32(0xFF000000) + g.integers(0, 0x800000, n_pivot).astype(np.uint32)) if not low else \
                  (U32(0x00FFFFFF) - g.integers(0, 0x800000, n_pivot).astype(np.uint32))
            piv[:5] = value_key(np.float32(-np.inf if low else np.inf))
            others = [rest]
        else:
            pre = 0
            for b in _PREFIX[:p]:
                pre = (pre << 8) | b
            pre <<= 8 * (4 - p)
            # same top p bytes, any byte p but the pivot's; a greater and a smaller prefix; the pivot bucket itself
            same = U32(pre) | (g.integers(1, 255, 200).astype(np.uint32) << U32(lowbits)) | g.integers(0, 1 << lowbits, 200).astype(np.uint32) \
                if lowbits else U32(pre) | g.integers(1, 255, 200).astype(np.uint32)
            span = 1 << (8 * (4 - p))
            above = U32(pre + span) + g.integers(0, span, 60).astype(np.uint32)
            below = U32(pre - span) + g.integers(0, span, 60).astype(np.uint32)
            piv = (U32(pre) | U32(t << lowbits)) + (g.integers(0, 1 << lowbits, n_pivot).astype(np.uint32) if lowbits else np.zeros(n_pivot, np.uint32))
            others = [same, above, below]
        allk = np.concatenate(others + [piv])
        n_above = int(sum((o > piv.max()).sum() for o in others))
        k = n_above + n_pivot // 2                                       # the k-th largest lies inside the pivot bucket
        x = value_of_key(allk[g.permutation(allk.size)])[None].copy()
        N = x.shape[1]
        case = x, N, k, reference_rows(x, N, k)
    else:
        # the k-th column c decides: byte j of the inverted column is 0xFF - byte j of c (j = 7 - p)
        j = 7 - p
        c = {(3, False): 700, (2, False): 300, (1, False): 200, (0, False): 512, (1, True): 0xFF13, (0, True): 0x2FF}[(j, low)]
        if c < MAXK:                                                      # an all-equal row: the k-th column is k - 1
            case = _tie_window(c + 300, 0, c + 300, c + 1, 0.5)
        else:                                                             # byte 1 == 0xFF needs a column past 65280: ties in a window
            case = _tie_window(c + 500, c - 299, 700, 300, 0.5)
        assert case[3][0, -1] == c and ((c >> (8 * j)) & 255) == (0xFF if low else 0x00)
    buckets, _ = radix_trace(case[0][0, :case[1]], case[2])
    assert buckets[p] == t, (p, low, buckets)
    return case


def index_byte2(N=70000, start=65000, width=2000, k=1000):
    """Background -1, ties 0.5 at [65000, 67000): the 1000 selected columns cross 65536, so index byte 2 decides (pass 5 stops in
    bucket 0xFE with 464 still wanted)."""
    return _tie_window(N, start, width, k, 0.5)


def index_byte3(N=(1 << 24) + 300, start=(1 << 24) - 100, width=200, k=150):
    """Background -1, ties 2.0 at [2^24 - 100, 2^24 + 100): the selected columns cross 2^24, so index byte 3 decides (pass 4 stops in
    bucket 0xFE with 50 still wanted).  67 MB; expectation by construction."""
    return _tie_window(N, start, width, k, 2.0)


def index_byte2_low(N=0xFF0000 + 400, start=0xFF0000 - 100, width=400, k=250):
    """The twin pivot_buckets cannot build small: the k-th column has byte 2 == 0xFF, so pass 5 walks down to bucket 0.  67 MB."""
    return _tie_window(N, start, width, k, 2.0)


def tie_window_pivot(case):
    """(buckets, needs) of a _tie_window case without sorting 16 M keys: only the tied columns can hold the k-th key."""
    x, N, k, exp = case
    tied = np.flatnonzero(x[0, :N] == x[0, exp[0, 0]])
    assert np.array_equal(tied[:k], exp[0])
    ks = (np.uint64(value_key(x[0, exp[0, :1]])[0]) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - tied.astype(np.uint64))
    kth = int(ks[k - 1])
    buckets = [(kth >> (56 - 8 * p)) & 255 for p in range(8)]
    needs = [int((ks[:k] >> np.uint64(56 - 8 * p) == np.uint64(kth >> (56 - 8 * p))).sum()) for p in range(8)]
    return buckets, needs


SMALL_N = ((1, 1), (2, 2), (63, 63), (255, 255), (256, 256), (257, 257), (1024, 1024), (1025, 1024))


def small_n(N, k, seed=51):
    """A standard-normal row, a row of few distinct values and an all-equal row, at the sizes around the block (256) and TOPK_MAXK."""
    g = np.random.default_rng(seed + N)
    x = np.stack([g.standard_normal(N).astype(np.float32), g.integers(-2, 3, N).astype(np.float32), np.full(N, 0.5, np.float32)])
    return x, N, k, reference_rows(x, N, k)


def many_rows(seed=61):
    """919 rows (the category count), one workgroup each: every row its own values, one tie-heavy row in the middle."""
    R, N, k = 919, 300, 7
    g = np.random.default_rng(seed)
    x = g.standard_normal((R, N)).astype(np.float32)
    x[R // 2] = g.integers(0, 2, N).astype(np.float32)
    x[R // 2, :20] = 0.0
    return x, N, k, reference_rows(x, N, k)


def merge_case():
    """Two chunk lists of 7 candidates per row, each sorted by the contract, as retrieve_topk lays them out (chunk-major: columns
    0..6 carry image indices < 100, columns 7..13 indices >= 100).  Row 0: the 7th place of the union is a zero that is -0.0 in the
    first list while the second holds +0.0.  Row 1: the first list leads with a sign-bit NaN.  -> (cand_idx, cand_val, k, expected
    columns [2, k])."""
    nz, nan_neg = np.float32(-0.0), f32_of(NAN_NEG)[()]
    val = np.array([[3.0, 1.0, nz, nz, -1.0, -2.0, -3.0, 4.0, 2.0, 1.0, 1.0, 0.0, 0.0, -5.0],
                    [nan_neg, 3.0, 1.0, 0.0, -1.0, -2.0, -3.0, np.inf, 2.0, 1.0, nz, nz, -4.0, -5.0]], dtype=np.float32)
    idx = np.array([[7, 2, 9, 40, 3, 5, 8, 103, 101, 150, 170, 104, 120, 199],
                    [5, 7, 2, 9, 3, 4, 8, 103, 101, 150, 104, 120, 110, 199]], dtype=np.int64)
    k = 7
    exp = np.array([[7, 0, 8, 1, 9, 10, 2], [0, 7, 1, 8, 2, 9, 3]], dtype=np.int64)
    return idx, val, k, exp
