"""tests/_topk_case.py on the CPU: the reference is torch's stable descending sort, the restated key order is the reference, every
builder's row puts the radix pivot where it says, and the by-construction expectations are the reference's."""
import numpy as np
import pytest
import torch

from tests import _topk_case as K


def _torch_order(row, k):
    return torch.sort(torch.from_numpy(np.ascontiguousarray(row)), descending=True, stable=True).indices[:k].numpy()


def _small_cases():
    yield "signed_zero", K.signed_zero()
    for k in K.RANDOM_BITS_K:
        yield f"random_bits-{k}", K.random_bits(k)
    for k in K.NAN_SIGNS_K:
        yield f"nan_signs-{k}", K.nan_signs(k)
    for N, k in K.SMALL_N:
        yield f"small_n-{N}", K.small_n(N, k)
    for p, low in K.PIVOT_CASES:
        yield f"pivot-{p}-{int(low)}", K.pivot_buckets(p, low)
    yield "many_rows", tuple(a[455:464] if isinstance(a, np.ndarray) else a for a in K.many_rows())


def test_reference_is_torch_stable_descending_sort_and_the_key_order():
    """NaNs of either sign first in column order, -0.0 tied with +0.0: torch defines all of it, and the corrected 64-bit keys sort
    the same way."""
    for name, (x, N, k, exp) in _small_cases():
        assert x.dtype == np.float32 and exp.dtype == np.int64 and exp.shape == (x.shape[0], k) and 0 < k <= min(N, K.MAXK), name
        for r in range(x.shape[0]):
            row = x[r, :N]
            assert np.array_equal(K.reference(row, k), exp[r]), (name, r)
            assert np.array_equal(_torch_order(row, k), exp[r]), (name, r)
            ks = K.keys(row)
            assert np.unique(ks).size == N and np.array_equal(np.argsort(ks)[::-1][:k], exp[r]), (name, r)


def test_the_issue_examples():
    z = np.array([-0.0, 0.0, -0.0, 0.0, -1.0], np.float32)
    assert K.reference(z, 4).tolist() == [0, 1, 2, 3]
    n = np.array([1.0, np.nan, np.inf, 0.0, -np.inf], np.float32)
    n.view(np.uint32)[3] = K.NAN_NEG
    assert K.reference(n, 5).tolist() == [1, 3, 2, 0, 4] == _torch_order(n, 5).tolist()
    # the mapping before the correction, replayed: -0.0 below +0.0, a sign-bit NaN below -inf
    def old_order(row):
        u = row.view(np.uint32)
        key = np.where(u & K.U32(0x80000000), ~u, u | K.U32(0x80000000)).astype(np.uint64) << np.uint64(32)
        return np.argsort(key | (np.uint64(0xFFFFFFFF) - np.arange(row.size, dtype=np.uint64)))[::-1].tolist()
    assert old_order(z)[:4] == [1, 3, 0, 2] and old_order(n) == [1, 2, 0, 4, 3]


def test_value_key_is_canonical_and_monotone():
    x = K.f32_of(np.array(K.NAN_PATTERNS + (0x7F800000, 0x7F7FFFFF, 0x00800000, 0x007FFFFF, 0x00000001, 0x00000000, 0x80000000, 0x80000001,
                                            0x807FFFFF, 0x80800000, 0xFF7FFFFF, 0xFF800000), dtype=np.uint32))
    key = K.value_key(x)
    n = len(K.NAN_PATTERNS)
    assert (key[:n] == 0xFFFFFFFF).all() and key[n + 5] == key[n + 6] == 0x80000000
    rest = np.delete(key[n:], 6)                                          # descending values, the second zero dropped: strictly descending keys
    assert (np.diff(rest.astype(np.int64)) < 0).all() and rest[0] < 0xFFFFFFFF
    assert np.array_equal(K.bits_of(K.value_of_key(rest)), np.delete(K.bits_of(x[n:]), 6))
    with pytest.raises(AssertionError):
        K.value_of_key(np.array([0xFF800001], np.uint32))                  # above +inf, below the NaNs' key: no value maps there


@pytest.mark.parametrize("p,low", K.PIVOT_CASES)
def test_pivot_rows_hit_their_bucket(p, low):
    x, N, k, exp = K.pivot_buckets(p, low)
    buckets, needs = K.radix_trace(x[0, :N], k)
    assert buckets[p] == (0 if low else 255)
    if p < 4:                                                             # the value rows: the pivot bucket holds more than the k-th alone
        assert needs[p] > 1
    assert np.array_equal(exp[0], K.reference(x[0, :N], k))


def test_pivot_passes_out_of_reach_of_a_small_row():
    """Pass 4 (index byte 3) cannot stop in bucket 0 below column 0xFF000000, pass 5 not below 0xFF0000: the large twin covers pass 5."""
    assert [c for c in ((4, True), (5, True)) if c in K.PIVOT_CASES] == []
    buckets, needs = K.tie_window_pivot(K.index_byte2_low())
    assert buckets[5] == 0 and buckets[4] == 0xFF and needs[5] < 250


def test_index_byte_cases_by_construction():
    for build, p, small in ((K.index_byte2, 5, dict(N=70000)), (K.index_byte3, 4, dict(N=(1 << 24) + 300))):
        case = build()
        x, N, k, exp = case
        assert x.shape == (1, N) == (1, small["N"]) and exp.shape == (1, k)
        buckets, needs = K.tie_window_pivot(case)
        lo, hi = int(exp[0, 0]), int(exp[0, -1])
        shift = 8 * (7 - p)
        assert lo >> shift != hi >> shift                                 # the selected set crosses the byte boundary
        assert buckets[p] == 0xFE and buckets[:4] == [b for b in K.value_key(x[0, lo:lo + 1])[0].tobytes()[::-1]]
        assert 1 < needs[p] < k and needs[p] == hi - ((hi >> shift) << shift) + 1
    # index_byte2 is small enough for the full replay and the sort
    x, N, k, exp = K.index_byte2()
    assert K.radix_trace(x[0], k) == K.tie_window_pivot((x, N, k, exp))
    assert np.array_equal(K.reference(x[0], k), exp[0])
    # index_byte3 and its twin on a shrunken copy: the same window, 600 columns either side of it
    for build in (K.index_byte3, K.index_byte2_low):
        x, N, k, exp = build()
        lo = int(exp[0, 0]) - 600
        cut = x[0, lo:min(N, lo + 1500)]
        assert np.array_equal(K.reference(cut, k) + lo, exp[0])
        assert (x[0, :lo] == -1.0).all() and (x[0, lo + 1500:] == -1.0).all()      # nothing but background outside the copy


def test_nan_signs_and_merge_case_by_construction():
    for k in K.NAN_SIGNS_K:
        x, N, k_, exp = K.nan_signs(k)
        nan = np.isnan(x)
        assert (nan.sum(1) == K.NAN_SIGNS_COUNT).all() and np.signbit(x[nan]).any() and not np.signbit(x[nan]).all()
        assert np.array_equal(exp, K.reference_rows(x, N, k))
    idx, val, k, exp = K.merge_case()
    half = idx.shape[1] // 2
    for r in range(2):
        for part in (slice(0, half), slice(half, None)):                 # each list sorted by the contract on (score, image index)
            v, i = val[r, part], idx[r, part]
            assert np.array_equal(K.reference(v, half), np.arange(half))
            assert all(i[a] < i[a + 1] for a in range(half - 1) if v[a] == v[a + 1] or (np.isnan(v[a]) and np.isnan(v[a + 1])))
        assert idx[r, :half].max() < idx[r, half:].min()                  # chunk-major
        assert np.array_equal(K.reference(val[r], k), exp[r])
        # the same answer from the union laid out by image index
        dense = np.full(200, -np.inf, np.float32)
        dense[idx[r]] = val[r]
        assert np.array_equal(K.reference(dense, k), idx[r, exp[r]])
    assert np.signbit(val[0, exp[0, -1]]) and val[0, exp[0, -1]] == 0 and not np.signbit(val[0, 11]) and val[0, 11] == 0
    assert K.bits_of(val[1, :1])[0] == K.NAN_NEG
