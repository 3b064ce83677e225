import ctypes

import numpy as np
import pytest

from tests import _rle_case as RC
from tests._rle_case import mask_from_runs as _mask_from_runs
from zutis_amd import _lib, rle, detgen


def test_rle_round_trip_and_format():
    for seed, shape in enumerate([(7, 5), (80, 112), (1, 1), (33, 64)]):
        m = detgen.det_normal("rle", shape, seed=seed) > 0.3
        r = rle.encode(m)
        assert r["size"] == list(shape) and isinstance(r["counts"], bytes)
        assert all(48 <= c < 48 + 64 for c in r["counts"])
        assert np.array_equal(rle.decode(r).astype(bool), m)
    z = np.zeros((4, 6), bool)
    assert np.array_equal(rle.decode(rle.encode(z)), z)
    o = np.ones((4, 6), bool)
    assert rle._counts(o).tolist() == [0, 24]                       # leading zero-run of length 0
    assert np.array_equal(rle.decode(rle.encode(o)).astype(bool), o)
    # long runs and negative deltas exercise the sign-extension branch
    big = np.zeros((300, 300), bool)
    big[5:290, 7] = True
    big[0:3, 200] = True
    assert np.array_equal(rle.decode(rle.encode(big)).astype(bool), big)


def test_known_counts_string():
    # column-major runs of [[0,1],[1,1]] are 1 zero, 3 ones -> counts [1,3] -> chars '1','3'
    assert rle.encode(np.array([[0, 1], [1, 1]], bool))["counts"] == b"13"


def test_mask_to_box():
    m = np.zeros((10, 12), bool)
    m[2:5, 3:9] = True
    assert rle.mask_to_box(m) == [3.0, 2.0, 8.0, 4.0]


def test_c_helper_matches_python_restatement():
    for seed, shape in enumerate([(7, 5), (80, 112), (1, 1), (33, 64), (336, 336)]):
        m = detgen.det_normal("rlec", shape, seed=seed) > 0.8
        assert rle.encode(m)["counts"] == rle.encode_py(m)["counts"]
    for m in (np.zeros((4, 6), bool), np.ones((4, 6), bool)):
        assert rle.encode(m)["counts"] == rle.encode_py(m)["counts"]
    big = np.zeros((300, 300), bool); big[5:290, 7] = True; big[0:3, 200] = True
    assert rle.encode(big)["counts"] == rle.encode_py(big)["counts"]


def test_rle_hand_derived_format_vectors(golden_dir):
    """RLE byte strings pinned to vectors derived BY HAND from the published COCO format (pycocotools maskApi.c rleToString;
    the package is absent), tests/golden/rle_vectors.json.  Worked examples (c = x & 31; x >>= 5; more = bit4(c) ? x != -1 :
    x != 0; char = (c | 32*more) + 48; counts i > 2 stored minus counts[i-2]):
      9            -> c=9, x=0, stop                      -> '9'
      40           -> c=8, x=1, more -> 8|32=40 -> 'X'; then c=1 -> '1'            -> "X1"
      1 - 2 = -1   -> c=31, x=-1, bit4 set and x == -1 -> stop -> 31+48 -> 'O'
      1000         -> c=8,x=31 -> 'X'; c=31,x=0, bit4 set, 0 != -1 -> more -> 63+48 -> 'o'; c=0 -> '0'   -> "Xo0"
      3 - 1000     -> -997: c=27,x=-32 -> 27|32 -> 'k'; c=0,x=-1, more (x != 0) -> 'P'; c=31,x=-1 stop -> 'O' -> "kPO"
      2000 - 5     -> 1995: c=11,x=62 -> '['; c=30,x=1, bit4 set, more -> 'n'; c=1 -> '1'   -> "[n1"
      31           -> c=31,x=0, bit4 set and 0 != -1 -> more -> 'o'; then '0' (a positive value whose top group has bit 4 set
                      needs one more all-zero group so that the decoder does not sign-extend it)
      16           -> c=16 -> same guard -> "`0"
    """
    import json
    vecs = json.load(open(f"{golden_dir}/rle_vectors.json"))["vectors"]
    assert len(vecs) >= 7
    for v in vecs:
        m = _mask_from_runs(v["size"], v["runs_colmajor"])
        want = v["counts"].encode("ascii")
        assert rle._counts(m).tolist() == v["runs_colmajor"], v["name"]
        assert rle.encode_py(m)["counts"] == want, v["name"]                 # NumPy/Python restatement
        assert rle.encode(m)["counts"] == want, v["name"]                    # C helper in libzutis_hip.so
        assert rle.encode(m)["size"] == v["size"]
        assert np.array_equal(rle.decode({"size": v["size"], "counts": want}), m), v["name"]
        assert rle._from_string(want) == v["runs_colmajor"], v["name"]


def test_batched_rle_from_transitions_host_entry():
    """zh_rle_from_transitions_host (all kept masks' strings in one C call, from the device's transition positions) == the per-mask
    path == the mask encoder: random, empty, full, a rectangle, a mask with pixel 0 set; a mask over the position capacity is
    reported as None (the caller re-encodes it)."""
    import numpy as np
    from zutis_amd import rle
    rng = np.random.default_rng(0)
    H, W = 37, 53
    masks = [(rng.random((H, W)) > 0.5).astype(np.uint8), np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)]
    m = np.zeros((H, W), np.uint8); m[5:20, 10:30] = 1; masks.append(m)
    m = np.zeros((H, W), np.uint8); m[0, 0] = 1; masks.append(m)
    pos, nr = [], []
    for m in masks:
        f = m.reshape(-1, order="F")
        t = np.flatnonzero(f[1:] != f[:-1]) + 1
        pos.append(t); nr.append((len(t), int(f[0])))
    keep = max(1, max(len(t) for t in pos))
    P = np.zeros((len(masks), keep), np.int32)
    for i, t in enumerate(pos):
        P[i, :len(t)] = t
    NR = np.array(nr, np.int32)
    out = rle.rles_from_transitions(P, NR, H, W)
    for i, m in enumerate(masks):
        assert out[i] == rle.encode(m) == rle.rle_from_transitions(pos[i], nr[i][1], H, W), i
        assert (rle.decode(out[i]) == m).all()
    short = rle.rles_from_transitions(P[:, :3], NR, H, W)
    assert short[0] is None and short[1] == rle.encode(masks[1])
    # the packed list of zh_mask_runs_kept: every mask's min(transitions, max_runs) entries back to back
    for max_runs in (keep, 3):
        flat = np.concatenate([t[:max_runs] for t in pos]).astype(np.int32)
        got = rle.rles_from_transitions(flat, NR, H, W, packed_max_runs=max_runs)
        for i, m in enumerate(masks):
            assert got[i] == (rle.encode(m) if len(pos[i]) <= max_runs else None), (max_runs, i)


# ---- the host entry points (csrc/rle_host.hip) at exact capacity and one byte short, on the value list tools/host/rle_host_check.cpp
#      walks under the host sanitizers; the expected strings are the Python restatement's (rle._to_string)
GUARD = 0xA5


def _at_capacities(call, want, what):
    """call(address, cap) -> length: with room for exactly the string it is written and the byte behind it stays; one byte less: -1
    and the byte behind the shorter buffer stays."""
    n = len(want)
    for cap in ([n, n - 1] if n else [0]):
        buf = (ctypes.c_ubyte * (n + 1))(*([GUARD] * (n + 1)))
        got = call(ctypes.addressof(buf), cap)
        assert buf[cap] == GUARD and all(b == GUARD for b in buf[cap:]), (what, cap)
        if cap == n:
            assert got == n and bytes(buf[:n]) == want, (what, got)
        else:
            assert got == -1, (what, got)


def _host_masks(golden_dir):
    import json
    ms = [_mask_from_runs(v["size"], v["runs_colmajor"]) for v in json.load(open(f"{golden_dir}/rle_vectors.json"))["vectors"]]
    ms += [_mask_from_runs((16, 64), RC.seeded_runs(1024, nc, lead, seed=nc)) for nc in (2, 3, 4, 257) for lead in (0, 1)]
    return ms + [np.zeros((0, 5), np.uint8), np.zeros((3, 0), np.uint8)]


def test_worked_values_in_the_python_restatement():
    """The docstring examples of test_rle_hand_derived_format_vectors as (value, characters) pairs: a negative value is the delta
    counts[3] - counts[1]."""
    for v, chars in RC.WORKED:
        assert rle._to_string(np.array([v] if v >= 0 else [5, -v, 7, 0])) == (chars if v >= 0 else rle._to_string(np.array([5, -v, 7])) + chars)
        assert rle._from_string(chars) == [v]


def test_host_entry_points_at_exact_capacity_and_one_byte_short(golden_dir):
    """zh_rle_encode_host, zh_rle_counts_to_string_host and zh_rle_from_transitions_host (strided, packed, a row over the stride, n = 0)
    against rle._to_string: the string at exact capacity, -1 one byte short, the guard byte behind the buffer intact in both."""
    L = _lib.load(raw=True)
    for m in _host_masks(golden_dir):                                   # zh_rle_encode_host (an empty mask is the one run of length 0)
        h, w = m.shape
        mc = np.ascontiguousarray(m)
        want = rle._to_string(rle._counts(m)) if m.size else b"0"
        _at_capacities(lambda a, cap: L.zh_rle_encode_host(mc.ctypes.data, h, w, a, cap), want, ("encode", m.shape))
    for cl in RC.count_lists():                                         # zh_rle_counts_to_string_host
        c = np.asarray(cl, np.int64)
        _at_capacities(lambda a, cap: L.zh_rle_counts_to_string_host(c.ctypes.data, c.size, a, cap), rle._to_string(c), ("counts", cl))
    # zh_rle_from_transitions_host, strided and packed, one row over `stride` (an empty string, its entries skipped in the packed list)
    masks = [m for m in _host_masks(golden_dir) if m.shape == (16, 64)]
    tr = [RC.transitions(m) for m in masks]
    stride = sorted(len(t) for t, _ in tr)[-2]                          # the longest list does not fit
    assert sum(len(t) > stride for t, _ in tr) == 1
    nr = np.array([(len(t), f) for t, f in tr], np.int32)
    rows = np.zeros((len(masks), stride), np.int32)
    for i, (t, _) in enumerate(tr):
        rows[i, :min(len(t), stride)] = t[:stride]
    packed = np.concatenate([t[:stride] for t, _ in tr]).astype(np.int32)
    parts = [rle._to_string(rle._counts(m)) if len(t) <= stride else b"" for m, (t, _) in zip(masks, tr)]
    for pos, is_packed in ((rows, 0), (packed, 1)):
        off = np.full(len(masks) + 1, -1, np.int64)
        _at_capacities(lambda a, cap: L.zh_rle_from_transitions_host(pos.ctypes.data, stride, is_packed, nr.ctypes.data, len(masks), 1024, a, cap,
                                                                     off.ctypes.data), b"".join(parts), ("transitions", is_packed))
    # ... and the values that need a mask of up to 2^31 pixels: one transition at pixel 1 (run 1 = H*W - 1), and 1, v + 1, 1, 1 (delta -v)
    for v in RC.EDGES[:-1]:
        for t, hw, runs in (([1], v + 1, [1, v]), ([1, v + 2, v + 3], v + 4, [1, v + 1, 1, 1])):
            if min(runs) < 1:
                continue
            p, one = np.asarray(t, np.int32), np.array([[len(t), 0]], np.int32)
            off = np.zeros(2, np.int64)
            _at_capacities(lambda a, cap: L.zh_rle_from_transitions_host(p.ctypes.data, len(t), 0, one.ctypes.data, 1, hw, a, cap, off.ctypes.data),
                           rle._to_string(np.asarray(runs, np.int64)), ("transitions", v))
    assert L.zh_rle_from_transitions_host(None, 4, 1, None, 0, 1024, None, 0, np.zeros(1, np.int64).ctypes.data) == 0      # n = 0


def test_numpy_decoder_is_the_one_parser(golden_dir):
    """decode_np(r) == decode(r) and counts_np == _from_string on the same vectors; decode_np raises counts_np's two errors."""
    strings = [(m.shape, rle._to_string(rle._counts(m))) for m in _host_masks(golden_dir) if m.size]
    for shape, s in strings:
        r = {"size": list(shape), "counts": s}
        assert np.array_equal(rle.decode_np(r), rle.decode(r)) and rle.counts_np(s).tolist() == rle._from_string(s)
        assert np.array_equal(rle.decode_np({"size": list(shape), "counts": s.decode("ascii")}), rle.decode(r))
    for cl in RC.count_lists():
        s = rle._to_string(np.asarray(cl, np.int64))
        assert rle.counts_np(s).tolist() == rle._from_string(s) == cl
    assert not rle.decode_np({"size": [2, 3], "counts": b""}).any()
    with pytest.raises(ValueError, match="ends inside a value"):
        rle.decode_np({"size": [4, 4], "counts": b"51X"})               # 'X' = 40 + 48: bit 5 set, nothing follows
    with pytest.raises(ValueError, match="more than 12 characters"):
        rle.decode_np({"size": [4, 4], "counts": b"5" + b"P" * 12 + b"0"})


def test_host_capacity_helper_keeps_its_values():
    """rle._host_capacity: the three buffer sizes as they were (8 characters per value + 16; encode: 4 per pixel, capped at 6)."""
    assert rle._host_capacity(5) == 8 * 5 + 16 and rle._host_capacity(1024 + 2, 4) == 8 * (1024 + 2) // 2 + 16
