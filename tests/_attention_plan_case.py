"""The case list that pins the attention launcher's plan (csrc/attention_dispatch.h, asked through zh_dev_attention_plan), and the
arithmetic the plan is held to, stated here independently of the header (tests/test_attention_plan_cpu.py).

A case is (batch, heads, Tq, Tk, dh, x3, causal, ksplit).  ask() describes it to the library as ops.attention would: contiguous
[batch, T, heads * dh] operands, the lo planes of a split pair one tensor further on.  Pointers are made-up addresses: nothing is
dereferenced, no GPU is needed."""
import collections
import ctypes

from zutis_amd import shape_rules as SR

Case = collections.namedtuple("Case", "batch heads Tq Tk dh x3 causal ksplit")
Plan = collections.namedtuple("Plan", "variant key_tile nqb items grid pipe ksplit kchunk workspace_bytes combine_grid")   # zh_dev_attention_plan's int[10]
F16, X3, X3_PIPE = 0, 1, 2                       # Plan.variant
BATCHES = (1, 2, 4, 8, 32)
SELF_ATTENTION = ((50, 12, 64), (442, 12, 64), (1201, 12, 64), (577, 16, 64), (5505, 6, 64), (100, 8, 96))   # (T, heads, dh); the last: the decoder's
CROSS_ATTENTION = ((100, 1764, 8, 96), (100, 4800, 8, 96), (20, 5504, 6, 64))                                # (Q, M, heads, dh)
CROSS_SETTINGS = (1, 8, 12, "auto")              # the engines' default, SelfMask's, the ZUTIS drop-in's, bench.py's config 4
CAUSAL = ((77, 8, 64),)
EDGE_TQ, EDGE_TK = (1, 127, 128, 129), (1, 31, 32, 33, 63, 64, 65)
# workgroup counts whose grid (rounded up to 8) is 512 / 520, 768 / 776, 1024 / 1032: whether the dh = 64 split-pair kernel is the pipelined one
GRID_EDGES = {505: True, 512: True, 513: False, 520: False, 761: False, 768: False, 769: True, 776: True,
              1017: True, 1024: True, 1025: False, 1032: False}


def product_cases():
    """The product's shapes at every batch, fp16 and split pairs, each with the key split shape_rules gives it."""
    out = []
    for B in BATCHES:
        for x3 in (False, True):
            for T, heads, dh in SELF_ATTENTION:
                out.append(Case(B, heads, T, T, dh, x3, False, SR.self_attention_key_split(B, T, heads, dh, x3, False)))
            for Q, M, heads, dh in CROSS_ATTENTION:
                for S in sorted({SR.cross_attention_key_split(s, B, heads, Q, M, x3) for s in CROSS_SETTINGS}):
                    out.append(Case(B, heads, Q, M, dh, x3, False, S))
            for T, heads, dh in CAUSAL:
                out.append(Case(B, heads, T, T, dh, x3, True, SR.self_attention_key_split(B, T, heads, dh, x3, True)))
    return out


def edge_cases():
    out = [Case(2, 3, Tq, Tk, dh, x3, False, 1) for dh in (64, 96) for x3 in (False, True) for Tq in EDGE_TQ for Tk in EDGE_TK]
    out += [Case(2, 3, T, T, 64, x3, True, 1) for x3 in (False, True) for T in EDGE_TQ]
    out += [Case(n, 1, 5, 40, dh, x3, False, 1) for n in GRID_EDGES for dh, x3 in ((64, True), (64, False), (96, True))]
    out += [Case(n // 4, 1, 5, 200, 64, True, False, 4) for n in GRID_EDGES if n % 4 == 0]       # the same grids through a key split
    return out


def sweep():
    return product_cases() + edge_cases()


def model(c: Case) -> Plan:
    """What the launcher must plan for an accepted case: the grid, chunk and workspace arithmetic in ten lines."""
    kt, S = (32 if c.x3 else 64), max(1, c.ksplit)
    nqb = -(-c.Tq // 128)
    items = c.batch * c.heads * nqb * S
    grid = -(-items // 8) * 8
    pipe = c.x3 and (c.dh == 96 or -(-grid // 512) <= -(-grid // 768))
    if S == 1:
        return Plan(X3_PIPE if pipe else X3 if c.x3 else F16, kt, nqb, items, grid, int(pipe), 1, 0, 0, 0)
    rows = S * c.batch * c.heads * c.Tq                                  # partial rows: dh floats of O, one running max, one row sum
    return Plan(X3_PIPE if pipe else X3 if c.x3 else F16, kt, nqb, items, grid, int(pipe), S, -(-(-(-c.Tk // kt)) // S) * kt,
                rows * (c.dh + 2) * 4, -(-(c.batch * c.Tq * c.heads * c.dh // 4) // 256))


PTR = 1 << 24                                    # a made-up 16-byte aligned device address


def arguments(lib, c: Case, workspace_bytes=None):
    """zh_attention_f16_splitk's argument list for `c` up to workspace_bytes (no stream), with the causal flag: what
    zh_dev_attention_plan takes before `plan`.  workspace_bytes None: exactly what zh_attention_splitk_workspace_size asks."""
    D = c.heads * c.dh
    lo_q, lo_k = (c.batch * c.Tq * D, c.batch * c.Tk * D) if c.x3 else (0, 0)
    split = c.ksplit > 1
    if workspace_bytes is None:
        workspace_bytes = lib.zh_attention_splitk_workspace_size(c.batch, c.heads, c.Tq, c.dh, c.ksplit) if split else 0
    return (PTR, D, c.Tq * D, 2 * PTR, D, c.Tk * D, 3 * PTR, D, c.Tk * D, 4 * PTR, D, c.Tq * D, c.batch, c.heads, c.Tq, c.Tk, c.dh,
            int(c.causal), lo_q, lo_k, lo_k, 0, c.ksplit, 5 * PTR if split else None, workspace_bytes)


def ask(lib, c: Case = None, workspace_bytes=None, **fields):
    """The library's plan for `c` (or for Case(**fields) over a 1-image, 1-head, dh = 64, fp16, unsplit default); None: an argument
    error, its text in zh_last_error()."""
    if c is None:
        c = Case(**{**dict(batch=1, heads=1, dh=64, x3=False, causal=False, ksplit=1), **fields})
    out = (ctypes.c_int * len(Plan._fields))()
    return Plan(*out) if lib.zh_dev_attention_plan(*arguments(lib, c, workspace_bytes), out) == 0 else None
