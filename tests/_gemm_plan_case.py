"""The deterministic case list that pins the GEMM dispatcher's plans (csrc/gemm_dispatch.h) to tests/golden/gemm_plans.json.

A case is the argument list of zh_dev_gemm_plan without the output array (FIELDS); pointers are made-up addresses: nothing is
dereferenced, only their alignment counts.  A group is (mode, forced tile code, tile_small): the overrides in force while its cases are
asked.  Shared by tools/gemm_plan_table.py and tests/test_gemm_plan_cpu.py.
"""
import collections

FIELDS = ("mode", "M", "N", "K", "batch", "lda", "ldw", "ldc", "strideC", "planeC", "ldr", "strideR", "res_rows", "out_kind", "act",
          "flags", "C", "bias", "residual", "has_pos")
Case = collections.namedtuple("Case", FIELDS)
MODES = {"f16": 0, "res16": 1, "x3": 2, "x2": 3}

# tile codes per mode (developer entry zh_dev_set_gemm_overrides, include/zutis_hip.h)
F16_CODES = (64, 128, 192, 256, 2064, 2128, 3064, 7032, 7096, 7128)
X3_CODES = (64, 96, 192, 256, 448, 512, 3064, 3066, 1288, 6464, 6496, 7096, 7128)
X2_CODES = (64, 96, 192, 256, 448, 512, 3064, 3066, 1288, 6464, 6496, 5122, 5124, 4484)
CODES = {"f16": F16_CODES, "res16": F16_CODES, "x3": X3_CODES, "x2": X2_CODES}
# ... plus the few-row kernel's code, a code of no mode, and a code of another mode only
FOREIGN = {"f16": 512, "res16": 448, "x3": 7032, "x2": 7128}
EXTRA = {m: (32, 777, FOREIGN[m]) for m in MODES}

ROWS = (1, 20, 32, 100, 128, 129, 442, 577, 1201, 1601, 3200, 4096, 4097, 14144, 56448, 147712, 257 * 256 - 37)
COLS = (1, 81, 96, 320, 512, 768, 1024, 1536, 2304, 3072, 4608)          # (L * D = 6 * 768 is the 4608 of the list)
KS = (64, 256, 768, 2048, 3072)
BATCHES = (1, 4, 12, 32)
# the rows / columns on which every epilogue layout is tried: few-row, ring, one-round, big-tile and peeled shapes
LAYOUT_ROWS = (20, 100, 129, 1201, 3200, 4097, 147712, 257 * 256 - 37)
LAYOUT_COLS = (81, 96, 768, 772, 1024, 4608)            # (772: rows of 2-byte elements that are 8- but not 16-byte multiples)
BASE_C, BASE_BIAS, BASE_RES = 0x7F0000000000, 0x7F1000000000, 0x7F2000000000


def groups():
    """[(mode name, forced code, tile_small)] in a fixed order."""
    return [(m, f, ts) for m in MODES for f in (0,) + CODES[m] + EXTRA[m] for ts in (0, 64)]


def _case(mode, M, N, K, batch, kind, *, ldc_pad=8, c_off=0, stride_pad=8, plane_pad=0, bias=None, res=None, res_off=0, ldr_pad=8,
          strider_pad=16, pos=False, flags=0, lda=None, ldw=None):
    """One case.  kind: 0 f32, 1 f16, 2 split; *_pad: elements added to the tight value; *_off: bytes added to the pointer;
    bias: None or a byte offset; res: None | 'periodic' | 'full'."""
    ldc = N + ldc_pad
    strideC = (M * ldc + stride_pad) if batch > 1 else 0
    planeC = ((batch * (M * ldc + stride_pad) + 31) // 8 * 8 + plane_pad) if kind == 2 else 0
    ldr = strideR = rows = 0
    if res:
        ldr = N + ldr_pad
        rows = 7 if res == "periodic" else M
        strideR = (rows * ldr + strider_pad) if (batch > 1 and res == "full") else 0
    return Case(MODES[mode], M, N, K, batch, (K + 8) if lda is None else lda, (K + 16) if ldw is None else ldw, ldc, strideC, planeC,
                ldr, strideR, rows, kind, 0, flags, BASE_C + c_off, 0 if bias is None else BASE_BIAS + bias,
                (BASE_RES + res_off) if res else 0, int(pos))


def _layouts(mode, kind):
    """Keyword sets of _case() that take an output of `kind` to the scalar, direct and wide store paths, one alignment rule at a time."""
    out = [dict(), dict(bias=0), dict(bias=4), dict(c_off=4), dict(c_off=8), dict(ldc_pad=4), dict(ldc_pad=5), dict(ldc_pad=0),
           dict(stride_pad=4), dict(stride_pad=3), dict(pos=True), dict(pos=True, bias=0)]
    if kind == 2:
        out += [dict(plane_pad=4), dict(plane_pad=4, ldc_pad=4)]
    if mode in ("x3", "x2"):
        out += [dict(flags=1), dict(flags=1, c_off=4)]
    for res in ("periodic", "full"):
        out += [dict(res=res), dict(res=res, res_off=8), dict(res=res, res_off=4), dict(res=res, ldr_pad=4), dict(res=res, ldr_pad=3),
                dict(res=res, strider_pad=4), dict(res=res, strider_pad=2), dict(res=res, pos=True), dict(res=res, bias=0, c_off=8)]
    return out


def _kinds(mode):
    return {"f16": (0, 1), "res16": (1,), "x3": (0, 1, 2), "x2": (0, 1, 2)}[mode]


def cases(mode, forced):
    """The cases of a group (the same for both tile_small values).  Every group: rows x columns x batches on aligned fp32 / fp16 rows,
    K cycling (it only matters to the 2^31 rule), the operand-size and grid-size edges; the unforced groups: every layout on
    LAYOUT_ROWS x LAYOUT_COLS x batch {1, 4}; the forced ones: a few layouts that change path, few-row choice or peel."""
    res = "full" if mode == "res16" else None           # zh_gemm_f16_res16 always has a residual
    out, i = [], 0
    for M in ROWS:
        for N in COLS:
            for batch in BATCHES:
                out.append(_case(mode, M, N, KS[i % len(KS)], batch, _kinds(mode)[i % len(_kinds(mode))], res=res))
                i += 1
    full = forced == 0
    for M in (LAYOUT_ROWS if full else (100, 3200, 257 * 256 - 37)):
        for N in (LAYOUT_COLS if full else (81, 768, 1024)):
            for batch in ((1, 4) if full else (1,)):
                for kind in _kinds(mode):
                    lays = _layouts(mode, kind) if full else [dict(c_off=8), dict(pos=True), dict(res="full"), dict(res="periodic"), dict(flags=1)]
                    for kw in lays:
                        if mode == "res16":
                            kw = dict(kw, res=kw.get("res") or "full")
                        if (kw.get("flags") and mode not in ("x3", "x2")) or (kw.get("pos") and (mode == "res16" or N % 4)):
                            continue                    # arguments the mode's entry does not have; pos tables need N % 4 == 0
                        out.append(_case(mode, M, N, KS[i % len(KS)], batch, kind, **kw))
                        i += 1
    # one batch item's A / W beyond 2^31 (not 2^32) elements: the two-slot tiles fall back; and a grid beyond 2^31 tiles of 64 x 64
    kind = _kinds(mode)[0]
    for M, N, lda, ldw in ((14144, 4608, 200000, 600000), (56448, 1024, 50000, 2400000)):
        out.append(_case(mode, M, N, 64, 1, kind, res=res, lda=lda))
        out.append(_case(mode, M, N, 64, 1, kind, res=res, ldw=ldw))
        out.append(_case(mode, M, N, 64, 1, kind, res=res, lda=lda // 2, ldw=ldw // 2))
    out.append(_case(mode, 1 << 30, 4608, 64, 32, kind, res=res, lda=0))
    # a surplus of under a quarter round (56 / 60 tiles) whose whole m-tile rows are more than one (4 rows of 24 / 18 tiles): no peel
    out += [_case(mode, M, 4608, 64, 1, kind, res=res) for M in (11515, 44539)]
    return out


# ---- canonical lines and digests
FAMILY, RING_PATH, SKINNY_PATH = ("ring", "skinny"), ("scalar", "direct", "wide"), ("scalar", "vec")
Plan = collections.namedtuple("Plan", "family code tile_m tile_n path peel")       # zh_dev_gemm_plan's int[6]


def peel_parts(c, M1):
    """The two calls of a peeled case: rows [0, M1) and [M1, M) — the pointer offsets of gemm_tail_peel, restated."""
    esz, rsz = (4 if c.out_kind == 0 else 2), (2 if c.mode == MODES["res16"] else 4)
    head = c._replace(M=M1, res_rows=c.res_rows if c.residual else 0)
    tail = c._replace(M=c.M - M1, C=c.C + M1 * c.ldc * esz, residual=(c.residual + M1 * c.ldr * rsz) if c.residual else 0,
                      res_rows=(c.res_rows - M1) if c.residual else 0)
    return head, tail


def _launch(p):
    return f"{FAMILY[p.family]} {p.code} {p.tile_m}x{p.tile_n} {(SKINNY_PATH if p.family else RING_PATH)[p.path]}"


def line(c, ask):
    """`M N K batch ... -> family code tile_m x tile_n path`, `-> peel M' ; first call ; second call`, or `-> error`.
    ask(case) -> Plan, or None for an argument error."""
    head = " ".join(f"{v:#x}" if k in ("C", "bias", "residual") else str(v) for k, v in zip(FIELDS, c))
    p = ask(c)
    if p is None:
        return head + " -> error"
    if not p.peel:
        return f"{head} -> {_launch(p)}"
    parts = [ask(s) for s in peel_parts(c, p.peel)]
    return f"{head} -> peel {p.peel} ; " + " ; ".join("error" if s is None else (_launch(s) + (f" peel {s.peel}" if s.peel else "")) for s in parts)


def digest(lines):
    import hashlib
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def library_ask(L):
    """ask() of line() through zh_dev_gemm_plan of the loaded library (the overrides in force are the caller's business)."""
    import ctypes
    out = (ctypes.c_int * 6)()

    def ask(c):
        return Plan(*out) if L.zh_dev_gemm_plan(*c, out) == 0 else None
    return ask


def group_lines(L, group):
    """The canonical lines of one group under its overrides (restored to none afterwards)."""
    mode, forced, tile_small = group
    if L.zh_dev_set_gemm_overrides(0, forced, tile_small) != 0:
        raise RuntimeError("zh_dev_set_gemm_overrides failed")
    try:
        ask = library_ask(L)
        return [line(c, ask) for c in cases(mode, forced)]
    finally:
        L.zh_dev_set_gemm_overrides(0, 0, 0)


def group_name(group):
    return "%s tile=%d tile_small=%d" % group


def ask_call(L, mode, M, N, K, *, out_kind, C, ldc, batch=1, lda=None, ldw=None, strideC=0, planeC=0, bias=0, residual=0, ldr=0, strideR=0,
             res_rows=0, act=0, flags=0, has_pos=False):
    """The plan of ONE call under the overrides in force, from the arguments a test is about to pass (pointers: data_ptr() values or 0).
    An argument error raises."""
    c = Case(MODES[mode], M, N, K, batch, K if lda is None else lda, K if ldw is None else ldw, ldc, strideC, planeC, ldr, strideR,
             res_rows, out_kind, act, flags, C, bias, residual, int(has_pos))
    p = library_ask(L)(c)
    if p is None:
        raise RuntimeError("zh_dev_gemm_plan: " + L.zh_last_error().decode("utf-8", "replace"))
    return p
