"""ctypes binding of libzutis_hip.so (include/zutis_hip.h).  Fails loudly: there is no CPU fallback."""
from __future__ import annotations

import collections
import ctypes as C
import functools
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZUTIS_HIP_LIB") or os.path.join(HERE, "libzutis_hip.so")   # override: developer A/B builds only
HEADER = os.path.join(os.path.dirname(HERE), "include", "zutis_hip.h")

_lib = None


class ZutisHipError(RuntimeError):
    pass


_CTYPES = {"int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "float": C.c_float, "double": C.c_double,
           "size_t": C.c_size_t, "zh_stream_t": C.c_void_p}
_DECL = re.compile(r"^[ \t]*([A-Za-z_][\w \t]*\*?)\s*\b(zh_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", re.M)

# One declaration of include/zutis_hip.h: C return type, [(C type, parameter name)], the ctypes forms of both, and whether a
# launch plan can replay it.
Entry = collections.namedtuple("Entry", "ret params restype argtypes plannable")


def _ctype(func: str, ctype: str, is_return: bool = False):
    if "*" in ctype:
        if not is_return:
            return C.c_void_p           # device and host pointers alike: callers pass addresses, ctypes arrays, byref() or None
        if ctype == "const char*":
            return C.c_char_p
    elif ctype in _CTYPES:
        return _CTYPES[ctype]
    raise ZutisHipError(f"{func}: no ctypes mapping for the C type {ctype!r} (zutis_amd/_lib.py _CTYPES)")


def parse_declarations(text: str) -> dict:
    """{name: Entry} for every zh_* function declared in `text` (the header), in declaration order.  Strict: a type outside
    _CTYPES, or a `zh_*(` outside comments that is not part of a declaration this parser reads, is an error."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in _DECL.finditer(text):
        ret, name = " ".join(m.group(1).split()), m.group(2)
        params = []
        for a in (" ".join(a.split()) for a in m.group(3).split(",")):
            if a in ("", "void"):
                continue
            t, _, n = a.rpartition(" ")
            while n.startswith("*"):
                t, n = t + "*", n[1:]
            if not (t and re.fullmatch(r"[A-Za-z_]\w*", n)):
                raise ZutisHipError(f"{name}: cannot read the parameter {a!r}")
            params.append((t, n))
        # plannable = device-pointer / scalar arguments only, stream last (zh_denormalize_u8 takes HOST float[3] pointers,
        # zh_pack_masks_u8 HOST pointer / count tables)
        plannable = (ret == "int" and bool(params) and params[-1][0] == "zh_stream_t" and not name.startswith("zh_plan_")
                     and name not in ("zh_denormalize_u8", "zh_pack_masks_u8"))
        out[name] = Entry(ret, params, _ctype(name, ret, True), [_ctype(name, t) for t, _ in params], plannable)
    unread = sorted(set(re.findall(r"\b(zh_[a-z0-9_]+)\s*\(", text)) - set(out))
    if unread:
        raise ZutisHipError(f"include/zutis_hip.h: declarations the binding parser cannot read: {unread}")
    return out


@functools.lru_cache(maxsize=None)
def _header_text() -> str:
    return open(HEADER).read()


@functools.lru_cache(maxsize=None)
def entries() -> dict:
    """parse_declarations() of include/zutis_hip.h: what load() binds and zutis_amd/plan.py builds its dispatcher from."""
    return parse_declarations(_header_text())


def declared_symbols():
    """Every function name declared in include/zutis_hip.h."""
    return sorted(entries())


def parse_constants(text: str) -> dict:
    """{name: int} for every `#define ZH_<NAME> <integer>` of `text` (the header) outside comments; a negative value stands in
    parentheses.  Strict like parse_declarations: a `#define ZH_...` whose value is not such an integer is an error."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(ZH_\w*)(.*)$", text, re.M):
        m = re.fullmatch(r"\s+(\d+|\(\s*-\s*\d+\s*\))\s*", value)
        if not m:
            raise ZutisHipError(f"include/zutis_hip.h: cannot read `#define {name}{value.rstrip()}` as an integer constant")
        out[name] = int(re.sub(r"[()\s]", "", m.group(1)))
    return out


@functools.lru_cache(maxsize=None)
def constants() -> dict:
    """parse_constants() of include/zutis_hip.h: the values the kernels were compiled with (csrc/common.h includes the same header),
    read by every Python module that names one."""
    return parse_constants(_header_text())


def header_abi_version() -> int:
    """ZH_ABI_VERSION of include/zutis_hip.h (the header travels with the package: bindings and library must agree on it)."""
    return constants()["ZH_ABI_VERSION"]


RECORDER = None   # zutis_amd.plan.Recorder while a launch plan is being recorded
COUNTER = None    # a dict while launches are being counted (bench.py: kernels per image): entry-point name -> calls


def _record(rec, name, fn, *args):
    rec.calls.append((name, args))
    return 0


def _count(counts, name, fn, *args):
    counts[name] = counts.get(name, 0) + 1
    return fn(*args)


class _Proxy:
    """Stands in for the CDLL while a plan is recorded or launches are counted: a plannable (= launching) entry point goes to
    on_call(sink, name, fn, args), everything else passes through.  One wrapper per name: __getattr__ only runs on a miss."""

    def __init__(self, lib, sink, on_call):
        self._lib, self._sink, self._on_call = lib, sink, on_call

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in entries() and entries()[name].plannable:
            fn = functools.partial(self._on_call, self._sink, name, fn)
        setattr(self, name, fn)
        return fn


_proxy = None     # the _Proxy of the RECORDER / COUNTER that was active at the last load()


def load(raw: bool = False):
    """Load the shared library (building nothing: run `python -m zutis_amd.build` / __graft_entry__.build())."""
    global _lib, _proxy
    if _lib is not None:
        if raw:
            return _lib
        sink, on_call = (RECORDER, _record) if RECORDER is not None else (COUNTER, _count)
        if sink is None:
            _proxy = None               # a finished recorder (and the tensors it keeps alive) is not held on to
            return _lib
        if _proxy is None or _proxy._sink is not sink:
            _proxy = _Proxy(_lib, sink, on_call)
        return _proxy
    if not os.path.exists(LIB_PATH):
        raise ZutisHipError(
            f"{LIB_PATH} is missing: the HIP extension is REQUIRED (no CPU fallback). "
            "Build it with `python -m zutis_amd.build`.")
    import torch  # noqa: F401  (first: the process must use ONE HIP runtime — the one torch loads; libzutis_hip binds to it)
    lib = C.CDLL(LIB_PATH)
    lib.zh_version.restype = C.c_int
    built, want = lib.zh_version(), header_abi_version()
    if built != want:       # a stale build: ctypes would pass the new argument lists to the old entry points
        raise ZutisHipError(f"{LIB_PATH} was built for ABI {built} but include/zutis_hip.h declares {want}: "
                            "rebuild it with `python -m zutis_amd.build`.")
    for name, e in entries().items():
        if not hasattr(lib, name):
            continue  # symbol check is test_capi's job; optional groups may be absent in partial builds
        fn = getattr(lib, name)
        fn.restype = e.restype
        fn.argtypes = e.argtypes
    _lib = lib
    return load(raw)


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().zh_last_error().decode("utf-8", "replace")
        raise ZutisHipError(f"{what} failed (rc={rc}): {msg}")
