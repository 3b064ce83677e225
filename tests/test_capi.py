"""CPU: the C-ABI library loads and exports every symbol include/zutis_hip.h declares (no compute calls)."""
import ctypes
import os

import pytest

from zutis_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)        # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_library_exports_every_declared_symbol(lib):
    syms = _lib.declared_symbols()
    assert len(syms) >= 18
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing


def test_every_declared_symbol_has_a_binding(lib):
    """Every `zh_...(` the header shows outside comments is an entry of the parse the bindings are derived from, and the loaded
    library's function carries argtypes with one item per declared parameter."""
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    seen = sorted(set(re.findall(r"\b(zh_[a-z0-9_]+)\s*\(", txt)))
    entries = _lib.entries()
    assert len(seen) >= 18 and not [s for s in seen if s not in entries]
    assert seen == _lib.declared_symbols()
    for s in seen:
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % s, txt).group(1).strip()
        n_params = 0 if decl in ("", "void") else decl.count(",") + 1
        argtypes = getattr(lib, s).argtypes
        assert argtypes is not None and len(argtypes) == n_params == len(entries[s].params), s


def test_header_types_map_to_ctypes(lib):
    """The C type -> ctypes map, pinned on declarations that between them use every C type of the header."""
    vp, i, l, f, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double
    want = {
        "zh_gemm_f16x3": (i, [vp, l, l, l, vp, l, l, l, vp, l, l, l, i, f, vp, vp, l, l, i, vp, vp, l, i, i, i,
                              i, i, i, i, i, i, vp]),                                  # pointers, long, int, float, stream
        "zh_topk_rows": (i, [vp, l, i, l, i, vp, ctypes.c_longlong, vp, vp, l, vp]),      # a long long scalar
        "zh_bilateral_workspace_size": (ctypes.c_size_t, [i, i, d, d, d]),              # size_t return, double
        "zh_mask_iou_counts": (i, [vp, i, l, vp, vp, vp, ctypes.c_size_t, vp]),         # size_t parameter
        "zh_last_error": (ctypes.c_char_p, []),                                         # const char* return, (void)
        "zh_rle_encode_host": (l, [vp, i, i, vp, l]),                                   # long return, char* parameter
        "zh_plan_run_multi": (i, [vp, vp, vp, i]),                                      # const void* const*, const zh_stream_t*
    }
    for name, (res, args) in want.items():
        e = _lib.entries()[name]
        assert (e.restype, e.argtypes) == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert _lib.entries()["zh_topk_rows"].params[6] == ("long long", "idx_add")


def test_unreadable_header_is_an_error():
    """Nothing is bound by default: an unknown C type, or a zh_ declaration in a shape the parser does not read, raises."""
    ok = "int zh_a(const float* x, long n, zh_stream_t stream);\nconst char* zh_b(void);\n"
    assert list(_lib.parse_declarations(ok)) == ["zh_a", "zh_b"] and _lib.parse_declarations(ok)["zh_a"].plannable
    with pytest.raises(_lib.ZutisHipError, match="zh_c.*short"):
        _lib.parse_declarations(ok + "int zh_c(short n, zh_stream_t stream);\n")
    with pytest.raises(_lib.ZutisHipError, match="zh_c.*float\\*"):
        _lib.parse_declarations(ok + "float* zh_c(int n);\n")
    with pytest.raises(_lib.ZutisHipError, match="zh_c"):
        _lib.parse_declarations(ok + "int zh_c(void (*callback)(int), zh_stream_t stream);\n")
    with pytest.raises(_lib.ZutisHipError, match="zh_c"):
        _lib.parse_declarations(ok + "int zh_c(int, zh_stream_t stream);\n")


def test_header_constants():
    """_lib.constants(): every `#define ZH_<NAME> <integer>` of the header, parenthesised negatives included; strict, and blind
    to comments."""
    c = _lib.constants()
    assert c["ZH_ERR_WORKSPACE"] == -3 and c["ZH_RCN_KMAX"] == 152 and c["ZH_PNG_SEGMENT_BYTES"] == 16384 and c["ZH_FILTER_BICUBIC"] == 3
    assert c["ZH_OK"] == 0 and c["ZH_ABI_VERSION"] == _lib.header_abi_version() and all(type(v) is int for v in c.values())
    ok = "#define ZH_A 7 /* seven */\n#define ZH_B (-2)\n  #  define ZH_C ( - 3 )\n#define OTHER foo\n"
    assert _lib.parse_constants(ok) == {"ZH_A": 7, "ZH_B": -2, "ZH_C": -3}
    for bad in ("#define ZH_X foo\n", "#define ZH_X\n", "#define ZH_X 1 + 2\n", "#define ZH_X(a) 3\n"):
        with pytest.raises(_lib.ZutisHipError, match="ZH_X"):
            _lib.parse_constants(ok + bad)
    assert _lib.parse_constants(ok + "/* #define ZH_X foo */\n/* text\n#define ZH_Y 5\n*/\n") == _lib.parse_constants(ok)


def test_kernel_sources_compile_against_the_header():
    """The header is the one definition on the C side too: csrc/common.h includes it and every source reaches common.h (so the
    compiler checks each entry point against its prototype), no file under csrc/ defines a name the header defines, and every
    extern "C" zh_* definition is a declared entry point."""
    import re
    csrc = build.CSRC
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    includes = {f: set(re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', t, re.M)) for f, t in text.items()}
    assert os.path.samefile(os.path.join(csrc, "../../include/zutis_hip.h"), _lib.HEADER)
    assert "../../include/zutis_hip.h" in includes["common.h"]

    def reaches_common(f, seen=()):
        return f == "common.h" or any(reaches_common(g, seen + (f,)) for g in includes.get(f, ()) if g not in seen)
    hips = [f for f in text if f.endswith(".hip")]
    assert sorted(hips) == sorted(build.SOURCES) and not [f for f in hips if not reaches_common(f)]
    for f, t in text.items():
        redefined = set(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", t, re.M)) & set(_lib.constants())
        assert not redefined, (f, sorted(redefined))
    defined = [n for t in text.values() for n in re.findall(r'extern\s+"C"\s+[^(){};]*?\b(zh_[a-z0-9_]+)\s*\(', t)]
    assert len(defined) >= 90 and len(set(defined)) == len(defined)
    assert not [n for n in defined if n not in _lib.entries()]


def test_depfile_reader_and_staleness(tmp_path):
    """build.read_depfile reads what the compiler's -MD -MF writes (continuation lines, `\\ ` for a space in a path); build.stale:
    an object is stale when it or its depfile is missing, or when a file the depfile names is newer or gone."""
    a, b, c = tmp_path / "a.hip", tmp_path / "dir with space" / "b.h", tmp_path / "c.h"
    b.parent.mkdir()
    for i, f in enumerate((a, b, c)):
        f.write_text("")
        os.utime(f, (1000 + i, 1000 + i))
    obj, dep = tmp_path / "a.o", tmp_path / "a.d"
    esc = lambda p: str(p).replace(" ", "\\ ")
    text = f"{esc(obj)}: {esc(a)} \\\n  {esc(b)} \\\n  {esc(c)}\n"
    assert build.stale(str(obj), str(dep))                       # neither exists
    dep.write_text(text)
    assert build.read_depfile(str(dep)) == [str(a), str(b), str(c)]
    assert build.stale(str(obj), str(dep))                       # no object
    obj.write_text("")
    os.utime(obj, (2000, 2000))
    assert not build.stale(str(obj), str(dep))
    os.utime(b, (2000, 2000))
    assert not build.stale(str(obj), str(dep))                   # as old as the object: not newer
    os.utime(b, (2001, 2001))
    assert build.stale(str(obj), str(dep))                       # the header behind the escaped space is newer
    os.utime(obj, (2002, 2002))
    assert not build.stale(str(obj), str(dep))
    c.unlink()
    assert build.stale(str(obj), str(dep))                       # a named file is gone
    dep.write_text(f"{esc(obj)}: {esc(a)}\n{esc(obj)}: {esc(b)}\n")          # one rule per compilation of the same source
    assert build.read_depfile(str(dep)) == [str(a), str(b)] and not build.stale(str(obj), str(dep))
    dep.unlink()
    assert build.stale(str(obj), str(dep))                       # no depfile


def test_version_arch_and_error_text(lib):
    assert lib.zh_version() == _lib.header_abi_version() >= 210        # a stale build is refused by _lib.load()
    assert lib.zh_arch() == b"gfx950"
    assert isinstance(lib.zh_last_error(), bytes)


def test_argument_validation_without_gpu(lib):
    # shape/alignment checks happen before any launch, so they are testable on CPU
    rc = lib.zh_gemm_f16(None, 0, 0, None, 0, 0, None, 0, 0, 0, None, None, 0, 0, 0, None, None, 0, 0, 0, 0, 0, 8, 8, 64, 1, None)
    assert rc == -1 and b"null" in lib.zh_last_error()
    rc = lib.zh_attention_f16(16, 8, 8, 16, 8, 8, 16, 8, 8, 16, 8, 8, 1, 1, 4, 4, 80, 1.0, 0, 0, 0, 0, None)
    assert rc == -1 and b"head_dim" in lib.zh_last_error()
    rc = lib.zh_attention_f16(16, 8, 8, 16, 8, 8, 16, 8, 8, 16, 8, 8, 1, 1, 4, 4, 64, 1.0, 64, 0, 64, 0, None)
    assert rc == -1 and b"all three or none" in lib.zh_last_error()
    # the reference-equivalent GEMM refuses plain fp16 operands (no silent precision downgrade)
    rc = lib.zh_gemm_f16x3(16, 64, 0, 0, 16, 64, 0, 0, 16, 8, 0, 0, 0, 1.0, None, None, 0, 0, 0, None, None, 0, 0, 0, 0, 0, 8, 8, 64, 1, 0, None)
    assert rc == -1 and b"A must be a split pair" in lib.zh_last_error()
    assert lib.zh_global_ln_l2_workspace_size(2, 1764, 512) == 2 * ((1764 * 512 + 4095) // 4096) * 16


def test_stale_library_is_refused(monkeypatch):
    """A library built for another ABI version must not be bound: ctypes would hand the new argument lists to old entry points."""
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "header_abi_version", lambda: 99999)
    with pytest.raises(_lib.ZutisHipError, match="built for ABI"):
        _lib.load()


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.ZutisHipError, match="REQUIRED"):
        _lib.load()


def test_ops_refuse_cpu_tensors(lib):
    import torch
    from zutis_amd import ops
    with pytest.raises(_lib.ZutisHipError):
        ops.gemm(torch.zeros(8, 64, dtype=torch.float16), torch.zeros(8, 64, dtype=torch.float16), torch.zeros(8, 8))


def test_launch_plan_dispatcher_matches_header_and_bindings(tmp_path, monkeypatch):
    """The native launch-plan dispatcher is generated from include/zutis_hip.h: every plannable entry point (stream last,
    device-pointer / scalar arguments) must be bound by ctypes with the same arity, the generated C must call it with
    one argument word per parameter, and the library must report the same op-id -> name mapping (no GPU needed)."""
    import struct
    from zutis_amd import _lib, plan
    ops_ = plan.parse_header()
    names = [n for n, _ in ops_]
    assert "zh_gemm_f16" in names and "zh_attention_f16" in names and "zh_bilateral_solve" in names
    assert not any(n.startswith("zh_plan_") for n in names) and "zh_denormalize_u8" not in names
    L = _lib.load(raw=True)
    for name, sig in ops_:
        assert len(getattr(L, name).argtypes) == len(sig) <= plan.MAX_ARGS + 1, name
        assert sig[-1][0] == "zh_stream_t"
    out = tmp_path / "gen.inc"
    assert plan.generate_dispatch(str(out)) == names
    txt = out.read_text()
    for i, (name, sig) in enumerate(ops_):
        line = [ln for ln in txt.splitlines() if ln.strip().startswith(f"case {i}:")][0]
        assert f"return {name}(" in line and line.count("c.a[") == len(sig) - 1
    for i, name in enumerate(names):
        assert L.zh_plan_op_name(i).decode() == name
    assert L.zh_plan_op_name(len(names)) is None
    # argument words: floats by bit pattern, pointers / ints zero-extended, None -> 0
    assert plan._word("float", 1.5) == struct.unpack("<I", struct.pack("<f", 1.5))[0]
    assert plan._word("double", -2.0) == struct.unpack("<Q", struct.pack("<d", -2.0))[0]
    assert plan._word("const float*", None) == 0 and plan._word("int", -1) == 0xFFFFFFFFFFFFFFFF
    # an entry point with more argument words than a plan command holds is refused when the dispatcher is generated
    monkeypatch.setattr(plan, "MAX_ARGS", max(len(sig) for _, sig in ops_) - 2)
    with pytest.raises(_lib.ZutisHipError, match="arguments before the stream"):
        plan.generate_dispatch(str(tmp_path / "too_wide.inc"))


def test_precision_site_sets():
    """Host logic (no kernels): named precisions and the closure of custom site sets."""
    from zutis_amd import engine as E
    assert E.resolve_precision("f16") == frozenset()
    assert E.resolve_precision("exact") == frozenset(E.ALL_SITES)
    assert E.resolve_precision("fast") == frozenset(E.HEAD_SITES)
    assert E.resolve_precision(["attn"]) == {"attn", "qkv"}
    assert E.resolve_precision(["mask"]) == {"mask", "ffn1"}
    with pytest.raises(E.ZutisHipError):
        E.resolve_precision("bf16")
    with pytest.raises(E.ZutisHipError):
        E.resolve_precision(["nope"])


def test_split_weight_packing_host_logic():
    """ops.split_weight (pack-time, plain torch — runs on CPU): W * 2^s with max|W| in [2^13, 2^14), hi + lo reproduces the
    scaled weight to ~2^-22 relative, lo is a NORMAL fp16 number wherever it is non-zero for typical weights, out_scale = 2^-s."""
    import math
    import torch
    from zutis_amd import ops
    g = torch.Generator().manual_seed(0)
    for scale in (0.03, 1.0, 1e-4, 300.0):
        w = torch.randn((64, 128), generator=g) * scale
        a = ops.split_weight(w)
        assert a.t.shape == (2, 64, 128) and a.plane == 64 * 128
        s = -math.log2(a.out_scale)
        assert s == int(s) and 2 ** 13 <= float(w.abs().max()) * 2 ** s < 2 ** 14
        rec = (a.t[0].double() + a.t[1].double()) * a.out_scale
        assert float(((rec - w.double()).abs() / w.double().abs().clamp_min(float(w.abs().max()) * 2 ** -10)).max()) < 2 ** -21
        lo = a.t[1].float().abs()
        assert float((lo[lo > 0] < 6.1e-5).float().mean()) < 0.02          # (almost) no subnormal lo halves
    z = ops.split_weight(torch.zeros((4, 64)))
    assert z.out_scale == 1.0 and float(z.t.abs().max()) == 0.0


def test_split_weight_one_plane_for_fp16_valued_weights_host_logic():
    """The f16x2 operand form (zh_gemm_f16x3 with planeW = 0): a weight whose values are fp16 numbers — what the reference's
    convert_weights leaves in the CLIP towers, clip_arch.py:566-587 — has an all-zero lo plane at ANY power-of-two scale, so it is
    packed as its hi plane alone, exactly; a single non-representable value brings the second plane back."""
    import torch
    from zutis_amd import ops
    g = torch.Generator().manual_seed(1)
    for scale in (0.03, 1.0, 2e-4, 300.0):
        w = (torch.randn((48, 64), generator=g) * scale).to(torch.float16).to(torch.float32)      # includes fp16 subnormals at 2e-4
        a = ops.split_weight(w)
        assert a.x2 and a.plane == 0 and a.t.shape == (1, 48, 64)
        assert torch.equal(a.hi.to(torch.float64) * a.out_scale, w.to(torch.float64))
        assert a.view(a.hi[:16]).x2                                                              # row slices keep the marker
        b = ops.split_weight(w, allow_x2=False)
        assert (not b.x2) and b.t.shape == (2, 48, 64) and not bool(b.t[1].any()) and torch.equal(b.t[0], a.hi)
        w2 = w.clone()
        w2[3, 5] = w2[3, 5] * (1.0 + 2.0 ** -14) + (2.0 ** -30 if w2[3, 5] == 0 else 0.0)          # not an fp16 number any more
        c = ops.split_weight(w2)
        assert (not c.x2) and c.plane != 0 and int((c.t[1] != 0).sum()) == 1
    ops.ALLOW_X2 = False
    try:
        assert not ops.split_weight(torch.ones((4, 64))).x2
    finally:
        ops.ALLOW_X2 = True
