"""Launch traces: the sequence of C-ABI calls an engine's forward makes, in a form that can be compared across commits.

trace(fn) runs fn under zutis_amd.plan.Recorder (nothing is launched: a trace cannot fault and costs allocation and Python only)
and returns one canonical line per recorded call: the entry name and its arguments, typed by include/zutis_hip.h —
  the stream is dropped; a float / double is its float.hex(); an integer is itself; a null pointer is 0; any other pointer is
  (k, byte offset) with k = the first-appearance index, in this trace, of the storage the pointer lies in.
So a trace holds every shape decision (which kernel, which split, which strides) and every buffer alias, and no address.

The engines' forwards read nothing back from the device, so a trace does not depend on data (inputs are zeros).  CASES are the
smallest shapes on both sides of every rule of zutis_amd/shape_rules.py; tools/launch_trace.py writes / checks / shows them and
tests/test_launch_trace_gpu.py holds them to tests/golden/launch_traces.json."""
import functools
import hashlib

import torch

from zutis_amd import _lib, detgen, plan


def canonical(calls, keepalive):
    """[(entry, args)] of a Recorder + its keepalive tensors -> [canonical line]."""
    base_of = {}
    for t in keepalive:
        if t.data_ptr():
            base_of[t.data_ptr()] = t.untyped_storage().data_ptr()
    order, lines = {}, []
    entries = _lib.entries()
    for name, args in calls:
        params = entries[name].params
        assert len(args) == len(params) and params[-1][0] == "zh_stream_t", name
        words = []
        for (ctype, pname), v in zip(params[:-1], args[:-1]):
            if "*" in ctype:
                if not v:
                    words.append("0")
                    continue
                if v not in base_of:
                    raise AssertionError(f"{name}: pointer argument {pname} was not recorded through ops._p")
                base = base_of[v]
                words.append(f"({order.setdefault(base, len(order))},{v - base})")
            elif ctype in ("float", "double"):
                words.append(float(v).hex())
            else:
                words.append(str(0 if v is None else int(v)))
        lines.append(name + " " + " ".join(words))
    return lines


def trace(fn):
    with plan.Recorder() as rec:
        fn()
    return canonical(rec.calls, rec.keepalive)


def digests(lines):
    """What the golden file keeps per call: `entry:first 12 hex digits of sha256(canonical line)`."""
    return [ln.split(" ", 1)[0] + ":" + hashlib.sha256(ln.encode()).hexdigest()[:12] for ln in lines]


@functools.lru_cache(maxsize=None)
def _weights(kind):
    sd = {"tiny": lambda: detgen.zutis_state_dict(detgen.TINY), "b16": lambda: detgen.zutis_state_dict(detgen.VIT_B16),
          "selfmask": detgen.selfmask_state_dict, "text": lambda: detgen.clip_text_state_dict(detgen.TEXT_TINY),
          "clip": lambda: {k: v for k, v in detgen.clip_full_state_dict(detgen.VIT_B32).items() if k.startswith("visual.")}}[kind]()
    return {k: torch.from_numpy(v).to("cuda:0") for k, v in sd.items()}


def _twice(make_engine, call, make_input):
    """A fresh engine, two consecutive calls: the first also records the geometry tables and the decoder's cached layer-0 block."""
    def run():
        eng, x = make_engine(), make_input()
        call(eng, x)
        call(eng, x)
    return run


def _zeros(B, H, W):
    return lambda: torch.zeros((B, 3, H, W), dtype=torch.float32, device="cuda:0")


def _zutis(kind, cfg, B, H, W, precision, cross_ksplit=None):
    from zutis_amd.engine import ZutisEngine

    def make():
        eng = ZutisEngine(_weights(kind), cfg.patch, cfg.dec_heads, precision=precision)
        if cross_ksplit is not None:
            eng.cross_ksplit = cross_ksplit
        return eng
    return _twice(make, lambda e, x: e.forward(x), _zeros(B, H, W))


def _selfmask(B, precision):
    from zutis_amd.engine import SelfMaskEngine
    return _twice(lambda: SelfMaskEngine(_weights("selfmask"), precision=precision), lambda e, x: e.forward(x), _zeros(B, 512, 683))


def _clip(precision):
    from zutis_amd.engine import ClipImageEncoder
    return _twice(lambda: ClipImageEncoder(_weights("clip"), detgen.VIT_B32.patch, precision=precision), lambda e, x: e.encode_image(x),
                  _zeros(4, 224, 224))


def _text():
    from zutis_amd.engine import ClipTextEncoder
    return _twice(lambda: ClipTextEncoder(_weights("text"), precision="exact"), lambda e, t: e.encode_text(t),
                  lambda: torch.from_numpy(detgen.text_tokens(5, detgen.TEXT_TINY)).to("cuda:0"))


CASES = {}
for _p in ("exact", "fast", "f16"):
    for _B in (1, 2):
        CASES[f"zutis_tiny_64x80_b{_B}_{_p}"] = _zutis("tiny", detgen.TINY, _B, 64, 80, _p)
CASES["zutis_b16_480x640_b1_exact_ksplit12"] = _zutis("b16", detgen.VIT_B16, 1, 480, 640, "exact", 12)
CASES["zutis_b16_336x336_b2_exact_ksplit1"] = _zutis("b16", detgen.VIT_B16, 2, 336, 336, "exact", 1)
CASES["zutis_b16_336x336_b8_exact_auto"] = _zutis("b16", detgen.VIT_B16, 8, 336, 336, "exact", "auto")
CASES["zutis_b16_336x336_b1_fast"] = _zutis("b16", detgen.VIT_B16, 1, 336, 336, "fast")
for _B in (1, 2, 4, 8):
    CASES[f"selfmask_512x683_b{_B}_exact"] = _selfmask(_B, "exact")
CASES["selfmask_512x683_b1_f16"] = _selfmask(1, "f16")
CASES["clip_b32_224x224_b4_exact"] = _clip("exact")
CASES["clip_b32_224x224_b4_half"] = _clip("half")
CASES["text_tiny_5_exact"] = _text()


def run_case(name):
    """The canonical lines of CASES[name]."""
    return trace(CASES[name])
