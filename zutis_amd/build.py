"""Builds zutis_amd/libzutis_hip.so (all HIP kernels, gfx950) with hipcc.  In-tree, no torch types.

    python -m zutis_amd.build [--force]
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libzutis_hip.so")
# float64 bilateral solver: no FMA contraction (bin edges and bistochastisation are bit-compared with NumPy/SciPy);
# preprocess.hip: Pillow's resampling coefficients are bit-compared with the host's double arithmetic
EXTRA_FLAGS = {"bilateral.hip": ["-ffp-contract=off"], "preprocess.hip": ["-ffp-contract=off"],
               "synth.hip": ["-ffp-contract=off"],   # synth.hip: Pillow's blend and HSV arithmetic, one IEEE operation at a time
               "polygon.hip": ["-ffp-contract=off"]}  # polygon.hip: rleFrPoly's double arithmetic, bit-compared with the host's
# the MFMA kernels live at the register budget of their occupancy: a spill is a 2-3x slowdown, so it is a build error
# (norm.hip: the row kernels keep a whole row in registers between the two moments and are launched more often than anything but the GEMMs)
NO_SCRATCH = {"gemm.hip", "gemm_x3.hip", "attention.hip", "norm.hip", "preprocess.hip", "synth.hip", "resample.hip", "label_paint.hip", "png.hip", "jpeg_enc.hip"}
MAX_SCRATCH = int(os.environ.get("ZH_BUILD_MAX_SCRATCH", "0"))    # bytes per lane tolerated: the MFMA loops must not spill (developer builds may raise it)
# waves per SIMD the design of a kernel relies on (source -> mangled-name substring -> minimum), checked against the compiler's
# remarks; a key that matches no kernel of its source is a build error (a renamed template would otherwise drop its guard)
MIN_OCCUPANCY = {"attention.hip": {"attn_f16_kernelILi64ELi4ELi1ELi0EE": 3, "attn_f16_kernelILi64ELi4ELi0ELi0EE": 3,
                                   "attn_f16_kernelILi64ELi4ELi1ELi1EE": 2, "attn_f16_kernelILi96ELi4ELi1ELi0EE": 2,
                                   "attn_f16_kernelILi96ELi4ELi0ELi0EE": 2, "attn_f16_kernelILi96ELi4ELi1ELi1EE": 2,
                                   # dh = 128 (ViT-L decoder): fp16 and the plain split-pair loop, two workgroups of 75 776 LDS bytes per CU
                                   "attn_f16_kernelILi128ELi4ELi0ELi0EE": 2, "attn_f16_kernelILi128ELi4ELi1ELi0EE": 2},
                 # the byte epilogue (zh_upsample_argmax_bytes) must not cost the arg-max kernels the occupancy of their int64 form (UaStore)
                 "resample.hip": {"upsample_argmax_pk_kernelI7UaBytes": 3, "upsample_argmax_lds_kernelI7UaBytes": 6,
                                  "upsample_argmax_kernelI7UaBytes": 8},
                 # the HBM-bound row kernels hide their load latency by occupancy; the split-K forms hold NPARTS planes of the row at once
                 # (one plane fits 8 waves only while its four loads are issued back to back: 59 VGPRs of the 64 that 8 waves allow)
                 "norm.hip": {"layernorm_kernelI6RowF32E": 8, "layernorm_kernelI6RowF16E": 8,
                              "sum_layernorm_kernelILi0EE": 8, "sum_layernorm_kernelILi1EE": 8, "sum_layernorm_kernelILi2EE": 6,
                              "sum_layernorm_kernelILi4EE": 4, "assemble_ln_kernelIfE": 8, "assemble_ln_kernelIDF16_E": 8,
                              "l2norm_rows_kernel": 8, "gln_partial_kernel": 8, "gln_apply_kernel": 8}}
SOURCES = ["capi.hip", "rle_host.hip", "gemm.hip", "gemm_x3.hip", "attention.hip", "norm.hip", "resample.hip", "metrics.hip", "instance.hip", "mask_rle.hip", "instance_paint.hip", "bilateral.hip", "components.hip", "preprocess.hip", "retrieval.hip", "text.hip", "criterion.hip", "assign.hip", "cocoeval.hip", "polygon.hip", "label_paint.hip", "png.hip", "jpeg_host.hip", "jpeg.hip", "jpeg_enc.hip", "synth.hip", "plan.hip"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def sources():
    return [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]


def _obj(src: str) -> str:
    return os.path.join(HERE, "_obj", os.path.basename(src)[:-4] + ".o")


def read_depfile(path: str) -> list:
    """The prerequisites a compiler-written depfile (-MD -MF) names: `target: dep dep \\<newline> dep`, a space inside a path
    written `\\ `.  It lists the source and every file the translation unit read."""
    deps = []
    for rule in open(path).read().replace("\\\n", " ").splitlines():
        m = re.match(r"(?:\\ |\S)+?:(?:\s|$)", rule)
        if m:
            deps += [d.replace("\\ ", " ") for d in re.findall(r"(?:\\ |\S)+", rule[m.end():])]
    return deps


def stale(obj: str, depfile: str) -> bool:
    """An object is stale when it or its depfile is missing, or when a file the depfile names is newer (or gone)."""
    if not (os.path.exists(obj) and os.path.exists(depfile)):
        return True
    t = os.path.getmtime(obj)
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in read_depfile(depfile))


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    objs = [_obj(s) for s in sources()]
    return any(stale(o, o[:-2] + ".d") for o in objs) or any(os.path.getmtime(o) > os.path.getmtime(LIB) for o in objs)


def build(force: bool = False, verbose: bool = True) -> str:
    if not force and not needs_build():
        return LIB
    objs = []
    os.makedirs(os.path.join(HERE, "_obj"), exist_ok=True)
    from . import plan
    plan.generate_dispatch(os.path.join(CSRC, "plan_gen.inc"))      # launch-plan dispatcher, generated from the header (rewritten only when its text changes)
    procs = []
    for src in sources():
        obj = _obj(src)
        dep = obj[:-2] + ".d"
        objs.append(obj)
        if not force and not stale(obj, dep):
            continue
        cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17"] + EXTRA_FLAGS.get(os.path.basename(src), []) + \
              ["-MD", "-MF", dep, "-c", src, "-o", obj]
        if os.path.basename(src) in NO_SCRATCH:
            cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((cmd, src, subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True)))
    for cmd, src, p in procs:
        _, err = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(err)
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
        if os.path.basename(src) in NO_SCRATCH:
            spills = [ln for ln in err.splitlines() if "ScratchSize [bytes/lane]:" in ln
                      and int(ln.split("ScratchSize [bytes/lane]:")[1].split()[0]) > MAX_SCRATCH]
            if spills:
                raise RuntimeError(f"{os.path.basename(src)}: a kernel spills to scratch (register budget exceeded): {spills[0].strip()}")
            fn = None
            min_occ = MIN_OCCUPANCY.get(os.path.basename(src), {})
            matched = set()
            for ln in err.splitlines():
                if "Function Name:" in ln:
                    fn = ln.split("Function Name:")[1].split()[0]
                elif "Occupancy [waves/SIMD]:" in ln and fn:
                    occ = int(ln.split("Occupancy [waves/SIMD]:")[1].split()[0])
                    for key, need in min_occ.items():
                        if key in fn:
                            matched.add(key)
                            if occ < need:
                                raise RuntimeError(f"{os.path.basename(src)}: {fn} compiles to {occ} waves/SIMD, its design needs {need}")
            unmatched = sorted(set(min_occ) - matched)
            if unmatched:
                raise RuntimeError(f"{os.path.basename(src)}: MIN_OCCUPANCY names no kernel of the compiler's remarks: {', '.join(unmatched)}")
        else:
            sys.stderr.write(err)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
