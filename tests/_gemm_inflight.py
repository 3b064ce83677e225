"""What the GEMM tile chooser decides for the GEMM calls of a recorded launch plan at a given number of launches in flight
(zh_dev_gemm_plan_inflight).  Shared by tests/test_gemm_inflight_gpu.py and tools/gemm_inflight_ab.py --flips.

A recorded call is (entry name, argument tuple) as zutis_amd.plan.Recorder keeps it: the very arguments of the C entry."""
import ctypes

from tests import _gemm_plan_case as PC

# argument names of the three GEMM entries, in the order of include/zutis_hip.h (the stream last)
_X3 = ("A lda strideA planeA W ldw strideW planeW C ldc strideC planeC out_kind out_scale bias residual ldr strideR res_rows "
       "pos_y pos_x ld_pos pos_h pos_w pos_f16 act M N K batch flags stream").split()
_F16 = ("A lda strideA W ldw strideW C ldc strideC out_f16 bias residual ldr strideR res_rows "
        "pos_y pos_x ld_pos pos_h pos_w pos_f16 act M N K batch stream").split()
_RES16 = "A lda strideA W ldw strideW C ldc strideC bias residual ldr strideR res_rows M N K batch stream".split()


def case_of(name, args):
    """The zh_dev_gemm_plan case (tests/_gemm_plan_case.Case) of one recorded GEMM call, None for any other entry."""
    names = {"zh_gemm_f16x3": _X3, "zh_gemm_f16": _F16, "zh_gemm_f16_res16": _RES16}.get(name)
    if names is None:
        return None
    assert len(names) == len(args), (name, len(args))
    a = dict(zip(names, args))
    if name == "zh_gemm_f16x3":
        mode, kind = (PC.MODES["x3"] if a["planeW"] else PC.MODES["x2"]), a["out_kind"]
    elif name == "zh_gemm_f16":
        mode, kind = PC.MODES["f16"], a["out_f16"]
    else:
        mode, kind = PC.MODES["res16"], 1
    return PC.Case(mode, a["M"], a["N"], a["K"], a["batch"], a["lda"], a["ldw"], a["ldc"], a["strideC"], a.get("planeC", 0), a["ldr"], a["strideR"],
                   a["res_rows"], kind, a.get("act", 0), a.get("flags", 0), a["C"] or 0, a["bias"] or 0, a["residual"] or 0, int(bool(a.get("pos_y"))))


def plan_at(L, case, inflight):
    """The Plan of a case at `inflight` launches in flight under the overrides in force; an argument error raises."""
    out = (ctypes.c_int * 6)()
    if L.zh_dev_gemm_plan_inflight(*case, inflight, out) != 0:
        raise RuntimeError("zh_dev_gemm_plan_inflight: " + L.zh_last_error().decode("utf-8", "replace"))
    return PC.Plan(*out)


def flips(L, calls, inflight):
    """[(case, plan at 1, plan at `inflight`)] for the recorded GEMM calls whose plan differs between the two."""
    out = []
    for name, args in calls:
        c = case_of(name, args)
        if c is not None:
            p1, pn = plan_at(L, c, 1), plan_at(L, c, inflight)
            if p1 != pn:
                out.append((c, p1, pn))
    return out
