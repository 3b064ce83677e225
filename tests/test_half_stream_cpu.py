"""Precision "half" (fp16 residual stream of ClipImageEncoder), the parts that need no GPU: the new fixture is pinned to the oracle,
the yardstick (the reference's own half-precision run) has teeth, the mode's rounding points restated in fp32 compute stay inside
the acceptance envelope, and the name resolves for ClipImageEncoder only."""
import numpy as np
import pytest
import torch

from tests import _half_stream_case as HC
from oracle import zutis_ref as O
from zutis_amd import detgen
from zutis_amd import engine as E
from zutis_amd._lib import ZutisHipError

TAGS = list(HC.CASES)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(f"{golden_dir}/encode_image_half.npz")


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_f32_is_the_oracle(gold, tag):
    """`{tag}_f32` (the reference's VisionTransformer in fp32 on the fp16-valued weights) against O.clip_encode_image, at the bound of
    tests/test_oracle_golden.py::test_oracle_encode_image_matches_reference."""
    cfg, sd, x = HC.case(tag)
    assert [int(v) for v in gold[f"{tag}_shape"]] == [x.shape[0], cfg.patch * cfg.grid, cfg.width, cfg.layers, cfg.patch, cfg.grid, cfg.embed_dim]
    with torch.no_grad():
        e = O.clip_encode_image(O.to_torch_params(sd), x, cfg.patch).numpy()
    ref = gold[f"{tag}_f32"]
    assert e.shape == ref.shape
    assert np.abs(e - ref).max() < 5e-7, np.abs(e - ref).max()


@pytest.mark.parametrize("tag", TAGS)
def test_yardstick_has_teeth(gold, tag):
    """The reference's half run differs from its fp32 run, and by less than the north-star tolerance."""
    e_ref = float(np.abs(gold[f"{tag}_ref_half"].astype(np.float64) - gold[f"{tag}_f32"]).max())
    print(f"{tag}: max |ref_half - f32| = {e_ref:.3e}")
    assert 0 < e_ref < 1e-3, e_ref
    assert gold[f"{tag}_ref_half"].dtype == np.float32 and np.abs(np.linalg.norm(gold[f"{tag}_f32"], axis=1) - 1).max() < 1e-5


@pytest.mark.parametrize("two_roundings", [True, False], ids=["two_roundings", "one_rounding"])
@pytest.mark.parametrize("tag", TAGS)
def test_restated_rounding_points_stay_inside_the_envelope(gold, tag, two_roundings):
    """The specification of the mode (tests/_half_stream_case.py::restate_half: fp32 compute, explicit roundings through fp16), in
    both admissible forms of the residual update, inside the envelope the GPU test holds the engine to."""
    cfg, sd, x = HC.case(tag)
    with torch.no_grad():
        got = HC.restate_half(sd, x, cfg.patch, two_roundings=two_roundings).numpy()
    HC.check_envelope(tag, got, gold)


def _cpu_visual(tag="small"):
    cfg, sd, _ = HC.case(tag)
    return cfg, HC.visual_params(sd, "cpu")


def test_clip_image_encoder_takes_the_name():
    cfg, P = _cpu_visual()
    enc = E.ClipImageEncoder(P, cfg.patch, prefix="visual.", precision="half")
    assert enc.precision == "half" and enc.half_stream is True
    assert enc.x3_sites == E.resolve_precision("fast")           # the contraction sites of `fast` ...
    for other in ("exact", "fast", "f16"):                       # ... and no other name carries the stream flag
        assert E.ClipImageEncoder(P, cfg.patch, prefix="visual.", precision=other).half_stream is False
    assert E.ClipImageEncoder(P, cfg.patch, prefix="visual.").precision == "exact"


def test_the_name_is_refused_everywhere_else():
    with pytest.raises(ZutisHipError, match="ClipImageEncoder only"):
        E.resolve_precision("half")
    assert E.resolve_precision("half", allow_half=True) == frozenset(E.HEAD_SITES)
    zsd = {k: torch.from_numpy(v) for k, v in detgen.zutis_state_dict(detgen.TINY).items()}
    with pytest.raises(ZutisHipError, match="fp32"):
        E.ZutisEngine(zsd, detgen.TINY.patch, detgen.TINY.dec_heads, precision="half")
    ssd = {k: torch.from_numpy(v) for k, v in detgen.selfmask_state_dict().items()}
    with pytest.raises(ZutisHipError, match="fp32"):
        E.SelfMaskEngine(ssd, precision="half")
    tsd = {k: torch.from_numpy(v) for k, v in detgen.clip_text_state_dict(detgen.TEXT_TINY).items()}
    with pytest.raises(ZutisHipError, match="fp32"):
        E.ClipTextEncoder(tsd, precision="half")
    E.ClipTextEncoder(tsd, precision="fast")                     # the constructors themselves work on these parameters


def test_unknown_names_still_raise():
    cfg, P = _cpu_visual()
    with pytest.raises(ZutisHipError, match="not in"):
        E.resolve_precision("bf16")
    with pytest.raises(ZutisHipError, match="not in"):
        E.ClipImageEncoder(P, cfg.patch, prefix="visual.", precision="halff")
    with pytest.raises(ZutisHipError):
        E.resolve_precision(["half"])                            # not a site name


def test_dropin_signature_and_default():
    import inspect
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zutis_amd", "dropin"))
    from utils.extract_image_embeddings import extract_image_embeddings
    assert inspect.signature(extract_image_embeddings).parameters["precision"].default == "exact"
    assert '"half"' in sys.modules[extract_image_embeddings.__module__].__doc__
