"""Drop-in replacement for the reference's networks/zutis.py (ZUTIS, MLP) on MI355X.

Same constructor signature, attributes, state_dict keys/shapes (275 for ViT-B/16), forward() and predict()
contract as the reference (networks/zutis.py:15-549), so main.py / trainer.py / coco20k_eval.py /
utils.utils.get_network run unchanged.  The *insides* are different: torch modules are used only as parameter
containers; forward()/predict() execute hand-written HIP kernels from libzutis_hip.so through
zutis_amd.engine.ZutisEngine.  There is no torch-op or CPU fallback: without the HIP library or a GPU the calls
raise.  Training (autograd) is out of scope for the HIP path: under autograd forward() DELEGATES to the reference's own
networks/zutis.py when a maintainer has made it importable beside this overlay (see `reference_zutis_class`), sharing this
module's Parameters so that trainer.py's optimizer, checkpoints and the later HIP evaluation all see one set of weights; when it
is not importable the call raises NotImplementedError.  Inference (no_grad / frozen parameters) never takes that route.

Differences a maintainer should know:
  * `clip` is optional.  If it is importable the constructor does what the reference does (clip.load, encode_text,
    build the visual tower from its state_dict).  Otherwise pass `text_embeddings=` (and optionally
    `clip_state_dict=`); the architecture comes from the clip_arch name.
  * pycocotools / torchvision are optional (zutis_amd.rle restates encode / masks_to_boxes).
"""
import importlib
import os
import sys
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from zutis_amd import instances as _instances
from zutis_amd import ops as _ops
from zutis_amd import rle as _rle
from zutis_amd.engine import ZutisEngine

try:  # optional third-party pieces of the reference environment
    import clip as _clip
except ImportError:  # pragma: no cover - absent in this image
    _clip = None
try:
    from pycocotools.mask import encode as _coco_encode
except ImportError:  # pragma: no cover
    _coco_encode = None

# clip_arch name -> (width, layers, patch, grid, embed_dim)   (openai/CLIP model cards; clip_arch.py:590-627 infers the same)
_VIT_ARCHS = {
    "ViT-B/32": (768, 12, 32, 7, 512),
    "ViT-B/16": (768, 12, 16, 14, 512),
    "ViT-L/14": (1024, 24, 14, 16, 768),
    "ViT-L/14@336px": (1024, 24, 14, 24, 768),
}


# Where the reference's own ZUTIS class is looked up for the TRAINING branch of main.py (trainer.py:136 back-propagates through
# forward): this overlay shadows `networks.zutis`, so the original has to be importable under another name.  The launch script calls
#     keep_reference_for_training("<reference checkout>/networks/zutis.py")        # once, after `import networks.zutis` (the overlay)
# (file-copy deployment, where the overlay overwrote networks/zutis.py: keep the original as networks/zutis_reference.py and pass that
# path, or set ZUTIS_REFERENCE_MODULE=networks.zutis_reference).  The helper loads the FILE under the private module name below and
# leaves `networks*` / `utils*` in sys.modules exactly as it found them — aliasing by hand (`import networks.zutis as m;
# sys.modules[...] = m`) needs the `del sys.modules[...]` lines of INTEGRATION.md and still leaves the reference's `utils` cached.
REFERENCE_MODULE_NAMES = ("zutis_reference_networks_zutis", "zutis_reference.networks.zutis")
_OVERLAID = ("networks", "networks.zutis", "networks.selfmask", "networks.selfmask.selfmask", "networks.clip_text",
             "utils", "utils.running_score", "utils.bilateral_solver", "utils.extract_image_embeddings")


def keep_reference_for_training(reference_zutis_py: str):
    """Make the reference's own ZUTIS class available to the training delegate: execute the reference's `networks/zutis.py` FILE under
    the private name `zutis_reference_networks_zutis`.  While it is imported its sibling imports (`networks.clip_arch`, `networks.transformer`,
    `networks.positional_embedding`, `utils.iou`, networks/zutis.py:9-12) resolve against the reference checkout that holds the file;
    afterwards every module name this overlay provides (`networks`, `networks.zutis`, `utils.running_score`, ...) is what it was
    before the call — the overlay stays the canonical `networks.zutis`, which is asserted.  Returns the reference's class."""
    import importlib.util
    path = os.path.abspath(reference_zutis_py)
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    root = os.path.dirname(os.path.dirname(path))
    mine = sys.modules.get(__name__)
    saved = {k: sys.modules.pop(k) for k in _OVERLAID if k in sys.modules}
    path0 = list(sys.path)
    try:
        sys.path.insert(0, root)                            # the reference's own networks/ and utils/ packages for ITS imports
        spec = importlib.util.spec_from_file_location(REFERENCE_MODULE_NAMES[0], path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[REFERENCE_MODULE_NAMES[0]] = mod
        try:
            spec.loader.exec_module(mod)
        except BaseException:
            del sys.modules[REFERENCE_MODULE_NAMES[0]]
            raise
    finally:
        sys.path[:] = path0
        for k in _OVERLAID:                                 # the reference's packages of the same names leave; its other modules
            sys.modules.pop(k, None)                        # (networks.clip_arch, utils.iou, ...) stay cached under their own names
        sys.modules.update(saved)
    cls = getattr(mod, "ZUTIS", None)
    if cls is None or cls is globals().get("ZUTIS") or hasattr(mod, "keep_reference_for_training"):      # (a second copy of THIS file)
        del sys.modules[REFERENCE_MODULE_NAMES[0]]
        raise ImportError(f"{path} does not define the reference's ZUTIS class (is it the overlay's file?)")
    assert mine is None or sys.modules.get(__name__) is mine, "keep_reference_for_training: the overlay must stay the canonical module"
    return cls


def reference_zutis_class():
    """The reference's ZUTIS class if a maintainer made it importable (see REFERENCE_MODULE_NAMES), else None."""
    names = tuple(n for n in (os.environ.get("ZUTIS_REFERENCE_MODULE"),) if n) + REFERENCE_MODULE_NAMES
    for name in names:
        mod = sys.modules.get(name)
        if mod is None:
            try:
                mod = importlib.import_module(name)
            except ImportError:
                continue
        cls = getattr(mod, "ZUTIS", None)
        if cls is not None and cls is not globals().get("ZUTIS"):
            return cls
    return None


def convert_weight_like_reference(key: str, value: torch.Tensor) -> torch.Tensor:
    """What the reference constructor does to one CLIP parameter: `build_model` loads the state_dict into a model whose
    conv / Linear weights AND biases, attention in_proj weight / bias and `proj` / `text_projection` were converted to fp16
    (convert_weights, clip_arch.py:566-587, applied before load_state_dict at :625-626), so those values are rounded to fp16;
    LayerNorm parameters, class_embedding and positional_embedding stay fp32.  `.float()` follows (zutis.py:55)."""
    v = value.detach().float()
    name = key.rsplit(".", 1)[-1]
    is_ln = ".ln_" in "." + key          # ln_pre / ln_post / ln_1 / ln_2 (LayerNorm is not in convert_weights' list)
    rounded = (not is_ln) and (name in ("weight", "bias", "in_proj_weight", "in_proj_bias", "proj", "text_projection"))
    return v.half().float() if rounded else v


class MLP(nn.Module):
    """Parameter container with the reference's keys `layers.{i}.weight/bias` (networks/zutis.py:535-549)."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x):
        raise RuntimeError("MLP is executed inside the fused HIP plan (zutis_amd.engine); call ZUTIS.forward")


class _ResidualAttentionBlock(nn.Module):
    """Keys of clip_arch.ResidualAttentionBlock (clip_arch.py:300-321): attn.*, ln_1.*, mlp.c_fc.*, mlp.c_proj.*, ln_2.*"""

    def __init__(self, d_model: int, n_head: int):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = nn.LayerNorm(d_model)
        self.mlp = nn.Module()
        self.mlp.c_fc = nn.Linear(d_model, d_model * 4)
        self.mlp.c_proj = nn.Linear(d_model * 4, d_model)
        self.ln_2 = nn.LayerNorm(d_model)


class _Transformer(nn.Module):
    def __init__(self, width: int, layers: int, heads: int):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.Sequential(*[_ResidualAttentionBlock(width, heads) for _ in range(layers)])


class VisionTransformer(nn.Module):
    """Parameter container with clip_arch.VisionTransformer's keys and init (clip_arch.py:335-354)."""

    def __init__(self, input_resolution: int, patch_size: int, width: int, layers: int, heads: int, output_dim: int):
        super().__init__()
        self.input_resolution, self.output_dim, self.patch_size = input_resolution, output_dim, patch_size
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = _Transformer(width, layers, heads)
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))
        self.width = width


class _DecoderLayer(nn.Module):
    """Keys of transformer.TransformerDecoderLayer (networks/transformer.py:231-251)."""

    def __init__(self, d_model, nhead, dim_feedforward=2048):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead)
        self.multihead_attn = nn.MultiheadAttention(d_model, nhead)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(d_model), nn.LayerNorm(d_model), nn.LayerNorm(d_model)


class _Decoder(nn.Module):
    def __init__(self, d_model, nhead, num_layers):
        super().__init__()
        self.layers = nn.ModuleList(_DecoderLayer(d_model, nhead) for _ in range(num_layers))
        self.num_layers = num_layers
        self.norm = nn.LayerNorm(d_model)
        self.return_intermediate = True


class ZUTIS(nn.Module):
    def __init__(
            self,
            categories: List[str],
            segmentation_type: str = "semantic",
            clip_arch: str = "ViT-B/16",
            n_queries: int = 100,
            n_decoder_layers: int = 6,
            n_heads: int = 8,
            device: torch.device = torch.device("cuda:0"),
            encoder_type: str = "clip",
            frozen_bn: Optional[bool] = True,
            stop_gradient: Optional[bool] = True,
            decoder_image_n_dims: Optional[int] = None,
            *,
            text_embeddings: Optional[torch.Tensor] = None,
            clip_state_dict: Optional[dict] = None,
            vision_config: Optional[Tuple[int, int, int, int, int]] = None,
    ):
        super(ZUTIS, self).__init__()
        assert segmentation_type in ["semantic", "instance"], f"Invalid segmentation type: {segmentation_type}."
        # the reference constructor's own arguments (zutis.py:16-29), kept for the training delegate (_training_delegate)
        self._ctor_args = dict(categories=categories, segmentation_type=segmentation_type, clip_arch=clip_arch, n_queries=n_queries,
                               n_decoder_layers=n_decoder_layers, n_heads=n_heads, device=device, encoder_type=encoder_type,
                               frozen_bn=frozen_bn, stop_gradient=stop_gradient, decoder_image_n_dims=decoder_image_n_dims)
        object.__setattr__(self, "_delegate", None)      # not a registered submodule: its parameters ARE this module's
        if encoder_type is None:
            encoder_type = "clip"
        if encoder_type != "clip":
            raise ValueError(encoder_type)      # reference zutis.py:105-106 (its "dino" branch imports a missing module)
        arch = clip_arch.lstrip("dilated")
        if "ViT" not in arch:
            raise NotImplementedError(f"{clip_arch}: only the CLIP-ViT encoders are on the MI355X hot path (SURVEY.md §2)")

        model = None
        if text_embeddings is None or (clip_state_dict is None and vision_config is None and arch not in _VIT_ARCHS):
            if _clip is None:
                raise ImportError("`clip` is not installed: pass text_embeddings= (unit-norm [n_categories, dim]) "
                                  "and, for non-standard towers, vision_config=/clip_state_dict=")
            model, _ = _clip.load(arch, device=device)                                   # zutis.py:35
        if text_embeddings is None:
            te = model.encode_text(_clip.tokenize(categories).to(device)).to(dtype=torch.float32).detach()  # :36
            te = te / te.norm(dim=1, keepdim=True)                                          # :37
        else:
            te = torch.as_tensor(text_embeddings, dtype=torch.float32).detach().to(device)
        self.text_embeddings = te.requires_grad_(False)
        self.category_to_text_embedding: Dict[str, torch.Tensor] = {
            category: text_embedding for category, text_embedding in zip(categories, self.text_embeddings)
        }
        self.n_dims_text: int = self.text_embeddings.shape[1]
        self.frozen_bn: bool = True if frozen_bn is None else frozen_bn
        self.stop_gradient: bool = True if stop_gradient is None else stop_gradient
        self.decoder_image_n_dims = decoder_image_n_dims

        sd = clip_state_dict if clip_state_dict is not None else (model.state_dict() if model is not None else None)
        if vision_config is not None:
            width, layers, patch, grid, embed = vision_config
        elif sd is not None:                                                               # clip_arch.py:595-600
            width = sd["visual.conv1.weight"].shape[0]
            layers = len([k for k in sd if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
            patch = sd["visual.conv1.weight"].shape[-1]
            grid = round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5)
            embed = sd["visual.proj"].shape[1]
        else:
            width, layers, patch, grid, embed = _VIT_ARCHS[arch]
        self.encoder = VisionTransformer(patch * grid, patch, width, layers, width // 64, embed)
        if sd is not None:                                                                 # clip_arch.py:620-627 + zutis.py:55
            vis = {k[len("visual."):]: convert_weight_like_reference(k, v) for k, v in sd.items() if k.startswith("visual.")}
            self.encoder.load_state_dict(vis, strict=True)
        self.encoder.requires_grad_(True)

        self.ffn1 = MLP(input_dim=width, hidden_dim=256, output_dim=width, num_layers=3)   # zutis.py:59-64
        self.ffn2 = MLP(input_dim=width, hidden_dim=256, output_dim=width, num_layers=3)   # zutis.py:66-71
        print(f"{encoder_type} is loaded.")
        self.decoder = _Decoder(width, n_heads, n_decoder_layers)                           # zutis.py:114-126
        self.query_embed = nn.Embedding(n_queries, width).weight                            # zutis.py:131-134

        self.n_queries: int = n_queries
        self.n_heads: int = n_heads
        self.device: torch.device = device
        self.clip_arch: str = clip_arch
        self.encoder_type: str = encoder_type
        self._engine: Optional[ZutisEngine] = None
        # "fast" | "exact" | "f16" (zutis_amd.engine): exact = every contraction in the reference-equivalent f16x3 mode
        self.precision: str = "exact"
        # shape_rules.cross_attention_key_split: this module serves batch-1 evaluation loops (coco20k_eval.py:241-268), where the decoder's cross-attention is
        # 8 workgroups per launch unless its keys are split: forward at 480x640 4.25 / 3.56 / 3.21 / 3.04 / 2.97 ms for splits 1 / 2 / 4 / 8 / 16
        self.cross_attention_key_split: int = 12     # round 4, 4800 keys: 36.2 / 31.1 us for splits 8 / 12 (30 ties with 12: the merge grows with it)
        # forward() of batches <= 4 replays a hipGraph captured per input shape (the eager path costs ~11 us of Python + ctypes per launch,
        # more than most of a one-image forward's ~165 kernels): the reference's callers evaluate image by image (val batch_size 1,
        # trainer.py:328-345, coco20k_eval.py:258-267).  False: always launch eagerly.
        self.use_hip_graph: bool = True
        self._shapes_seen: Dict[Tuple[int, ...], int] = {}

    # ------------------------------------------------------------------ plumbing
    def _get_engine(self) -> ZutisEngine:
        if self._engine is not None and self._engine.precision != self.precision:
            self._engine = None                  # precision switched after construction
        if self._engine is None:
            self._engine = ZutisEngine(dict(self.named_parameters()), self.encoder.patch_size, self.n_heads,
                                       precision=self.precision)
            self._engine.cross_ksplit = self.cross_attention_key_split      # batch-1 evaluation loops: see shape_rules.cross_attention_key_split
        return self._engine

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._engine = None                      # parameters may have moved: rebuild the plan lazily
        return out

    def _training_delegate(self):
        """The reference's own ZUTIS (stock torch ops, autograd) over THIS module's Parameter objects — built once, only when a
        caller back-propagates through forward() and the reference class is importable (reference_zutis_class).  Same 275 keys,
        so every parameter slot of the delegate is re-pointed at ours: the optimizer main.py built over self.parameters() trains
        the weights the HIP engine later evaluates (its pack is keyed on the parameters' versions)."""
        d = self._delegate
        if d is None:
            cls = reference_zutis_class()
            if cls is None:
                return None
            d = cls(**self._ctor_args)
            mine = dict(self.named_parameters())
            theirs = dict(d.named_parameters())
            if set(mine) != set(theirs):
                raise RuntimeError("training delegate: the reference module's parameter names differ from this overlay's "
                                   f"({sorted(set(mine) ^ set(theirs))[:4]} ...)")
            for name, p in mine.items():
                mod, _, leaf = name.rpartition(".")
                owner = d.get_submodule(mod) if mod else d
                if leaf in owner._parameters:
                    owner._parameters[leaf] = p
                else:                                     # a bare Parameter attribute (query_embed = nn.Embedding(...).weight, zutis.py:131-134)
                    setattr(owner, leaf, p)
            object.__setattr__(self, "_delegate", d)
        d.text_embeddings = self.text_embeddings           # every call: update_text_embeddings() re-binds the attribute
        d.train(self.training)
        return d

    def update_text_embeddings(self, categories):
        if _clip is None:
            raise ImportError("update_text_embeddings needs the `clip` package (reference zutis.py:333-338)")
        model, _ = _clip.load(self.clip_arch.lstrip("dilated"), device=self.device)
        te = model.encode_text(_clip.tokenize(categories).to(self.device)).to(dtype=torch.float32).detach()
        self.text_embeddings = (te / te.norm(dim=1, keepdim=True)).requires_grad_(False)
        print(f"text embeddings have been changed for {', '.join(categories)}")

    # ------------------------------------------------------------------ forward
    def forward_transformer_encoder(self, x: torch.Tensor):
        tok, h, w = self._get_engine().encode(x.float())
        return tok.clone(), h, w            # the engine's buffer is reused by the next call: hand out a copy

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """x: b x 3 x h x w  ->  {"mask_proposals": b x L x Q x 2h' x 2w' (sigmoid), "patch_tokens": b x 2h' x 2w' x dim}"""
        eng = self._get_engine()

        def wants_grad():
            # the engine's flat parameter table, not self.parameters(): the module walk is ~0.2 ms of Python per call, and in a batch-1
            # evaluation loop the GPU idles through whatever the host does between one image's predict and the next image's launch
            return torch.is_grad_enabled() and any(p.requires_grad for p in eng.params.values())

        def train_or_refuse():
            # trainer.py:136 back-propagates through forward: the reference's own module over this module's Parameters when it is importable
            d = self._training_delegate()
            if d is not None:
                return d(x)
            raise NotImplementedError(
                "ZUTIS on MI355X is inference-only (the training loop is out of scope) and the reference's networks/zutis.py is not "
                "importable as a training delegate (zutis_amd.dropin.networks.zutis.REFERENCE_MODULE_NAMES / ZUTIS_REFERENCE_MODULE, "
                "INTEGRATION.md): wrap the call in torch.no_grad() or call .requires_grad_(False) as trainer.evaluate / "
                "coco20k_eval.py do")
        if self.use_hip_graph and x.shape[0] <= 4:       # host-bound regime: replay a captured hipGraph per input shape
            # ... from the SECOND time a shape is seen: capturing costs three eager forwards, and a native-resolution evaluation set holds
            # shapes that occur once (they run eagerly, as before round 4) next to the few that most images share (480x640, 640x480, ...)
            key = tuple(x.shape)
            seen = self._shapes_seen.get(key, 0)
            if seen < 2:
                if len(self._shapes_seen) > 4096:
                    self._shapes_seen.clear()
                self._shapes_seen[key] = seen + 1
            if seen >= 2 and self._delegate is None:     # a replay: launch first, check behind the launch (a training call drops the outputs;
                #                                          once a delegate exists — a training run — the check comes first)
                out = eng.forward_graphed(x.float().contiguous())
                if wants_grad():
                    return train_or_refuse()
                return out
            if wants_grad():
                return train_or_refuse()
            if seen >= 1:
                return eng.forward_graphed(x.float().contiguous())
            return eng.forward(x.float())
        if wants_grad():
            return train_or_refuse()
        return eng.forward(x.float())

    # ------------------------------------------------------------------ predict
    @torch.no_grad()
    def predict(
            self,
            dict_outputs: dict,
            mask_type: str,
            threshold: float = 0.5,
            image_ids: Optional[List[int]] = None,
            size: Optional[Tuple[int, int]] = None,
            label_id_to_category: Optional[Dict[int, str]] = None,
            new_label_id_to_old_label_id: Optional[Dict[int, int]] = None,
            temperature: float = 5,
            nms_type: str = "hard",
            return_logits: bool = False
    ):
        assert mask_type in ["semantic", "instance"]
        eng = self._get_engine()
        if mask_type == "semantic":                                                        # zutis.py:355-372
            size = None if size is None else (int(size[0]), int(size[1]))
            out = eng.predict_semantic(dict_outputs["patch_tokens"], self.text_embeddings, size, return_logits)
            if return_logits:
                return out
            labels = out.cpu().numpy()
            eng.check_finite()                   # the forward's status word, read behind the synchronisation the label copy just made
            return labels

        return self._predict_instances(dict_outputs, threshold, image_ids, size, label_id_to_category, new_label_id_to_old_label_id,
                                       temperature, nms_type)[0]

    def _predict_instances(self, dict_outputs, threshold, image_ids, size, label_id_to_category, new_label_id_to_old_label_id, temperature,
                           nms_type, paint: Optional[dict] = None):
        """predict(mask_type="instance") -> (predictions, ids).  paint (None: ids is None): the keyword arguments of
        ZutisEngine.paint_kept — the picture of the kept masks is launched behind the NMS, and ids[i] is prediction i's id in the map."""
        eng = self._get_engine()
        # instance prediction                                                              # zutis.py:374-470
        mask_proposals: torch.Tensor = dict_outputs["mask_proposals"]
        if len(mask_proposals.shape) == 5:
            mask_proposals = mask_proposals[:, -1, ...]
        size = None if size is None else (int(size[0]), int(size[1]))
        # the reference's two range asserts (zutis.py:385-386): a flag the statistics kernel raises while it reads the proposals anyway,
        # fetched with the NMS results (every device -> host copy is a stream synchronisation; the predict used to make four)
        range_flag = eng.status_word()           # the engine's sticky status word: bit 0 range (set below), bit 1 non-finite (set by the forward)
        masks_dev, scores, category_ids = eng.instance_candidates(
            mask_proposals, dict_outputs["patch_tokens"], self.text_embeddings, threshold, temperature, size, range_flag=range_flag)
        B, Q, Hm, Wm = masks_dev.shape
        if image_ids is None:
            image_ids = [0 for _ in range(B)]

        # The reference pulls all B x Q x H x W boolean masks to the host, then loops (zutis.py:423-469).  Here the masks
        # stay on the GPU: IoU counts come from the popcount kernel, the greedy per-category NMS loop runs in one kernel
        # launch (zh_mask_nms, one workgroup per image), the runs / boxes / areas of the KEPT masks are extracted from the loop's device
        # outputs (zh_mask_runs_kept), and only those cross PCIe.
        def raise_on(status: int):
            if status:
                range_flag.zero_()
                eng.raise_on_status(status)      # a non-finite forward: ZutisHipError, not a range assert
                assert not (status & _ops.STATUS_RANGE), "mask proposals outside [0, 1]"        # zutis.py:385-386
        if nms_type is None:
            raise_on(int(range_flag.item()))
            confidence_scores: np.ndarray = scores.cpu().numpy()
            category_ids_h: np.ndarray = category_ids.cpu().numpy()
            kept = [(bi, int(c), q, float(s)) for bi in range(B)
                    for q, (s, c) in enumerate(zip(confidence_scores[bi], category_ids_h[bi])) if c != 0]
            sel = np.array([bi * Q + q for bi, _, q, _ in kept], dtype=np.int32)
            slots = None
            if paint is not None:
                table, slots = _instances.slot_table(kept, B, Q, masks_dev.device)
                eng.paint_kept(masks_dev, *table, **paint)
            rles, boxes, areas = eng.encode_masks(masks_dev.view(B * Q, Hm, Wm), sel)
        else:
            assert nms_type in ["hard", "linear", "gaussian"]
            kept, rles, boxes, areas, status, *slots = eng.instance_nms_encode(masks_dev, scores, category_ids, nms_type,
                                                                               range_flag=range_flag, paint=paint)
            slots = slots[0] if slots else None
            raise_on(status)
        predictions: List[dict] = list()
        ids: Optional[List[int]] = None if slots is None else list()
        for k, ((bi, c, q, s), r, box, area) in enumerate(zip(kept, rles, boxes, areas)):
            if area == 0:                               # `if m.sum() == 0: continue` (zutis.py:281,439)
                continue
            if ids is not None:
                ids.append(slots[k] + 1)
            label_id = new_label_id_to_old_label_id[c] if new_label_id_to_old_label_id is not None else c
            prediction = {
                "category_id": label_id,
                "segmentation": r,                      # same dict as pycocotools.mask.encode(np.asfortranarray(m))
                "score": float(s),
                "image_id": image_ids[bi],
                "image_size": (Hm, Wm),
                "bbox": box,
            }
            if label_id_to_category is not None:
                prediction["pred_class"] = label_id_to_category[label_id]
            predictions.append(prediction)
        return predictions, ids

    @torch.no_grad()
    def predict_instances_painted(self, dict_outputs: dict, threshold: float = 0.5, image_ids: Optional[List[int]] = None,
                                  size: Optional[Tuple[int, int]] = None, label_id_to_category: Optional[Dict[int, str]] = None,
                                  new_label_id_to_old_label_id: Optional[Dict[int, int]] = None, temperature: float = 5,
                                  nms_type: str = "hard", *, packed: Optional[torch.Tensor] = None, desc: Optional[torch.Tensor] = None,
                                  desc_host=None, colours: Optional[torch.Tensor] = None, palette: Optional[torch.Tensor] = None,
                                  alpha: int = 128, outline: bool = True, min_score: float = 0.0, id_format: str = "u8",
                                  ids_out: Optional[torch.Tensor] = None, overlay_out: Optional[torch.Tensor] = None):
        """predict(mask_type="instance") with a picture of what it returns, painted on the device behind the NMS (zh_instance_paint; what
        utils/visualiser.py:154-187 draws with detectron2): the same predict arguments, and
          ids_out     None or u8 [B,H,W] (id_format "u8", up to 255 queries) / u8 [B,H,W,3] ("rg16": R = id & 255, G = id >> 8, B = 0) on the
                      device: per pixel the id of the prediction of highest score (ties: the lower id) among those with score > min_score
                      that cover it, 0 where none does;
          overlay_out None or u8 [B,H,W,3] on the device: the decoded images (packed / desc: the views of the batch's staging buffer, as
                      ZutisEngine.label_bytes takes them; desc_host: the loader's host copy of desc, checked instead of a blocking read)
                      with every such pixel blended with its prediction's colour — (img * (256 - alpha) + colour * alpha + 128) >> 8 — or,
                      with outline, in the pure colour where a 4-neighbour belongs to another prediction or to none;
          colours     u8 [B,Q,3] on the device, one per id (id - 1), or palette u8 [n,3] by the network's category index, or neither: entry
                      id - 1 of zutis_amd.instance_paint.instance_colours.
        Not both outputs None.  The launch rides the predict's stream: the buffers are complete once the predict has returned (its one
        copy of the small results is behind them); no copy and no synchronisation is added.  Returns (predictions, ids): the list
        predict(mask_type="instance") returns, and per prediction its id in the map (ids are unique per image, not across a batch)."""
        if ids_out is None and overlay_out is None:
            raise ValueError("predict_instances_painted: ids_out and overlay_out are both None")
        paint = dict(packed=packed, desc=desc, desc_host=desc_host, colours=colours, palette=palette, alpha=alpha, outline=outline,
                     min_score=min_score, id_format=id_format, ids_out=ids_out, overlay_out=overlay_out)
        return self._predict_instances(dict_outputs, threshold, image_ids, size, label_id_to_category, new_label_id_to_old_label_id,
                                       temperature, nms_type, paint=paint)

    @torch.no_grad()
    def score_semantic(self, dict_outputs: dict, gt_dev: torch.Tensor, metric_meter, size: Optional[Tuple[int, int]] = None,
                       gt_format: str = "u8") -> None:
        """metric_meter.update(gt, self.predict(dict_outputs, "semantic", size=size)) with the confusion matrix counted by the arg-max
        kernel itself (zutis.py:355-372 + utils/running_score.py:11-16): no label map, no copy to the host.  gt_dev: u8 on the
        device, [B,H,W] or ([B,H,W,3], gt_format "rg16"); metric_meter: the drop-in RunningScore."""
        metric_meter.update_device(self, dict_outputs, gt_dev, gt_format=gt_format, size=size)

    @staticmethod
    def non_maximum_suppression_indices(binary_masks, scores, category_ids, nms_type="hard", nms_threshold=0.3,
                                        sigma=0.5, threshold=0.001, iou=None):
        """Host form of the greedy per-category mask NMS with the reference's control flow (zutis.py:211-299), returning
        (category, query index, score) in its emission order.  predict() runs the device kernel (zh_mask_nms) instead; this
        method is kept as the call surface for code that passes its own masks and as the host-side cross-check in the tests.
        `iou` is the Q x Q matrix from the bit-packed popcount kernel (exact integer counts / float64 divide = utils/iou.py
        on boolean masks)."""
        assert nms_type in ["hard", "linear", "gaussian"]
        out = []
        for c in set(np.asarray(category_ids, dtype=np.int64)):     # the reference's own iteration order (zutis.py:237-238)
            c = int(c)
            if c == 0:
                continue
            cand = list(np.nonzero(category_ids == c)[0])
            cs = scores[cand].copy()
            selected = []
            while len(cand) > 0:
                order = np.argsort(cs)
                cand, cs = [cand[i] for i in order], cs[order]
                best, best_s = cand[-1], cs[-1]
                selected.append((best, best_s))
                nc, ns = [], []
                for m, s in zip(cand[:-1], cs[:-1]):
                    v = iou[m, best] if iou is not None else (
                        np.logical_and(binary_masks[m], binary_masks[best]).sum()
                        / (np.logical_or(binary_masks[m], binary_masks[best]).sum() + 1e-7))
                    if nms_type == "hard":
                        wgt = 0 if v > nms_threshold else 1
                    elif nms_type == "linear":
                        wgt = (1 - v) if v > nms_threshold else 1
                    else:
                        wgt = np.exp(-(v * v) / sigma)
                    s = s * wgt
                    if s > threshold:
                        nc.append(m)
                        ns.append(s)
                cand, cs = nc, np.array(ns)
            for m, s in selected:
                if np.any(binary_masks[m]):             # binary_masks: [Q,H,W] masks or a [Q] "mask is non-empty" vector
                    out.append((c, int(m), s.item() if hasattr(s, "item") else float(s)))
        return out
