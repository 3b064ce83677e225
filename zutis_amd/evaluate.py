"""Evaluation from image files: the loop of trainer.evaluate (trainer.py:295-384) / coco20k_eval.py over the drop-in ZUTIS with the
validation dataset's work split between decoding threads and the device, and the confusion matrix counted where the labels are made.

The reference's loop, per image: DataLoader workers decode, run to_tensor + normalize and pickle an fp32 tensor to the parent; the
parent uploads it, forwards, pulls an int64 label map to the host (predict "semantic"), and RunningScore.update converts ground truth
and prediction to int64 and uploads both again.  Here the file pipeline of preprocess.py: threads decode the image and its
ground-truth PNG one batch ahead into pinned staging (EvalBatchLoader: batches of one file size); per batch (device_batches) ONE
host-to-device copy of bytes (3 per image pixel, 1 or 3 per ground-truth pixel) and ops.resize_normalize (Pillow BILINEAR + to_tensor
+ normalize, bit for bit; the identity when the image is not resized); then the module's own forward, and
zh_upsample_argmax_score, which adds every pixel's (gt, label) pair to one device
histogram while the label is in a register — no label map, no copy back.  The histogram crosses to the host once, at the end.
"""
from __future__ import annotations

import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import preprocess
from .preprocess import MAX_THREADS


def _require_dropin(network, who: str):
    if not (hasattr(network, "_get_engine") and hasattr(network, "predict") and hasattr(network, "text_embeddings")):
        raise TypeError(f"{who} needs the MI355X drop-in ZUTIS (networks/zutis.py of the overlay): there is no torch / CPU fallback")


def collect_instance_predictions(network, out: dict, batch, image_ids: Optional[Sequence], per_image: List[List[dict]], **predict_args):
    """predict(mask_type="instance") of one batch at the files' size (trainer.py:337-345, coco20k_eval.py:258-265): predict numbers the
    images by their positions in the path list, which file each dict under per_image and are then replaced by image_ids' entry (None: 0)."""
    for p in network.predict(dict_outputs=out, mask_type="instance", size=batch.size_hw, image_ids=list(batch.indices), **predict_args):
        i = p["image_id"]
        p["image_id"] = image_ids[i] if image_ids is not None else 0
        per_image[i].append(p)


def confusion_scores(hist: np.ndarray):
    """RunningScore.get_scores (utils/running_score.py:24-49) of a float64 [n, n] confusion matrix: (scores, per-class IoU)."""
    n = hist.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                    # an empty matrix: NaN scores, as get_scores gives, without the notice
        acc = np.diag(hist).sum() / hist.sum()
        acc_cls = np.nanmean(np.diag(hist) / hist.sum(axis=1))
        iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
        mean_iu = np.nanmean(iu)
        freq = hist.sum(axis=1) / hist.sum()
        fwavacc = (freq[freq > 0] * iu[freq > 0]).sum()
    return {"Pixel Acc": acc, "Mean Acc": acc_cls, "FreqW Acc": fwavacc, "Mean IoU": mean_iu}, dict(zip(range(n), iu))


@torch.no_grad()
def evaluate_from_files(network, p_images: Sequence[str], p_gts: Sequence[str], n_categories: int, *, gt_format: str = "u8",
                        max_size: Optional[int] = None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), batch_size: int = 4,
                        n_workers: int = 16, window: int = 512, instance: bool = False, image_ids: Optional[Sequence] = None,
                        new_label_id_to_old_label_id: Optional[Dict[int, int]] = None, nms_type: Optional[str] = "hard",
                        return_labels: bool = False, coco_annotations=None) -> dict:
    """trainer.evaluate's loop (trainer.py:316-347) from lists of image files and ground-truth PNGs.

    network: the drop-in ZUTIS (zutis_amd/dropin/networks/zutis.py) on a GPU, its text embeddings those of the n_categories classes.
    gt_format "u8": 8-bit grey / palette PNGs, label = the byte (coco2017.py:135, coco20k.py:179); "rg16": RGB PNGs, label = R + 256 G
    (imagenet_s.py:93).  Pixels whose label is not below n_categories (255, 1000) are not counted, as _fast_hist masks them.
    max_size None: the image goes in at its own size; max_size=1024: the longer edge is capped with Pillow BILINEAR
    (imagenet_s.py:71-76, preprocess.longer_edge_size).  Either way the prediction is scored at the file's own (H, W)
    (trainer.py:322-325).  Batches hold up to batch_size images of one file size out of a window of `window` paths
    (preprocess.bucket_batches of preprocess.eval_bucket_key); n_workers (at most 16) threads decode.
    instance=True: predict(mask_type="instance", size=(H, W), image_ids=..., new_label_id_to_old_label_id=..., nms_type=...) per batch
    (trainer.py:337-345); image_ids: one per image (None: 0, as predict's default).
    Returns {"scores", "cls_iu": RunningScore.get_scores()'s pair, "confusion_matrix": float64 [n, n], "instance_predictions": the
    prediction dicts in input-path order ([] without instance), "labels": {index: int64 [H, W] label map} with return_labels, else None}.
    coco_annotations (a COCO annotation dict or the path of its JSON) together with instance=True adds "coco_metrics": coco_eval.mask_ap of
    the instance predictions against it (trainer.py:400-405), over image_ids when they are given (coco20k_eval.py:282).
    A missing or unreadable file and a ground truth of the wrong mode or size are raised here (FileNotFoundError / OSError /
    ValueError); no decoding thread outlives the call and the device stays usable."""
    p_images, p_gts = list(p_images), list(p_gts)
    if len(p_images) != len(p_gts):
        raise ValueError("evaluate_from_files: one ground-truth file per image")

    def source(dev):
        loader = preprocess.EvalBatchLoader(p_images, p_gts, max_size, batch_size, max(1, min(int(n_workers), MAX_THREADS)), window=window,
                                            gt_format=gt_format)
        return loader, lambda batch, views: views[2]                                    # the PNG's bytes, as they arrived with the images

    return _evaluate(network, "evaluate_from_files", p_images, n_categories, source, gt_format=gt_format, mean=mean, std=std,
                     instance=instance, image_ids=image_ids, new_label_id_to_old_label_id=new_label_id_to_old_label_id, nms_type=nms_type,
                     return_labels=return_labels, coco_annotations=coco_annotations)


def _evaluate(network, who: str, p_images: List[str], n_categories: int, source, *, gt_format, mean, std, instance, image_ids,
              new_label_id_to_old_label_id, nms_type, return_labels, coco_annotations) -> dict:
    """The loop evaluate_from_files and evaluate_from_annotations share.  source(dev) -> (the batch loader, ground_truth(batch, views) ->
    the batch's ground truth on the device: u8 [B, H, W], or [B, H, W, 3] with gt_format "rg16"); it is called only when there are images."""
    if image_ids is not None and len(image_ids) != len(p_images):
        raise ValueError(f"{who}: one image id per image")
    _require_dropin(network, who)
    n = int(n_categories)
    if network.text_embeddings.shape[0] != n:
        raise ValueError(f"{who}: the network holds {network.text_embeddings.shape[0]} text embeddings, n_categories is {n}")
    eng = network._get_engine()
    dev = eng._device()
    hist = torch.zeros((n * n,), dtype=torch.int64, device=dev)
    per_image: List[List[dict]] = [[] for _ in p_images]
    labels_out: Optional[Dict[int, np.ndarray]] = {} if return_labels else None
    if p_images:
        lut = torch.from_numpy(preprocess.normalise_table(mean, std)).to(dev)
        loader, ground_truth = source(dev)
        with preprocess.device_batches(loader, dev, preprocess.resize_normalize_of(lut)) as steps:
            for batch, views, x in steps:
                B, (H, W) = len(batch.paths), batch.size_hw
                out = network(x)                                                       # the module's forward: its hipGraph replay applies
                labels = torch.empty((B, H, W), dtype=torch.int64, device=dev) if return_labels else None
                eng.score_semantic(out["patch_tokens"], network.text_embeddings, ground_truth(batch, views), hist, gt_format=gt_format,
                                   size=(H, W), labels=labels)
                if instance:
                    collect_instance_predictions(network, out, batch, image_ids, per_image,
                                                 new_label_id_to_old_label_id=new_label_id_to_old_label_id, nms_type=nms_type)
                if return_labels:
                    for i, m in zip(batch.indices, labels.cpu().numpy()):
                        labels_out[i] = m
            eng.check_finite()                                                         # the forwards' status word: one read for the whole run
    cm = hist.cpu().numpy().reshape(n, n).astype(np.float64)                           # the one crossing of the histogram
    scores, cls_iu = confusion_scores(cm)
    res = {"scores": scores, "cls_iu": cls_iu, "confusion_matrix": cm, "instance_predictions": [p for ps in per_image for p in ps],
           "labels": labels_out}
    if coco_annotations is not None and instance:
        from . import coco_eval
        res["coco_metrics"] = coco_eval.mask_ap(coco_annotations, res["instance_predictions"], image_ids=image_ids, device=dev)
    return res


@torch.no_grad()
def evaluate_from_annotations(network, p_images: Sequence[str], coco_annotations, n_categories: int, *, image_ids: Sequence,
                              max_size: Optional[int] = None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), batch_size: int = 4,
                              n_workers: int = 16, window: int = 512, instance: bool = False,
                              new_label_id_to_old_label_id: Optional[Dict[int, int]] = None, nms_type: Optional[str] = "hard",
                              return_labels: bool = False, label_of: Optional[Dict[int, int]] = None, order: str = "file",
                              overlap: str = "last", crowd: str = "label", ignore_value: int = 255) -> dict:
    """evaluate_from_files without ground-truth files: the semantic ground truth of each batch is painted on the device from the COCO
    annotation file (annotation_labels.LabelPainter.paint: one launch per batch) where the PNG's bytes used to arrive — no ground-truth
    PNG, decode or host-to-device copy.  coco_annotations: the annotation dict or the path of its JSON (`instances_*.json`); image_ids:
    the COCO id of every image of p_images (the `images` entry gives the size the file must have); label_of / order / overlap / crowd /
    ignore_value: annotation_labels.paint_plan's; the other keywords and the result are evaluate_from_files'.  The segmentations are
    converted once, before the first batch.  The batches are the ones evaluate_from_files forms for the same files, batch_size and window
    (preprocess.PredictBatchLoader), so the scores are those of evaluate_from_files over annotation_labels.write_semantic_masks' PNGs,
    count for count.  instance=True: the same annotation dict goes to coco_eval.mask_ap and the result gains "coco_metrics"."""
    from . import annotation_labels, coco_eval
    p_images = list(p_images)
    if image_ids is None or len(image_ids) != len(p_images):
        raise ValueError("evaluate_from_annotations: one image id per image")
    image_ids = list(image_ids)
    gt = coco_eval._load(coco_annotations)
    plan = annotation_labels.paint_plan(gt, image_ids, label_of=label_of, order=order, overlap=overlap, crowd=crowd, ignore_value=ignore_value)

    def source(dev):
        painter = annotation_labels.LabelPainter(plan, dev)
        loader = preprocess.PredictBatchLoader(p_images, max_size, batch_size, max(1, min(int(n_workers), MAX_THREADS)), window=window)

        def ground_truth(batch, views):
            for i in batch.indices:
                if (plan.images[i]["h"], plan.images[i]["w"]) != tuple(batch.size_hw):
                    raise ValueError(f"{p_images[i]}: a file of {tuple(batch.size_hw)} pixels, the annotations give image "
                                     f"{plan.images[i]['id']!r} as {(plan.images[i]['h'], plan.images[i]['w'])}")
            return painter.paint(batch.indices)
        return loader, ground_truth

    return _evaluate(network, "evaluate_from_annotations", p_images, n_categories, source, gt_format="u8", mean=mean, std=std,
                     instance=instance, image_ids=image_ids, new_label_id_to_old_label_id=new_label_id_to_old_label_id, nms_type=nms_type,
                     return_labels=return_labels, coco_annotations=gt if instance else None)


def eval_files_of(dataset):
    """(p_images, p_gts, gt_format, max_size) for evaluate_from_files from one of the reference's validation dataset objects, by its
    `name` and the attributes and path rules its __getitem__ uses:

      imagenet-s50 / -s300 / -s919 (datasets/imagenet_s.py:63-99): p_images / p_gts as globbed, label R + 256 G -> "rg16", max_size = its
                            max_size (1024);
      coco2017, coco20k     (datasets/coco2017.py:121-149, coco20k.py:165-202): get_image_path(image_id) over image_ids, the mask at
                            {dir_dataset}/annotations/semantic_segmentation_masks/{file name without .jpg}.png read as it is -> "u8", None.

    TypeError for anything else — coca among them: its __getitem__ rewrites the mask (`gt[gt == 255] = label_id`, datasets/coca.py:42-43,
    the label taken from the file's directory), which neither format expresses — and for an imagenet-s split without ground truth."""
    name = getattr(dataset, "name", None)
    if isinstance(name, str) and name.startswith("imagenet-s"):
        if not hasattr(dataset, "p_gts"):
            raise TypeError(f"eval_files_of: the {name} dataset has no ground truth (its test split)")
        return list(dataset.p_images), list(dataset.p_gts), "rg16", int(dataset.max_size)
    if name in ("coco2017", "coco20k"):
        p_images = [dataset.get_image_path(i) for i in dataset.image_ids]
        p_gts = [f"{dataset.dir_dataset}/annotations/semantic_segmentation_masks/{p.split('/')[-1].split('.jpg')[0]}.png" for p in p_images]
        return p_images, p_gts, "u8", None
    if name == "coca":
        raise TypeError("eval_files_of: coca's __getitem__ maps the mask's 255 to the label of the file's directory (datasets/coca.py:42-43): "
                        "its ground truth is not one of the two file formats")
    raise TypeError(f"eval_files_of: no path rules for the dataset {name!r} ({type(dataset).__name__})")


def eval_annotations_of(dataset):
    """(p_images, p_annotations, image_ids) for evaluate_from_annotations from one of the reference's COCO validation dataset objects, by
    its `name` and the attributes its __init__ / __getitem__ use: get_image_path(image_id) over image_ids (datasets/coco2017.py:124-126,
    coco20k.py:168-170) and p_annotations, the file its COCO object was read from (coco2017.py:22, coco20k.py:20).  TypeError for
    anything else, as eval_files_of."""
    name = getattr(dataset, "name", None)
    if name not in ("coco2017", "coco20k"):
        raise TypeError(f"eval_annotations_of: no annotation file rules for the dataset {name!r} ({type(dataset).__name__})")
    image_ids = list(dataset.image_ids)
    return [dataset.get_image_path(i) for i in image_ids], str(dataset.p_annotations), image_ids
