"""Drop-in replacement for the reference's criterion.py (Criterion) on MI355X.

Same constructor arguments and defaults, `text_embeddings` attribute, `__call__` keywords and return dict as the reference
(criterion.py:8-23, 63-161): 4-D [b, Q, h, w] and 5-D [b, L, Q, h, w] proposals, the reference's AssertionError when a proposal
leaves [0, 1], images whose GT masks sum to 0 skipped (the mask loss is still divided by the batch size), NaN CE when every pixel
is ignored, and `instance_indices` / `query_indices` of the last (image, layer) matched.  Forward and backward run the HIP kernels
of zutis_amd/criterion.py; gradients flow into whatever torch graph produced the proposals and patch tokens (the training
delegate of networks/zutis.py, or any other).  A semantic label that is neither < n_categories nor ignore_index raises ValueError
(the reference's torch call would hit a device-side assert).  There is no CPU fallback: CPU tensors raise.

The constructor is the reference's, argument for argument (tests/test_criterion_cpu.py pins the signature), so HipCriterion's
keyword-only `assignment` is reached as an attribute here: `criterion.assignment = "device"` on an instance, or
`Criterion.default_assignment = "device"` once at start-up for every instance built afterwards.  "host" (default) is scipy on the
host, as the reference; "device" gives the same matches from the GPU solver, with no host trip for ground truth that is already on
the device (see HipCriterion).
"""
from zutis_amd.criterion import HipCriterion


class Criterion(HipCriterion):
    default_assignment = "host"

    def __init__(self, text_embeddings, weight_ce_loss=1.0, weight_mask_loss=1.0, weight_dice_loss=1.0, weight_bce_loss=1.0,
                 ignore_index=255):
        super().__init__(text_embeddings, weight_ce_loss, weight_mask_loss, weight_dice_loss, weight_bce_loss, ignore_index,
                         assignment=self.default_assignment)


__all__ = ["Criterion"]
