"""Drop-in replacement for the reference's criterion.py (Criterion) on MI355X.

Same constructor arguments and defaults, `text_embeddings` attribute, `__call__` keywords and return dict as the reference
(criterion.py:8-23, 63-161): 4-D [b, Q, h, w] and 5-D [b, L, Q, h, w] proposals, the reference's AssertionError when a proposal
leaves [0, 1], images whose GT masks sum to 0 skipped (the mask loss is still divided by the batch size), NaN CE when every pixel
is ignored, and `instance_indices` / `query_indices` of the last (image, layer) matched.  Forward and backward run the HIP kernels
of zutis_amd/criterion.py; gradients flow into whatever torch graph produced the proposals and patch tokens (the training
delegate of networks/zutis.py, or any other).  A semantic label that is neither < n_categories nor ignore_index raises ValueError
(the reference's torch call would hit a device-side assert).  There is no CPU fallback: CPU tensors raise.
"""
from zutis_amd.criterion import HipCriterion


class Criterion(HipCriterion):
    pass


__all__ = ["Criterion"]
