"""Drop-in for the original CSPN release's module (network/libs/post_process/CSPN.py:14-231).

Same constructors and forward signatures as the reference classes, called positionally ``layer(guidance, blur_depth,
sparse_depth)`` and ``layer(guidance, blur_depth)``.  No parameters, no buffers (empty state_dict).  ``prop_time`` is the one
extension: the reference hard-codes 16 iterations (CSPN.py:36, :146).  The recurrence — eight |guidance| gates as box-normalised
3x3 filters on the depth, their element-wise maximum, the sparse blend — runs in libcspn_hip.so (include/cspn_max8.h), forward
and backward; fp32 only, as the reference.  See functional.cspn_max8_propagate.
"""
import torch.nn as nn

from ..functional import cspn_max8_propagate


class AffinityPropagate(nn.Module):

    def __init__(self, spn=False, prop_time=16):
        super(AffinityPropagate, self).__init__()
        self.spn = spn           # kept for parity with CSPN.py:18 (the reference never reads it either)
        self.prop_time = prop_time

    def forward(self, guidance, blur_depth, sparse_depth):
        """guidance [B,C>=8,H,W] (channels 0..7 used), blur_depth [B,1,H,W], sparse_depth [B,1,H,W] -> refined depth [B,1,H,W]."""
        if sparse_depth is None:
            raise ValueError("CSPN.AffinityPropagate needs sparse_depth; AffinityPropagate_prediction is the form without it")
        return cspn_max8_propagate(guidance, blur_depth, sparse_depth, self.prop_time)


class AffinityPropagate_prediction(nn.Module):

    def __init__(self, spn=False, prop_time=16):
        super(AffinityPropagate_prediction, self).__init__()
        self.spn = spn
        self.prop_time = prop_time

    def forward(self, guidance, blur_depth):
        """guidance [B,C>=8,H,W] (channels 0..7 used), blur_depth [B,1,H,W] -> refined depth [B,1,H,W]; no sparse blend."""
        return cspn_max8_propagate(guidance, blur_depth, None, self.prop_time)
