"""fp16 reference of the deformation field's fp16 mode (qf_deform_field_forward_f16), for the tests.

The reference's own precision (field.py:135-138,157-171,186-203): ``x01`` fp32, an fp16 tcnn ``Encoding`` (fp16 table,
fp16 output), ``torch.cat([x01, h])`` promoting back to fp32, and the fp32 ``BasicDecoder`` with fp32 biases.  The
kernel's choice where tcnn's is not pinned: table rows converted to fp32 exactly, blended in fp32, each blended feature
rounded once (round-to-nearest-even) to fp16.
"""
import torch
from torch import Tensor

from oracle.fields import DeformWeights, basic_decoder, hash_encode
from tests.fp16_reference import half_round


def deform_field_f16(x: Tensor, wts: DeformWeights) -> Tensor:
    """Field.density at the reference's precision: [N,3] -> [N,1]."""
    x01 = (x + wts.scale) / (2.0 * wts.scale)
    h = half_round(hash_encode(x01, half_round(wts.table), wts.levels))
    return basic_decoder(torch.cat([x01, h], dim=1), wts.layers)
