"""fp16 reference of the fused field kernel's fp16 mode (qf_field_forward_f16), for the tests.

The precision tcnn stores the reference's hash grid and fully fused MLPs in: fp16 table, weights and layer inputs,
fp32 accumulation.  Mirrors ``oracle.fields.*_bf16`` with ``t.half().float()`` at the kernel's rounding points:

* the table (rows converted to fp32 exactly, blended in fp32);
* the 8 blended features into the base MLP, every activation after a ReLU, the head input (SH | geo | the constant 1);
* every weight; the SG head's b1 (it rides in the first weight tile), while b2 / bout stay fp32.

torch's ``.half()`` is round-to-nearest-even, keeps fp16 subnormals and overflows to +-inf.
"""
from typing import List

import torch
import torch.nn.functional as F
from torch import Tensor

from oracle.fields import NGPWeights, features_to_rgb, hash_encode, normalize_to_aabb, sh4


def half_round(t: Tensor) -> Tensor:
    """Round-to-nearest-even to fp16, returned as fp32 (what an fp32-accumulating fp16 MFMA consumes)."""
    return t.half().float()


def _mlp_nobias_f16(x: Tensor, weights: List[Tensor]) -> Tensor:
    h = x
    for w in weights[:-1]:
        h = F.relu(F.linear(half_round(h), half_round(w)))
    return F.linear(half_round(h), half_round(weights[-1]))


def query_density_f16(x: Tensor, wts: NGPWeights):
    """(density [n,1], geo features [n,15]) with fp16 table / weights / inter-layer activations, fp32 accumulation."""
    selector, x01 = normalize_to_aabb(x, wts.aabb)
    enc = hash_encode(x01.reshape(-1, 3), half_round(wts.table), wts.levels)      # blend in fp32
    out = _mlp_nobias_f16(enc, wts.base)
    raw, feat = out[:, :1], out[:, 1:16]
    return torch.exp(raw - 1.0) * selector[:, None], feat


def ngp_forward_f16(x: Tensor, d: Tensor, wts: NGPWeights):
    """(rgb, density) of the NGP head in fp16."""
    density, feat = query_density_f16(x, wts)
    sh = sh4(((d + 1.0) / 2.0) * 2.0 - 1.0)
    h = torch.cat([sh, feat, torch.ones_like(feat[:, :1])], dim=-1)
    return torch.sigmoid(_mlp_nobias_f16(h, wts.head_tcnn)[:, :3]), density


def sg_forward_f16(x: Tensor, d: Tensor, wts: NGPWeights):
    """(rgb, density) of the SG head in fp16: w1/b1/w2/wout and the layer inputs fp16, b2/bout fp32."""
    density, feat = query_density_f16(x, wts)
    (w1, b1), (w2, b2), (wo, bo) = wts.head_layers
    h = F.relu(F.linear(half_round(feat), half_round(w1), half_round(b1)))
    h = F.relu(F.linear(half_round(h), half_round(w2), b2))
    f = F.linear(half_round(h), half_round(wo), bo)
    return features_to_rgb(f, d, wts.n_lobes), density
