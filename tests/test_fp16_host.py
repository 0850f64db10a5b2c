"""CPU: the fp16 field mode's host side -- the C entry point is declared, exported and bound, the frame job carries
its precision where the reserved word was, an unknown compute_dtype is refused, and the fp16 reference rounds as the
kernel does (subnormals kept)."""
import ctypes
import os
import re

import pytest
import torch

from tests import fp16_reference as ref16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_f16_entry_is_declared_exported_and_bound(lib):
    from quadraturefields_amd import _C
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qf_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+qf_field_forward_f16\s*\(", text)
    assert re.search(r"\bqf_sg_head_f16\b", text)
    getattr(ctypes.CDLL(_C.LIB_PATH), "qf_field_forward_f16")
    assert "qf_field_forward_f16" in _C.EXPORTED_SYMBOLS
    # same argument list as the bf16 entry
    assert _C._SIGNATURES["qf_field_forward_f16"] == _C._SIGNATURES["qf_field_forward_bf16"]
    assert lib.qf_field_forward_f16 is not None


def test_frame_job_field_precision_takes_the_reserved_word():
    from quadraturefields_amd import _C
    assert _C.FrameJob.field_precision.offset == 52
    assert _C.FrameJob.field_precision.size == 4
    assert "reserved_" not in dict(_C.FrameJob._fields_)
    assert ctypes.sizeof(_C.FrameJob) == 248                               # unchanged by the rename
    assert _C.FrameJob().field_precision == _C.FIELD_FP32 == 0
    assert (_C.FIELD_BF16, _C.FIELD_FP16) == (1, 2)
    text = open(os.path.join(ROOT, "include", "qf_hip.h")).read()
    for name, value in (("QF_FIELD_FP32", 0), ("QF_FIELD_BF16", 1), ("QF_FIELD_FP16", 2)):
        assert re.search(rf"#define {name} {value}\b", text), name


@pytest.mark.parametrize("cls", ["NGPRadianceField", "NGPRadianceFieldSGNew"])
def test_unknown_compute_dtype_is_refused_at_the_first_call(cls):
    from quadraturefields_amd.radiance_fields import ngp
    kw = {"use_viewdirs": False} if cls == "NGPRadianceFieldSGNew" else {}
    f = getattr(ngp, cls)(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=8, **kw)
    f.compute_dtype = "fp17"
    x = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="'fp32', 'bf16', 'fp16'"):
        f(x, x)
    with pytest.raises(ValueError, match="fp17"):
        f.query_density(x)


def test_reference_rounding_is_fp16_rne_and_keeps_subnormals():
    from oracle import fields as ofields
    x = torch.tensor([1e-6])
    assert ref16.half_round(x).item() != 0.0
    assert ref16.half_round(x).item() == 17 * 2.0 ** -24                  # nearest fp16 subnormal
    assert ref16.half_round(x).item() != ofields.bf16_round(x).item()
    # round to nearest even at a tie, overflow to +-inf
    tie = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11])
    assert ref16.half_round(tie).tolist() == [1.0, 1.0 + 2 * 2.0 ** -10]
    assert ref16.half_round(torch.tensor([70000.0, -70000.0])).tolist() == [float("inf"), float("-inf")]
