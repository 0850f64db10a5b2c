"""CPU: the deformation field's fp16 mode on the host side -- the C entry point is declared, exported and bound with
the fp32 entry's argument list, an unknown compute_dtype is refused before anything runs, the default stays fp32, and
the seeded test state tells the fp16 reference from the fp32 oracle by far more than the GPU tests' bars."""
import ctypes
import os
import re

import pytest
import torch

from tests import fp16_deform_reference as ref16d
from tests import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _field(log2_T=16):
    from quadraturefields_amd.field import Field
    return Field(scale=1.5, precision=16, log2_T=log2_T, L=16, max_res=512, min_res=16, output_dim=1, hidden_size=32,
                 num_features=2, back_prop=False, nl="relu")


def test_deform_f16_entry_is_declared_exported_and_bound(lib):
    from quadraturefields_amd import _C
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qf_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+qf_deform_field_forward_f16\s*\(", text)
    getattr(ctypes.CDLL(_C.LIB_PATH), "qf_deform_field_forward_f16")
    assert "qf_deform_field_forward_f16" in _C.EXPORTED_SYMBOLS
    # same argument list as the fp32 entry (only the table's element type differs)
    assert _C._SIGNATURES["qf_deform_field_forward_f16"] == _C._SIGNATURES["qf_deform_field_forward"]
    assert lib.qf_deform_field_forward_f16 is not None
    assert "`qf_deform_field_forward_f16`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_compute_dtype_defaults_to_fp32_and_precision_selects_nothing():
    from quadraturefields_amd.field import Field
    assert Field.compute_dtype == "fp32"
    assert Field.COMPUTE_DTYPES == ("fp32", "fp16")
    assert _field().compute_dtype == "fp32"                 # precision=16, as the reference's scripts build it


@pytest.mark.parametrize("value", ["bf16", "half", "fp17"])
def test_unknown_compute_dtype_is_refused_at_the_first_call(value):
    f = _field(log2_T=8)
    f.compute_dtype = value
    x = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="'fp32', 'fp16'"):
        f(x, return_grad=False)
    with pytest.raises(ValueError, match=value):
        f.density(x)
    with torch.enable_grad(), pytest.raises(ValueError, match=value):    # the training route checks it too
        f.density(x)


def test_the_seeded_state_tells_fp16_from_fp32():
    """The GPU tests require >= 99 % of points within 2e-5 of the fp16 reference; the fp32 oracle must be nowhere near
    that on the same data, or those tests could not tell the two modes apart."""
    from oracle import fields as ofields
    from quadraturefields_amd import synthetic
    f = _field()
    f.load_state_dict(synthetic.seeded_deform_state(f.xyz_encoder.grid.n_params), strict=False)
    wts = helpers.oracle_deform_weights(f)
    x, _ = helpers.random_points(3001, seed=9, outside_frac=0.0)
    d = (ref16d.deform_field_f16(x, wts) - ofields.deform_field(x, wts)).abs()[:, 0]
    assert (d <= 2e-5).float().mean().item() < 0.5          # measured 0.11
    assert d.median().item() > 2.5 * 2e-5                   # measured 9.4e-5
    # and the reference really is the fp16 encoding: its features sit on the fp16 grid
    x01 = (x + wts.scale) / (2.0 * wts.scale)
    h = ref16d.half_round(ofields.hash_encode(x01, ref16d.half_round(wts.table), wts.levels))
    assert torch.equal(h, h.half().float())


def test_switching_the_instance_back_to_fp32_releases_the_fp16_table_at_once():
    f = _field(log2_T=8)
    f.compute_dtype = "fp16"
    half = f._half_table()
    assert half.dtype == torch.float16 and f._half_table() is half       # built once, reused
    f.compute_dtype = "fp32"
    assert getattr(f, "_half_cache", None) is None                        # before any evaluation
