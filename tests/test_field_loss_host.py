"""CPU: the formulas of qf_field_quadrature_loss (csrc/field_train.hip) and the input sets of its GPU tests.

The kernel implements the backward of stage 2's loss written out by hand; tests/field_loss_reference.closed_form is
that derivation in float64.  Here it is pinned against torch's double autograd, the loss against
``Field.compute_field_loss``, and the GPU tests' inputs are checked to stay clear of the branch points.
"""
import pytest
import torch

from tests import field_loss_reference as R


@pytest.fixture(scope="module")
def wts():
    return R.seeded_weights(**R.TABLES["hashed"])


@pytest.mark.parametrize("upstream", [1.0, -2.5])
def test_closed_form_backward_equals_double_autograd(wts, upstream):
    inp = R.seeded_inputs(500, seed=1)
    cf = R.closed_form(inp, wts, upstream)
    ag = R.autograd_step(inp, wts, upstream)
    assert ag["bout"] is None                                   # lout.bias does not enter the loss
    for k in ("loss", "value", "grad", "d_enc") + R.NAMES:
        got, want = cf[k][0], ag[k].reshape(cf[k][0].shape)
        scale = float(want.abs().max())
        assert scale > 0, k
        assert float((got - want).abs().max()) <= 1e-12 * scale, (k, float((got - want).abs().max()), scale)
        assert bool((cf[k][1] >= cf[k][0].abs() * (1 - 1e-12)).all()), k      # M bounds the value it belongs to


def test_probe_subset_uses_the_batch_mean(wts):
    """n_total: a subset's loss and gradients are its share of the batch's."""
    inp = R.seeded_inputs(64, seed=2)
    full = R.closed_form(inp, wts)
    a, b = R.closed_form(inp.rows(torch.arange(0, 20)), wts, n_total=64), R.closed_form(inp.rows(torch.arange(20, 64)), wts, n_total=64)
    for k in ("loss",) + R.NAMES:
        assert torch.allclose(a[k][0] + b[k][0], full[k][0], rtol=1e-11, atol=1e-14), k


def test_loss_is_compute_field_loss_of_the_oracle_gradient(wts):
    from quadraturefields_amd.field import Field
    inp = R.seeded_inputs(300, seed=3)
    ag = R.autograd_step(inp, wts)
    want = Field.compute_field_loss(None, inp.weights.double(), inp.weights_rev.double(), ag["grad"], inp.dirs.double())
    assert abs(float(ag["loss"]) - float(want)) <= 1e-14 * abs(float(want))


def test_inputs_exercise_both_signs_and_empty_space(wts):
    inp = R.seeded_inputs(4000, seed=4)
    cf = R.closed_form(inp, wts)
    empty = (inp.weights == 0) & (inp.weights_rev == 0)
    assert 0.15 < float(empty.float().mean()) < 0.25
    norms = inp.dirs.norm(dim=1)
    assert float(norms.min()) < 0.5 and float(norms.max()) > 3.0             # unnormalised
    for q in (cf["p"], cf["r"]):
        assert 0.1 < float((q > 0).float().mean()) < 0.9, float((q > 0).float().mean())


@pytest.mark.parametrize("table", sorted(R.TABLES))
@pytest.mark.parametrize("n,seed", [(1, 11), (17, 12), (4000, 13), (98309, 14)])
def test_gpu_input_sets_stay_clear_of_the_branch_points(table, n, seed):
    """The share of points with some branch quantity within 2^-22 of its magnitude is at most 0.1 % (expected: about
    34 * 2 * 2^-22 = 2e-5), and the spare points replace them all."""
    w = R.seeded_weights(**R.TABLES[table])
    inp, share = R.clean_inputs(n, seed, w)
    assert share <= 1e-3, share
    assert float(R.closed_form(inp, w)["margin"].min()) >= R.MARGIN
