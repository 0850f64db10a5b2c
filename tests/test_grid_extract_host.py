"""CPU: the stage-2 Field configuration (train_field.py:238-252) and the host side of field_utils' grid extraction:
constructor, state-dict layout, level table, lattice axis, slab planner, the pooling order, refusals."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle import fields as ofields

STAGE2 = dict(scale=0.5, precision=16, log2_T=30, L=16, max_res=512, min_res=16, output_dim=1, hidden_size=16,
              num_features=2, back_prop=False, nl="elu")


@pytest.fixture(scope="module")
def stage2_field():
    from quadraturefields_amd.field import Field
    return Field(**STAGE2)


def test_stage2_field_constructs_with_the_reference_layout(stage2_field):
    f = stage2_field
    assert isinstance(f.decoder_field.activation, torch.nn.ELU) and f.decoder_field.activation.alpha == 1.0
    shapes = {k: tuple(v.shape) for k, v in f.state_dict().items() if not k.startswith(("center", "xyz_m", "half"))}
    lv = ofields.grid_levels(16, 30, 16, ofields.field_per_level_scale(512, 0.5, 16, 16))
    assert shapes == {"xyz_encoder.params": (2 * lv.n_entries,),
                      "decoder_field.layers.0.weight": (16, 35), "decoder_field.layers.0.bias": (16,),
                      "decoder_field.layers.1.weight": (16, 16), "decoder_field.layers.1.bias": (16,),
                      "decoder_field.lout.weight": (1, 16), "decoder_field.lout.bias": (1,)}
    # all 16 levels dense, resolutions 16 .. 256: 39 601 112 rows
    assert lv.n_entries == 39_601_112 and not any(lv.hashed)
    assert lv.resolution[0] == 16 and lv.resolution[-1] == 256
    d = f.xyz_encoder.grid.desc
    assert list(d.offset) == lv.offset and list(d.resolution) == lv.resolution and list(d.scale) == lv.scale
    assert not f.deform_kernel


def test_accepted_and_refused_configurations():
    from quadraturefields_amd.field import Field
    base = dict(STAGE2, log2_T=12)
    for nl, hidden in itertools.product(("relu", "elu"), (16, 32)):
        f = Field(**dict(base, nl=nl, hidden_size=hidden))
        assert f.decoder_field.layers[0].weight.shape == (hidden, 35)
        assert f.deform_kernel == (nl == "relu" and hidden == 32)
    for bad in (dict(output_dim=2), dict(bias=False), dict(bias_last=False), dict(hidden_size=64), dict(nl="tanh")):
        with pytest.raises(NotImplementedError, match="hidden_size 16 or 32"):
            Field(**dict(base, **bad))


def test_lattice_axis_is_the_references():
    from quadraturefields_amd.field_utils import lattice_axis
    for n, s in ((32, 0.5), (1024, 0.5), (5, 1.5), (64, 0.37)):
        want = torch.linspace(-1, 1, 2 * n) * s
        got = lattice_axis(n, s)
        assert got.dtype == torch.float32 and torch.equal(got, want)


def test_slab_planner_covers_once():
    from quadraturefields_amd.field_utils import plan_slabs
    for n, step in ((1, None), (7, 1), (7, 3), (1024, 64), (1000, 64), (13, 100)):
        slabs = plan_slabs(n, step)
        cover = torch.zeros(n, dtype=torch.int64)
        for b, c in slabs:
            assert c >= 1
            cover[b:b + c] += 1
        assert torch.equal(cover, torch.ones(n, dtype=torch.int64))
        assert [b for b, _ in slabs] == sorted(b for b, _ in slabs)
    with pytest.raises(ValueError):
        plan_slabs(0)
    with pytest.raises(ValueError):
        plan_slabs(8, 0)


def test_pooling_order_is_torch_cpu_avgpool3d():
    """The reference pools on the CPU (field_utils.py:282-283,314-315).  Its summation order, read off torch here
    rather than assumed: from 0, first index outermost, last innermost, then / 8 -- ``pool2`` (and the kernel) use it.
    Other orders give other bits on values of wide dynamic range."""
    from quadraturefields_amd.field_utils import pool2
    g = torch.Generator().manual_seed(0)
    t = torch.randn(32, 32, 32, generator=g) * torch.exp(6 * torch.randn(32, 32, 32, generator=g))
    want = F.avg_pool3d(t[None, None], 2, 2)[0, 0]
    assert torch.equal(pool2(t), want)
    v = t.reshape(16, 2, 16, 2, 16, 2)
    s = torch.zeros(16, 16, 16)
    for dz, dy, dx in itertools.product(range(2), repeat=3):        # last index outermost: differs
        s += v[:, dx, :, dy, :, dz]
    assert not torch.equal(s / 8, want)


def test_host_tensors_are_refused():
    from quadraturefields_amd import field_utils
    from quadraturefields_amd.field import Field
    f = Field(**dict(STAGE2, log2_T=12))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        field_utils.field_grids(f, grid_size=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        field_utils.density_grid(f, 0.5, grid_size=4)
