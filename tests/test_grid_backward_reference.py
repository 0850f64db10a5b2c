"""Pins tests/grid_backward_reference.py (the float64 reference of the hash-grid backward) on the CPU: it must equal
float64 torch.autograd of a trilinear forward on the same corner rows, its fmaf emulation must be the correctly rounded
fmaf, and the route-edge configs of tests/test_gpu_grid_backward.py must sit on the edges of csrc/grid_backward.hip."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from quadraturefields_amd import _C
from tests import grid_backward_reference as R

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quadraturefields_amd", "csrc",
                   "grid_backward.hip")


@pytest.fixture(autouse=True)
def _autograd_on():
    with torch.enable_grad():
        yield


def _f32(v):
    return float(np.float32(v))


def _round_f32(q: Fraction) -> float:
    """Round an exact rational to the nearest fp32, ties to even (normal range)."""
    if q == 0:
        return 0.0
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    ulp = Fraction(2) ** (e - 23)
    m = a / ulp
    lo = m.numerator // m.denominator
    rem = m - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    r = float(lo * ulp)
    return r if q > 0 else -r


def _fma_exact(scale, x):
    return _round_f32(Fraction(scale) * Fraction(x) + Fraction(1, 2))


def _desc(log2_t, base, b):
    return _C.make_grid_desc(16, log2_t, base, b)


def test_fmaf_emulation_is_the_correctly_rounded_fma(lib):
    # scale * x = 2^-25 + 4688 * 2^-71: float64 rounds 0.5 + that onto the fp32 tie 0.5 + 2^-25, whose even neighbour
    # 0.5 is wrong; the exact sum is above the tie, so fmaf gives 0.5 + 2^-24
    s_dr, x_dr = 1 + 2896 * 2.0 ** -23, 2.0 ** -25 * (1 - 2895 * 2.0 ** -23)
    assert float(np.float32(np.float64(s_dr) * np.float64(x_dr) + 0.5)) == 0.5
    assert _fma_exact(s_dr, x_dr) == 0.5 + 2.0 ** -24
    scales = [1.0, 15.0, 107.0, _f32(2047.9999), s_dr] + [float(v) for v in _desc(19, 16, 1.447269237440378).scale]
    xs = [0.0, 1.0, -0.0, 2.0 ** -30, -(2.0 ** -30), 2.0 ** -149, _f32(1e-7), _f32(-1e-3), _f32(1.02), x_dr,
          _f32(0.5), _f32(1 / 3)]
    g = np.random.default_rng(0)
    # near-ties: x with scale * x just off (and on) an fp32 midpoint around 0.5, and random x in [-0.05, 1.05]
    for s in scales:
        for j in (1, 3, 5):
            xs.append(_f32(j * 2.0 ** -25 / s))
            xs.append(float(np.nextafter(np.float32(j * 2.0 ** -25 / s), np.float32(1))))
    xs += [float(v) for v in g.uniform(-0.05, 1.05, 200).astype(np.float32)]
    xs += [float(v) for v in (g.uniform(-1, 1, 200) * 2.0 ** -g.integers(7, 40, 200)).astype(np.float32)]
    xt = torch.tensor(xs, dtype=torch.float32)
    for s in scales:
        s = _f32(s)
        got = R.fmaf32(s, xt).tolist()
        want = [_fma_exact(s, x) for x in xs]
        assert got == want, s


def _small_inputs(n, lvs, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g)
    x[: n // 10] = x[: n // 10] * 1.04 - 0.02                    # some points outside [0, 1]
    if n >= 8:
        x[1, :] = 0.0
        x[2, :] = 1.0
        x[3, 0] = (3 + 0.5) / lvs[0].scale                       # on a cell face of level 0 (up to rounding)
        x[4, :] = 2.0 ** -30
    rows = lvs[-1].offset + lvs[-1].rows
    table = torch.randn(rows, 2, generator=g)
    dfeat = torch.randn(n, 32, generator=g)
    dfeat[2::5] = 0.0
    dfeat[1::7, 3] = 0.0
    v = torch.randn(n, 3, generator=g)
    v[::4, 1] = 0.0
    return x.float().contiguous(), table.float().contiguous(), dfeat.float().contiguous(), v.float().contiguous()


def _autograd_case(desc, n, seed):
    lvs = R.levels_of(desc)
    x, table, dfeat, v = _small_inputs(n, lvs, seed)
    idx_frac = [(lv,) + R.level_corners(x, lv) for lv in lvs]
    xd = x.double().requires_grad_(True)
    td = table.double().requires_grad_(True)
    dd = dfeat.double().requires_grad_(True)
    feat = R.trilinear_forward_fp64(xd, td, idx_frac)
    loss = (feat * dd).sum()
    g_t, g_x = torch.autograd.grad(loss, [td, xd], create_graph=True)
    second = torch.autograd.grad((g_x * v.double()).sum(), [dd, xd, td])
    return lvs, (x, table, dfeat, v), (g_t, g_x), second


def _close(pair, want):
    val, mag = pair
    want = want.detach().reshape(val.shape)
    assert torch.all(mag >= val.abs() * (1 - 1e-12))
    assert torch.allclose(val, want, rtol=1e-11, atol=1e-13 * float(mag.max()) + 1e-300)


DESCS = {"dense+hashed": (12, 4, 1.5), "ngp-like": (14, 16, 1.447269237440378), "all-dense": (21, 100, 1.01)}


@pytest.mark.parametrize("name", sorted(DESCS))
@pytest.mark.parametrize("n", [1, 37, 200])
def test_reference_equals_fp64_autograd(lib, name, n):
    desc = _desc(*DESCS[name])
    lvs, (x, table, dfeat, v), (g_t, g_x), (s_d, s_x, s_t) = _autograd_case(desc, n, seed=n)
    if name == "dense+hashed":
        assert 0 < int(desc.hashed_mask) < (1 << 16) - 1          # both kinds of level
    ref = R.grid_backward_ref(desc, x, table, dfeat)
    _close(ref["grad_table"], g_t)
    _close(ref["dx"], g_x)
    ref2 = R.grid_double_backward_ref(desc, x, table, dfeat, v)
    _close(ref2["g_dfeat"], s_d)
    _close(ref2["g_x"], s_x)
    _close(ref2["grad_table"], s_t)
    # k: at most 8 (point, corner) terms per point and level, and a row has terms iff it has a magnitude
    for r in (ref, ref2):
        assert 0 < int(r["k"].sum()) <= 8 * 16 * n
        assert torch.equal(r["k"] > 0, r["grad_table"][1].sum(1) > 0)


def test_corner_rows_wrap_and_hash_like_the_kernel(lib):
    """Spot values of level_corners worked out by hand from field_common.h: the dense wrap at x01 = 1 and for a point
    below 0 ((uint32)(int32) of a negative floor), and the uint32 hash."""
    dense = R.Level(offset=10, rows=64, res=4, scale=3.0, hashed=False)
    idx, frac = R.level_corners(torch.tensor([[1.0, 1.0, 1.0], [-0.25, 0.0, 0.0]]), dense)
    # x = 1: pos 3.5, cell 3; corner (4,4,4) = 4 + 16 + 64 = 84 -> 84 % 64 = 20
    assert idx[0, 7].item() == 10 + 20 and idx[0, 0].item() == 10 + (3 + 12 + 48) % 64
    assert frac[0].tolist() == [0.5, 0.5, 0.5]
    # x = -0.25: pos -0.25, floor -1 -> 0xFFFFFFFF; corner 0 = (2^32 - 1) + 0 + 0 -> % 64 = 63, corner 1 = 0
    assert idx[1, 0].item() == 10 + (2 ** 32 - 1) % 64 and idx[1, 1].item() == 10
    assert frac[1, 0].item() == 0.75
    hashed = R.Level(offset=0, rows=1 << 10, res=300, scale=299.0, hashed=True)
    x = torch.tensor([[0.3, 0.6, 0.9]])
    idx, _ = R.level_corners(x, hashed)
    cx, cy, cz = (int(np.floor(np.float32(299.0) * np.float32(v) + np.float32(0.5))) for v in (0.3, 0.6, 0.9))
    want = ((cx + 1) ^ ((cy * R.PRIME_Y) & R.MASK32) ^ (((cz + 1) * R.PRIME_Z) & R.MASK32)) & 1023
    assert idx[0, 5].item() == want


def _consts():
    src = open(SRC).read()
    c = {k: int(v) for k, v in re.findall(r"constexpr int (k\w+) = (\d+);", src)}
    thresholds = re.findall(r"n (?:<|>=) \(1 << (\d+)\)", src)
    return c, thresholds


def test_route_constants_are_the_sources():
    c, thresholds = _consts()
    assert c["kLdsRows"] == R.LDS_ROWS
    assert c["kMaxLdsParts"] == R.MAX_LDS_PARTS
    assert c["kScatterThreads"] == R.SCATTER_THREADS
    assert c["kScatterUnroll"] == R.SCATTER_UNROLL
    # the first-order and the second-order entry points switch at the same batch size
    assert len(thresholds) == 2 and all(1 << int(t) == R.LDS_MIN_N for t in thresholds)


def _level_table(desc):
    return [(lv.res, lv.rows, lv.hashed, R.parts(lv.rows), lv.rows % R.LDS_ROWS) for lv in R.levels_of(desc)]


def test_route_edge_configs_sit_on_their_edges(lib):
    # qf_grid_desc_init's all-dense config: 50 partitions exactly, 63 (walk) and 65 (atomics)
    edges = _level_table(_desc(*R.init_args("edges")))
    assert all(not h for _, _, h, _, _ in edges)
    by_res = {r: (rows, p, tail) for r, rows, _, p, tail in edges}
    assert by_res[100] == (1000000, 50, 0)
    assert by_res[108][1] == 63 and by_res[109][1] == 65
    assert any(p <= R.MAX_LDS_PARTS for *_, p, _ in edges) and any(p > R.MAX_LDS_PARTS for *_, p, _ in edges)
    assert all(p != R.MAX_LDS_PARTS for *_, p, _ in edges)          # the init rule skips 64: the hand desc has it
    # the hand-edited desc: exactly 64 partitions, 65 with a last partition of 8 rows, a walked level whose last
    # partition holds 8 rows; every level passes fill_grid_args
    hand = _level_table(R.hand_desc(_C.GridDesc))
    assert (109, 64 * R.LDS_ROWS, False, 64, 0) in hand and (108, 64 * R.LDS_ROWS, False, 64, 0) in hand
    assert (109, 64 * R.LDS_ROWS + 8, False, 65, 8) in hand
    assert (100, 50 * R.LDS_ROWS + 8, False, 51, 8) in hand
    for res, rows, hashed, _, _ in hand:
        assert (rows & (rows - 1)) == 0 if hashed else res * res <= rows
    assert 109 ** 3 > 64 * R.LDS_ROWS                               # its upper corner rows wrap
    # the deformation field's reference table: dense levels 0-10 (up to 9.5 M rows; the walk takes levels 0-7, levels
    # 8-10 have 103 to 477 partitions), every hashed level has 839 partitions: quad atomics
    f24 = _level_table(_desc(*R.init_args("field24")))
    assert [h for _, _, h, _, _ in f24] == [False] * 11 + [True] * 5
    assert f24[-1][1] == 1 << 24 and R.parts(1 << 24) == 839
    assert 9_000_000 < max(rows for _, rows, h, _, _ in f24 if not h) < 10_000_000
    assert sum(rows for _, rows, _, _, _ in f24) > 100_000_000
    assert [p <= R.MAX_LDS_PARTS for *_, p, _ in f24] == [True] * 8 + [False] * 8
    # NGP / Field at T = 2^19: every level walks; NGP at 2^21: the hashed levels take the atomics
    assert all(p <= R.MAX_LDS_PARTS for *_, p, _ in _level_table(_desc(*R.init_args("ngp19"))))
    assert all(p <= R.MAX_LDS_PARTS for *_, p, _ in _level_table(_desc(*R.init_args("field19"))))
    n21 = _level_table(_desc(*R.init_args("ngp21")))
    assert any(p > R.MAX_LDS_PARTS for *_, p, _ in n21) and any(p <= R.MAX_LDS_PARTS for *_, p, _ in n21)


def test_scatter_plan_matches_table_scatter_ws():
    """scatter_plan restates table_scatter_ws's chunking (the GPU test places its probes by it)."""
    src = open(SRC).read()
    assert "3 * qf_cu_count_cached() / 8 > 16 ? 3 * qf_cu_count_cached() / 8 : 16" in src
    assert "int chunks = (per_level + parts / 2) / parts;" in src
    lvs = [R.Level(0, 4096, 16, 15.0, False), R.Level(0, 1 << 19, 100, 99.0, True),
           R.Level(0, 65 * R.LDS_ROWS, 109, 108.0, False)]
    assert R.scatter_plan(lvs, 256) == [(True, 1, 96), (True, 27, 4), (False, 65, 1)]
