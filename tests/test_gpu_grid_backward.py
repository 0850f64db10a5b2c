"""The hash-grid backward (csrc/grid_backward.hip: qf_grid_encode_backward, qf_grid_encode_backward_ws,
qf_grid_encode_double_backward) against the float64 reference of tests/grid_backward_reference.py, on both table
scatter routes -- the quad atomics and the LDS-partitioned walk -- and at their edges.

Bar, per element, with M the reference's sum over absolute values of every factor, u = 2^-24 and k the number of
terms: |got - ref| <= (k + 8) u M.  A table row's k is the number of (point, corner) terms that land in it (+1 for a
non-zero initial value, which is part of the sum); a per-point output's k is the fixed number of terms of its sum
(R.K_DX, R.K_GX, R.K_GDFEAT).  Each term is a product with at most 8 fp32 roundings (1 - frac, the products, the
three-term D of the second order, the scale), and any order of adding k of them -- atomic arrival order, LDS partial
sums flushed with atomics -- adds at most (k - 1) u of their absolute sum: the bound is rigorous, not fitted, and holds
for every summation order.  A row with M = 0 must be exactly 0, which catches terms that leak into the wrong level or
row.  Max err / (u M) of each check is printed as an ERR_RATIO line (and appended to $QF_ERR_RATIO_LOG when set).
"""
import ctypes
import os

import pytest
import torch

from quadraturefields_amd import _C
from tests import grid_backward_reference as R

pytestmark = pytest.mark.gpu

U = R.U
SIZES = ["1", "63", "65", "2^15-1", "2^15", "2^15+8193", "2^20+5"]
SENTINEL = 0x5A


def _n(expr):
    return int(eval(expr.replace("^", "**")))


def _report(case, name, value):
    print(f"ERR_RATIO grid {case} {name} {value:.3g}")
    path = os.environ.get("QF_ERR_RATIO_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"grid {case} {name} {value:.6g}\n")


def _desc(name):
    if name == "hand":
        return R.hand_desc(_C.GridDesc)
    log2_t, base, b = R.init_args(name)
    return _C.make_grid_desc(16, log2_t, base, b)


def _rows(desc):
    return int(desc.offset[16])


@pytest.fixture(scope="module")
def cu(lib, device):
    c = lib.qf_device_cu_count()
    assert c > 0
    return c


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _inputs(desc, n, device, seed):
    """x01 with points on cell faces, at 0 and 1, tiny, and 5 % slightly outside [0, 1]; dfeat with all-zero rows and
    rows zero in one feature of a level; v with zero components; a table at grid-parameter scale."""
    g = _gen(device, seed)
    lvs = R.levels_of(desc)
    x = torch.rand(n, 3, generator=g, device=device)
    pick = lambda frac: torch.rand(n, generator=g, device=device) < frac          # noqa: E731
    out = pick(0.05)
    side = torch.rand(n, 3, generator=g, device=device)
    nudge = torch.rand(n, 3, generator=g, device=device) * 0.02
    xo = torch.where(side < 0.5, -nudge, 1.0 + nudge)
    x = torch.where(out[:, None] & (torch.rand(n, 3, generator=g, device=device) < 0.5), xo, x)
    face = pick(0.05)                                 # on cell faces of a random level: pos = m + 1 (frac 0 or ~1)
    lvl = torch.randint(0, 16, (n,), generator=g, device=device)
    sc = torch.tensor([lv.scale for lv in lvs], device=device, dtype=torch.float64)[lvl]
    m = torch.floor(torch.rand(n, 3, generator=g, device=device, dtype=torch.float64) * sc[:, None])
    x = torch.where(face[:, None], ((m + 0.5) / sc[:, None]).float(), x)
    x = torch.where(pick(0.01)[:, None], torch.zeros_like(x), x)
    x = torch.where(pick(0.01)[:, None], torch.ones_like(x), x)
    x = torch.where(pick(0.01)[:, None], torch.full_like(x, 2.0 ** -30), x)
    if n >= 4:
        x[0], x[1], x[n - 1] = 0.0, 1.0, 2.0 ** -27
    dfeat = torch.randn(n, 32, generator=g, device=device)
    dfeat[pick(0.1)] = 0.0
    dfeat[torch.rand(n, 32, generator=g, device=device) < 0.05] = 0.0             # one feature of a level
    v = torch.randn(n, 3, generator=g, device=device)
    v[torch.rand(n, 3, generator=g, device=device) < 0.1] = 0.0
    table = (torch.rand(_rows(desc), 2, generator=g, device=device) * 2 - 1) * 1e-1
    return x.contiguous(), table.contiguous(), dfeat.contiguous(), v.contiguous()


def _g0(rows, device, seed):
    """A non-zero initial gradient on half the rows: the kernels must add to it."""
    g = _gen(device, seed)
    t = torch.randn(rows, 2, generator=g, device=device) * 1e-2
    t[torch.rand(rows, generator=g, device=device) < 0.5] = 0.0
    return t


def check(case, name, got, pair, k, g0=None):
    """|got - ref| <= (k + 8) u M elementwise; rows / elements with M = 0 must be exactly 0."""
    val, mag = pair
    if g0 is not None:
        val = val + g0.double()
        mag = mag + g0.double().abs()
        k = k + 1
    if isinstance(k, torch.Tensor):
        k = k.double().reshape(-1, *([1] * (val.dim() - 1)))
    got = got.reshape(val.shape)
    assert bool(torch.isfinite(got).all()), f"{case} {name}: non-finite output"
    err = (got.double() - val).abs()
    bar = (k + 8) * U * mag
    bad = err > bar
    nbad = int(bad.sum())
    if nbad:
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{case} {name}: {nbad} elements over the bar; first at flat {i}: got "
                             f"{float(got.reshape(-1)[i])!r} ref {float(val.reshape(-1)[i])!r} M "
                             f"{float(mag.reshape(-1)[i])!r} bar {float(bar.reshape(-1)[i])!r}")
    pos = mag > 0
    ratio = float((err[pos] / (U * mag[pos])).max()) if bool(pos.any()) else 0.0
    _report(case, name, ratio)
    return ratio


# --- the C entry points ----------------------------------------------------------------------------------------------

def _ws(lib, n, device, short=0):
    need = int(lib.qf_grid_backward_workspace_bytes(n))
    ws = torch.full((max(need, 1),), SENTINEL, dtype=torch.uint8, device=device)
    return ws, need - short


def _walked(ws):
    """Did the LDS walk run?  It writes the level-major copy of dfeat into the workspace; the atomics never touch it."""
    return not bool((ws == SENTINEL).all())


def bwd_atomic(lib, desc, table, x, dfeat, gt, dx):
    rc = lib.qf_grid_encode_backward(ctypes.byref(desc), _C.ptr(table), _C.ptr(x), _C.ptr(dfeat), x.shape[0],
                                     _C.ptr(gt), _C.ptr(dx), _C.stream())
    assert rc == 0, rc


def bwd_ws(lib, desc, table, x, dfeat, gt, dx, short=0):
    ws, nbytes = _ws(lib, x.shape[0], x.device, short)
    rc = lib.qf_grid_encode_backward_ws(ctypes.byref(desc), _C.ptr(table), _C.ptr(x), _C.ptr(dfeat), x.shape[0],
                                        _C.ptr(gt), _C.ptr(dx), _C.ptr(ws), nbytes, _C.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return _walked(ws)


def dbl(lib, desc, table, x, dfeat, v, g_d, g_x, gt, ws_mode=None):
    """ws_mode None: no workspace; 0: exactly the workspace size; 1: one byte short.  Returns whether the walk ran."""
    ws, nbytes = (None, 0) if ws_mode is None else _ws(lib, x.shape[0], x.device, ws_mode)
    rc = lib.qf_grid_encode_double_backward(ctypes.byref(desc), _C.ptr(table), _C.ptr(x), _C.ptr(dfeat), _C.ptr(v),
                                            x.shape[0], _C.ptr(g_d), _C.ptr(g_x), _C.ptr(gt), _C.ptr(ws), nbytes,
                                            _C.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return ws is not None and _walked(ws)


def _expect_walk(desc, n, cu):
    return n >= R.LDS_MIN_N and any(w for w, _, _ in R.scatter_plan(R.levels_of(desc), cu))


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


# --- full batches ----------------------------------------------------------------------------------------------------

CONFIGS = ["ngp19", "ngp21", "field19", "edges", "hand"]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("config", CONFIGS)
def test_first_order_vs_fp64(lib, device, cu, config, size):
    """Table and input gradient, quad atomics from zero and the workspace route (the LDS walk from 2^15 points on)
    onto a non-zero initial gradient."""
    n = _n(size)
    desc = _desc(config)
    x, table, dfeat, _ = _inputs(desc, n, device, seed=n + len(config))
    ref = R.grid_backward_ref(desc, x, table, dfeat)
    case = f"{config} n={size}"
    gt, dx = torch.zeros_like(table), _nan((n, 3), device)
    bwd_atomic(lib, desc, table, x, dfeat, gt, dx)
    check(case, "grad_table atomic", gt, ref["grad_table"], ref["k"])
    check(case, "dx", dx, ref["dx"], R.K_DX)
    g0 = _g0(table.shape[0], device, n)
    gt, dx = g0.clone(), _nan((n, 3), device)
    assert bwd_ws(lib, desc, table, x, dfeat, gt, dx) == _expect_walk(desc, n, cu)
    check(case, "grad_table ws", gt, ref["grad_table"], ref["k"], g0=g0)
    check(case, "dx ws", dx, ref["dx"], R.K_DX)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("config", ["ngp19", "field19", "edges", "hand"])
def test_second_order_vs_fp64(lib, device, cu, config, size):
    """g_dfeat, g_x and the table term without a workspace (quad atomics, onto zero), then the table term through the
    workspace route (the kSecond LDS walk from 2^15 points on) onto a non-zero initial gradient."""
    n = _n(size)
    desc = _desc(config)
    x, table, dfeat, v = _inputs(desc, n, device, seed=3 * n + len(config))
    ref = R.grid_double_backward_ref(desc, x, table, dfeat, v)
    case = f"{config} n={size}"
    g_d, g_x, gt = _nan((n, 32), device), _nan((n, 3), device), torch.zeros_like(table)
    assert not dbl(lib, desc, table, x, dfeat, v, g_d, g_x, gt)
    check(case, "g_dfeat", g_d, ref["g_dfeat"], R.K_GDFEAT)
    check(case, "g_x", g_x, ref["g_x"], R.K_GX)
    check(case, "grad_table2 atomic", gt, ref["grad_table"], ref["k"])
    g0 = _g0(table.shape[0], device, n + 1)
    gt = g0.clone()
    assert dbl(lib, desc, table, x, dfeat, v, None, None, gt, ws_mode=0) == _expect_walk(desc, n, cu)
    check(case, "grad_table2 ws", gt, ref["grad_table"], ref["k"], g0=g0)


@pytest.mark.parametrize("order", [1, 2])
def test_deformation_reference_table_log2_t_24(lib, device, cu, order):
    """The deformation field's reference table (101.6 M rows, dense levels 0-10 walked, hashed levels 839 partitions
    each: quad atomics) at a training batch: the touched rows against the reference, then every other row of the
    813 MB gradient exactly zero."""
    n = _n("2^20+5")
    desc = _desc("field24")
    x, table, dfeat, v = _inputs(desc, n, device, seed=24 + order)
    ref = (R.grid_backward_ref(desc, x, table, dfeat) if order == 1
           else R.grid_double_backward_ref(desc, x, table, dfeat, v))
    touched = ref["k"] > 0
    k = ref["k"][touched]
    pair = (ref["grad_table"][0][touched], ref["grad_table"][1][touched])
    for route in ("atomic", "ws"):
        gt = torch.zeros_like(table)
        if order == 1:
            dx = _nan((n, 3), device)
            if route == "atomic":
                bwd_atomic(lib, desc, table, x, dfeat, gt, dx)
            else:
                assert bwd_ws(lib, desc, table, x, dfeat, gt, dx)
            check(f"field24 o{order}", f"dx {route}", dx, ref["dx"], R.K_DX)
        else:
            g_d, g_x = _nan((n, 32), device), _nan((n, 3), device)
            assert dbl(lib, desc, table, x, dfeat, v, g_d, g_x, gt, ws_mode=None if route == "atomic" else 0) == (route == "ws")
            check(f"field24 o{order}", f"g_dfeat {route}", g_d, ref["g_dfeat"], R.K_GDFEAT)
            check(f"field24 o{order}", f"g_x {route}", g_x, ref["g_x"], R.K_GX)
        check(f"field24 o{order}", f"grad_table touched {route}", gt[touched], pair, k)
        gt[touched] = 0.0
        assert int(torch.count_nonzero(gt)) == 0, route
        del gt


# --- sparse probes ---------------------------------------------------------------------------------------------------

def _probe_points(desc, n, cu):
    """Point indices that the walk of each level handles at its edges: the first and last point of the first and
    last point chunk, the last unrolled slot of the first trip and of the last trip that has one."""
    pts = set()
    span = R.SCATTER_UNROLL * R.SCATTER_THREADS
    last_slot = (R.SCATTER_UNROLL - 1) * R.SCATTER_THREADS
    for walk, _, chunks in R.scatter_plan(R.levels_of(desc), cu):
        for c in {0, chunks - 1}:
            lo, hi = n * c // chunks, n * (c + 1) // chunks
            if hi <= lo:
                continue
            pts.update((lo, hi - 1))
            for t in (0, R.SCATTER_THREADS - 1):
                if lo + last_slot + t < hi:
                    pts.add(lo + last_slot + t)
            j = (hi - 1 - lo - last_slot) // span
            if j >= 0:
                pts.add(lo + j * span + last_slot)
    return sorted(pts)


def _boundary_points(desc, lv_i):
    """Positions in a dense level whose corner rows straddle partition boundaries (first and last boundary)."""
    lv = R.levels_of(desc)[lv_i]
    xs = []
    nparts = R.parts(lv.rows)
    for q in sorted({1, nparts - 1}):
        if q < 1 or q * R.LDS_ROWS >= lv.rows:
            continue
        for v0 in (q * R.LDS_ROWS - 1, q * R.LDS_ROWS - lv.res, q * R.LDS_ROWS - lv.res * lv.res):
            if v0 < 0:
                continue
            c = (v0 % lv.res, (v0 // lv.res) % lv.res, v0 // (lv.res * lv.res))
            xs.append([(ci + 0.25) / lv.scale for ci in c])
    return xs


PROBE_CASES = [("ngp19", None), ("edges", None), ("hand", None), ("edges", 0), ("edges", 7), ("edges", 8),
               ("hand", 6), ("hand", 7), ("hand", 14), ("ngp21", 15)]


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("config,level", PROBE_CASES)
def test_sparse_probes(lib, device, cu, config, level, order):
    """dfeat (and v) zero except on a few dozen points at the walk's edges, the dense levels' probes on corner rows
    straddling partition boundaries; level set: dfeat non-zero in that level only, every other level's rows must stay
    exactly 0.  With k <= a few, a lost, doubled or misrouted term is many times the bar."""
    n = _n("2^20+5")
    desc = _desc(config)
    lvs = R.levels_of(desc)
    x, table, dfeat, v = _inputs(desc, n, device, seed=7 + order)
    pts = _probe_points(desc, n, cu)
    dense = [i for i, lv in enumerate(lvs) if not lv.hashed and R.parts(lv.rows) > 1 and (level is None or i == level)]
    bpts = [xy for i in dense for xy in _boundary_points(desc, i)]
    free = [p for p in range(1, n - 1, 4099) if p not in set(pts)][:len(bpts)]
    for p, xy in zip(free, bpts):
        x[p] = torch.tensor(xy, device=device)
    pts = sorted(set(pts) | set(free))
    assert 12 <= len(pts) <= 400
    keep = torch.zeros(n, dtype=torch.bool, device=device)
    keep[pts] = True
    dfeat = torch.where(keep[:, None], dfeat, torch.zeros_like(dfeat))
    dfeat[pts] = torch.where(dfeat[pts] == 0, torch.ones_like(dfeat[pts]), dfeat[pts])      # every probe term counts
    if level is not None:
        lvmask = torch.zeros(32, dtype=torch.bool, device=device)
        lvmask[2 * level:2 * level + 2] = True
        dfeat = dfeat * lvmask
    v = torch.where(keep[:, None], v, torch.zeros_like(v))
    # the boundary probes really straddle their partition boundary
    for i in dense:
        idx, _ = R.level_corners(x[free], lvs[i])
        part = (idx - lvs[i].offset) // R.LDS_ROWS
        assert bool((part.max(1).values > part.min(1).values).any()), (config, i)
    ref = (R.grid_backward_ref(desc, x, table, dfeat) if order == 1
           else R.grid_double_backward_ref(desc, x, table, dfeat, v))
    assert int(ref["k"][ref["grad_table"][1].sum(1) > 0].max()) <= 24
    case = f"probe o{order} {config} level={'all' if level is None else level}"
    for route in ("atomic", "ws"):
        gt = torch.zeros_like(table)
        if order == 1:
            if route == "atomic":
                bwd_atomic(lib, desc, table, x, dfeat, gt, None)
            else:
                assert bwd_ws(lib, desc, table, x, dfeat, gt, None)
        else:
            assert dbl(lib, desc, table, x, dfeat, v, None, None, gt, ws_mode=None if route == "atomic" else 0) == (route == "ws")
        check(case, f"grad_table {route}", gt, ref["grad_table"], ref["k"])
        if level is not None:
            out = torch.ones(table.shape[0], dtype=torch.bool, device=device)
            out[lvs[level].offset:lvs[level].offset + lvs[level].rows] = False
            assert int(torch.count_nonzero(gt[out])) == 0, route


# --- contracts -------------------------------------------------------------------------------------------------------

def test_workspace_short_by_one_byte_takes_the_quad_atomics(lib, device, cu):
    desc = _desc("ngp19")
    for n in (_n("2^15+8193"), _n("2^15-1")):
        x, table, dfeat, v = _inputs(desc, n, device, seed=11)
        ref = R.grid_backward_ref(desc, x, table, dfeat)
        ref2 = R.grid_double_backward_ref(desc, x, table, dfeat, v)
        for short in (1, 0):
            walk = short == 0 and n >= R.LDS_MIN_N
            gt = torch.zeros_like(table)
            assert bwd_ws(lib, desc, table, x, dfeat, gt, None, short=short) == walk, (n, short)
            check(f"ws short={short} n={n}", "grad_table", gt, ref["grad_table"], ref["k"])
            gt = torch.zeros_like(table)
            assert dbl(lib, desc, table, x, dfeat, v, None, None, gt, ws_mode=short) == walk, (n, short)
            check(f"ws short={short} n={n}", "grad_table2", gt, ref2["grad_table"], ref2["k"])


def test_quad_atomics_add_into_grad_table(lib, device):
    """Both orders through the quad atomics add to a non-zero initial gradient (the walk's case is in the full-batch
    tests)."""
    desc = _desc("hand")
    n = _n("2^15+8193")
    x, table, dfeat, v = _inputs(desc, n, device, seed=12)
    g0 = _g0(table.shape[0], device, 12)
    gt = g0.clone()
    bwd_atomic(lib, desc, table, x, dfeat, gt, None)
    ref = R.grid_backward_ref(desc, x, table, dfeat)
    check("accumulate o1", "grad_table atomic", gt, ref["grad_table"], ref["k"], g0=g0)
    ref2 = R.grid_double_backward_ref(desc, x, table, dfeat, v)
    gt = g0.clone()
    dbl(lib, desc, table, x, dfeat, v, None, None, gt)
    check("accumulate o2", "grad_table atomic", gt, ref2["grad_table"], ref2["k"], g0=g0)


@pytest.mark.parametrize("outputs", ["g_dfeat", "g_x", "grad_table", "all"])
@pytest.mark.parametrize("size", ["65", "2^15+8193"])
def test_double_backward_output_subsets(lib, device, outputs, size):
    n = _n(size)
    desc = _desc("edges")
    x, table, dfeat, v = _inputs(desc, n, device, seed=13)
    ref = R.grid_double_backward_ref(desc, x, table, dfeat, v)
    want = {"g_dfeat", "g_x", "grad_table"} if outputs == "all" else {outputs}
    g_d = _nan((n, 32), device) if "g_dfeat" in want else None
    g_x = _nan((n, 3), device) if "g_x" in want else None
    gt = torch.zeros_like(table) if "grad_table" in want else None
    dbl(lib, desc, table, x, dfeat, v, g_d, g_x, gt, ws_mode=0)
    case = f"subset {outputs} n={size}"
    if g_d is not None:
        check(case, "g_dfeat", g_d, ref["g_dfeat"], R.K_GDFEAT)
    if g_x is not None:
        check(case, "g_x", g_x, ref["g_x"], R.K_GX)
    if gt is not None:
        check(case, "grad_table2", gt, ref["grad_table"], ref["k"])


def test_zero_points_write_nothing(lib, device):
    desc = _desc("ngp19")
    x, table, dfeat, v = _inputs(desc, 8, device, seed=14)
    gt = torch.full_like(table, 3.0)
    dx, g_d, g_x = torch.full((8, 3), 3.0, device=device), torch.full((8, 32), 3.0, device=device), torch.full((8, 3), 3.0, device=device)
    ws = torch.full((1 << 20,), SENTINEL, dtype=torch.uint8, device=device)
    d = ctypes.byref(desc)
    P = _C.ptr
    assert lib.qf_grid_encode_backward(d, P(table), P(x), P(dfeat), 0, P(gt), P(dx), _C.stream()) == 0
    assert lib.qf_grid_encode_backward_ws(d, P(table), P(x), P(dfeat), 0, P(gt), P(dx), P(ws), 1 << 20,
                                          _C.stream()) == 0
    assert lib.qf_grid_encode_double_backward(d, P(table), P(x), P(dfeat), P(v), 0, P(g_d), P(g_x), P(gt), P(ws),
                                              1 << 20, _C.stream()) == 0
    torch.cuda.synchronize()
    for t in (gt, dx, g_d, g_x):
        assert bool((t == 3.0).all())
    assert not _walked(ws)


# --- the autograd routes ---------------------------------------------------------------------------------------------

def test_encoding_autograd_first_and_second_order(lib, device):
    """tinycudann.Encoding: _GridEncodeFn's backward (table and input gradient) and _GridInputGradFn's backward
    (create_graph=True: g_dfeat, g_x and the table term) at a batch that takes the walk."""
    from oracle import fields as ofields
    from quadraturefields_amd import tinycudann as tcnn
    n = _n("2^15+8193")
    enc = tcnn.Encoding(3, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19,
                            "base_resolution": 16, "per_level_scale": ofields.ngp_per_level_scale(4096, 16, 16)}).to(device)
    desc = enc.grid.desc
    x, _, dfeat, v = _inputs(desc, n, device, seed=15)
    table = enc.params.detach().reshape(-1, 2)
    ref = R.grid_backward_ref(desc, x, table, dfeat)
    ref2 = R.grid_double_backward_ref(desc, x, table, dfeat, v)
    with torch.enable_grad():
        xg = x.clone().requires_grad_(True)
        (enc(xg) * dfeat).sum().backward()
        check("Encoding o1", "params.grad", enc.params.grad, ref["grad_table"], ref["k"])
        check("Encoding o1", "x.grad", xg.grad, ref["dx"], R.K_DX)
        enc.params.grad = None
        xg = x.clone().requires_grad_(True)
        dg = dfeat.clone().requires_grad_(True)
        gx, = torch.autograd.grad((enc(xg) * dg).sum(), [xg], create_graph=True)
        check("Encoding o2", "gx (forward)", gx.detach(), ref["dx"], R.K_DX)
        (gx * v).sum().backward()
        check("Encoding o2", "params.grad", enc.params.grad, ref2["grad_table"], ref2["k"])
        check("Encoding o2", "dfeat.grad", dg.grad, ref2["g_dfeat"], R.K_GDFEAT)
        check("Encoding o2", "x.grad", xg.grad, ref2["g_x"], R.K_GX)


def test_field_fused_backward_table_gradient(lib, device):
    """Field at the reference's scales (min_res 16, max_res 512, scale 1.5), log2_T 19: the table gradient of the
    fused training route (_DeformTrainFn) is the grid backward of its own d_enc."""
    from quadraturefields_amd.field import Field
    n = _n("2^15+8193")
    f = Field(scale=1.5, log2_T=19, L=16, max_res=512, min_res=16, hidden_size=32, nl="relu").to(device)
    desc = f.xyz_encoder.grid.desc
    assert list(desc.scale) == list(_desc("field19").scale)
    g = _gen(device, 16)
    x = ((torch.rand(n, 3, generator=g, device=device) * 2 - 1) * 1.5).contiguous()
    w = torch.randn(n, generator=g, device=device)
    with torch.enable_grad():
        (f.density(x)[:, 0] * w).sum().backward()
    got = f.xyz_encoder.params.grad
    # d_enc as _DeformTrainFn computes it (qf_deform_mlp_backward, checked against fp64 in test_gpu_mlp_backward.py)
    x01 = _C.f32c((x - f.xyz_min) / (f.xyz_max - f.xyz_min))
    table = f.xyz_encoder.params.detach().reshape(-1, 2).contiguous()
    enc = torch.empty((n, 32), device=device)
    f._density_fused(x, None, enc_out=enc, compute_dtype="fp32")
    d = f.decoder_field
    ws = [_C.f32c(t.detach()) for t in (d.layers[0].weight, d.layers[0].bias, d.layers[1].weight, d.layers[1].bias,
                                        d.lout.weight)]
    grads = [torch.zeros_like(t) for t in ws] + [torch.zeros_like(d.lout.bias)]
    d_enc = torch.empty((n, 32), device=device)
    _C.check(lib.qf_deform_mlp_backward(_C.ptr(enc), _C.ptr(x01), _C.ptr(w), *[_C.ptr(t) for t in ws], n,
                                        _C.ptr(d_enc), None, *[_C.ptr(t) for t in grads], _C.stream()), "mlp bwd")
    ref = R.grid_backward_ref(desc, x01, table, d_enc)
    check("Field o1", "params.grad", got, ref["grad_table"], ref["k"])
