"""Float64 reference of the hash-grid backward (csrc/grid_backward.hip), with error magnitudes and term counts.

The corner rows and fractional positions are the kernels' own (field_common.h: level_indices), taken bit for bit:
  * pos = fmaf(scale, x, 0.5) in fp32.  ``fmaf32`` emulates the single rounding exactly: the product of two fp32
    values is exact in float64, TwoSum gives the exact error of adding 0.5, and the one case where rounding the float64
    sum to fp32 could differ from rounding the exact sum -- the float64 sum sits on an fp32 tie while the exact sum
    does not -- is decided by the sign of that error.  (oracle.fields.hash_encode rounds twice, which differs when
    |scale * x| < 2^-6; the test inputs include such points, so the emulation is needed, not just convenient.)
  * floor, the (uint32)(int32) cast, uint32 hashing or dense strides with `% rows` wrap, all as uint32 arithmetic.
Each level's rows, res, scale and hashed bit come from the desc itself, so a hand-edited desc is honoured.

Everything after the indices is float64 on the inputs' device, one level at a time.  Every output comes with M, the same
sum over the absolute values of every factor, and the table outputs with k, the number of (point, corner) terms that
land in each row with a non-zero magnitude (a term whose magnitude is 0 has a zero factor: the kernels add an exact 0
for it, or skip it).  Any fp32 evaluation order of a sum of k terms, each a product of a few rounded factors, is within
(k + 8) u M of the exact value, u = 2^-24 (see tests/test_gpu_grid_backward.py).
"""
from dataclasses import dataclass

import torch

U = 2.0 ** -24
PRIME_Y = 2654435761
PRIME_Z = 805459861
MASK32 = 0xFFFFFFFF
N_LEVELS = 16

# fixed term counts of the per-point outputs (16 levels x 8 corners x 2 features, x 2 mixed axes for g_x; 8 corners
# x 3 axes for one g_dfeat element)
K_DX = 16 * 8 * 2
K_GX = 16 * 8 * 2 * 2
K_GDFEAT = 8 * 3


@dataclass
class Level:
    offset: int
    rows: int
    res: int
    scale: float          # the fp32 value, as a Python float
    hashed: bool


def levels_of(desc):
    """The per-level constants the kernels read (fill_grid_args), from a GridDesc."""
    return [Level(int(desc.offset[l]), int(desc.offset[l + 1]) - int(desc.offset[l]), int(desc.resolution[l]),
                  float(desc.scale[l]), bool((int(desc.hashed_mask) >> l) & 1)) for l in range(N_LEVELS)]


def fmaf32(scale: float, x: torch.Tensor, addend: float = 0.5) -> torch.Tensor:
    """fmaf(scale, x, addend) for fp32 scale and addend and an fp32 tensor x: one correctly rounded fp32 result."""
    p = x.double() * scale                              # exact: 24 x 24 significant bits
    s = p + addend
    bb = s - p
    e = (p - (s - bb)) + (addend - bb)                  # TwoSum: p + addend == s + e exactly
    f = s.float()
    fd = f.double()
    up = torch.nextafter(f, torch.full_like(f, float("inf")))
    dn = torch.nextafter(f, torch.full_like(f, float("-inf")))
    # s on the tie between f and a neighbour: the exact sum is off the tie by e, whose sign picks the side
    f = torch.where((s == (fd + up.double()) * 0.5) & (e > 0), up, f)
    f = torch.where((s == (fd + dn.double()) * 0.5) & (e < 0), dn, f)
    return f


def _mul32(a: torch.Tensor, b: int) -> torch.Tensor:
    """(a * b) mod 2^32 for int64 tensors a in [0, 2^32) and a constant b in [0, 2^32), without int64 overflow."""
    lo, hi = a & 0xFFFF, a >> 16
    return (lo * b + (((hi * b) & 0xFFFF) << 16)) & MASK32


def level_corners(x01: torch.Tensor, lv: Level):
    """Global table rows [n,8] (int64) of the 8 corners, corner bit d = upper cell along axis d, and frac [n,3] (fp32)."""
    pos = torch.stack([fmaf32(lv.scale, x01[:, d].float()) for d in range(3)], 1)
    fl = torch.floor(pos)
    frac = pos - fl                                     # exact in fp32
    g = fl.to(torch.int64) & MASK32                     # (uint32)(int32)floor
    c = [torch.stack([g[:, d], (g[:, d] + 1) & MASK32], 1) for d in range(3)]   # [n,2] per axis
    if lv.hashed:
        hy, hz = _mul32(c[1], PRIME_Y), _mul32(c[2], PRIME_Z)
    else:
        hy, hz = _mul32(c[1], lv.res), _mul32(c[2], (lv.res * lv.res) & MASK32)
    idx = []
    for k in range(8):
        a, b, z = c[0][:, k & 1], hy[:, (k >> 1) & 1], hz[:, k >> 2]
        if lv.hashed:
            v = (a ^ b ^ z) & (lv.rows - 1)
        else:
            v = (a + b + z) & MASK32
            v = torch.where(v >= lv.rows, v % lv.rows, v)
        idx.append(v + lv.offset)
    return torch.stack(idx, 1), frac


def _axis_factors(frac: torch.Tensor):
    """a[c] [n,8,3]: the linear factor of corner c along each axis (frac or 1 - frac, float64), s [8,3]: its sign."""
    f = frac.double()
    bits = torch.tensor([[(c >> d) & 1 for d in range(3)] for c in range(8)], device=frac.device, dtype=torch.bool)
    a = torch.where(bits[None], f[:, None, :], 1.0 - f[:, None, :])
    s = torch.where(bits, 1.0, -1.0).to(torch.float64)
    return a, s


def _partial(a, s, d):
    """d w_c / d frac_d [n,8]: sign along d times the other two factors."""
    o = [e for e in range(3) if e != d]
    return s[None, :, d] * a[:, :, o[0]] * a[:, :, o[1]]


def _rows(desc_or_levels):
    lvs = desc_or_levels if isinstance(desc_or_levels, list) else levels_of(desc_or_levels)
    return lvs, lvs[-1].offset + lvs[-1].rows


def grid_backward_ref(desc, x01, table, dfeat, levels=None):
    """First order: d(sum dfeat . grid(x01)) / d table and / d x01.

    Returns dict with (value, M) pairs ``grad_table`` [rows,2], ``dx`` [n,3] and ``k`` [rows] (int64)."""
    lvs, rows = _rows(levels if levels is not None else desc)
    dev = x01.device
    n = x01.shape[0]
    gt, gt_m = torch.zeros(rows, 2, dtype=torch.float64, device=dev), torch.zeros(rows, 2, dtype=torch.float64, device=dev)
    k = torch.zeros(rows, dtype=torch.int64, device=dev)
    dx, dx_m = torch.zeros(n, 3, dtype=torch.float64, device=dev), torch.zeros(n, 3, dtype=torch.float64, device=dev)
    for l, lv in enumerate(lvs):
        idx, frac = level_corners(x01, lv)
        a, s = _axis_factors(frac)
        w = a.prod(2)                                                    # [n,8], >= 0
        g = dfeat[:, 2 * l:2 * l + 2].double()                           # [n,2]
        flat = idx.reshape(-1)
        for f in range(2):
            term = (w * g[:, f:f + 1]).reshape(-1)
            gt[:, f].index_add_(0, flat, term)
            gt_m[:, f].index_add_(0, flat, term.abs())
        k.index_add_(0, flat, ((w * g.abs().sum(1, keepdim=True)) > 0).reshape(-1).long())
        t = table[idx].double()                                          # [n,8,2]
        sdot = (t * g[:, None, :]).sum(2)
        sabs = (t.abs() * g.abs()[:, None, :]).sum(2)
        for d in range(3):
            pd = _partial(a, s, d)
            dx[:, d] += lv.scale * (pd * sdot).sum(1)
            dx_m[:, d] += abs(lv.scale) * (pd.abs() * sabs).sum(1)
    return {"grad_table": (gt, gt_m), "dx": (dx, dx_m), "k": k}


def grid_double_backward_ref(desc, x01, table, dfeat, v, levels=None):
    """Second order: the backward of gx = J(x01; table)^T dfeat along v = dL/dgx [n,3] (the comment above
    grid_double_backward_table_kernel): with D_l(c) = scale_l sum_d v_d dw_c/dfrac_d,
      g_dfeat[l,f] = sum_c D_l(c) table[c][f],   grad_table[c][f] += D_l(c) dfeat[l,f],
      g_x[e] = sum_l scale_l^2 sum_{d != e} v_d sum_c (d2 w_c / dfrac_d dfrac_e) (dfeat_l . table[c]).
    Returns dict with (value, M) pairs ``g_dfeat`` [n,32], ``g_x`` [n,3], ``grad_table`` [rows,2] and ``k`` [rows]."""
    lvs, rows = _rows(levels if levels is not None else desc)
    dev = x01.device
    n = x01.shape[0]
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)       # noqa: E731
    gt, gt_m, gd, gd_m, gx, gx_m = z(rows, 2), z(rows, 2), z(n, 32), z(n, 32), z(n, 3), z(n, 3)
    k = torch.zeros(rows, dtype=torch.int64, device=dev)
    vv = v.double()
    for l, lv in enumerate(lvs):
        idx, frac = level_corners(x01, lv)
        a, s = _axis_factors(frac)
        pd = [_partial(a, s, d) for d in range(3)]
        D = lv.scale * sum(vv[:, d:d + 1] * pd[d] for d in range(3))                        # [n,8]
        Dm = abs(lv.scale) * sum(vv[:, d:d + 1].abs() * pd[d].abs() for d in range(3))
        g = dfeat[:, 2 * l:2 * l + 2].double()
        t = table[idx].double()
        flat = idx.reshape(-1)
        for f in range(2):
            term = (D * g[:, f:f + 1]).reshape(-1)
            gt[:, f].index_add_(0, flat, term)
            gt_m[:, f].index_add_(0, flat, (Dm * g[:, f:f + 1].abs()).reshape(-1))
            gd[:, 2 * l + f] = (D * t[:, :, f]).sum(1)
            gd_m[:, 2 * l + f] = (Dm * t[:, :, f].abs()).sum(1)
        k.index_add_(0, flat, ((Dm * g.abs().sum(1, keepdim=True)) > 0).reshape(-1).long())
        gc = (t * g[:, None, :]).sum(2)                                  # dfeat_l . table[c], [n,8]
        gcm = (t.abs() * g.abs()[:, None, :]).sum(2)
        s2 = lv.scale * lv.scale
        for e in range(3):
            for d in range(3):
                if d == e:
                    continue
                o = 3 - d - e                                            # the third axis
                mixed = s[None, :, d] * s[None, :, e] * a[:, :, o]       # d2 w_c / dfrac_d dfrac_e
                gx[:, e] += s2 * vv[:, d] * (mixed * gc).sum(1)
                gx_m[:, e] += s2 * vv[:, d].abs() * (mixed.abs() * gcm).sum(1)
    return {"g_dfeat": (gd, gd_m), "g_x": (gx, gx_m), "grad_table": (gt, gt_m), "k": k}


def trilinear_forward_fp64(x01, table, idx_frac):
    """float64 forward built on fixed corner indices: frac carries the fp32 value and d frac / d x = scale, so float64
    autograd of it differentiates exactly what the kernels differentiate.  idx_frac: [(Level, idx, frac)] per level."""
    out = []
    for lv, idx, frac in idx_frac:
        f = frac.double() + lv.scale * (x01 - x01.detach())
        bits = [[(c >> d) & 1 for d in range(3)] for c in range(8)]
        feat = 0.0
        for c in range(8):
            w = 1.0
            for d in range(3):
                w = w * (f[:, d] if bits[c][d] else 1.0 - f[:, d])
            feat = feat + w[:, None] * table[idx[:, c]]
        out.append(feat)
    return torch.cat(out, 1)


# ---------------------------------------------------------------------------------------------------------------------
# Route constants of csrc/grid_backward.hip the GPU tests place their edges by (tests/test_grid_backward_reference.py
# parses them from the source, so a retune cannot move the edges away from the tests unnoticed).
LDS_ROWS = 20000            # kLdsRows: rows per LDS partition
MAX_LDS_PARTS = 64          # kMaxLdsParts: more partitions than this -> the quad atomics for that level
SCATTER_THREADS = 1024      # kScatterThreads
SCATTER_UNROLL = 8          # kScatterUnroll: points per lane and trip of the walk
LDS_MIN_N = 1 << 15         # smallest batch that takes the LDS walk


def field_per_level_scale(scale=1.5, min_res=16, max_res=512, n_levels=16):
    """Field's growth factor (field.py: exp(log(max_res * scale / min_res) / (L - 1)))."""
    import numpy as np
    return float(np.exp(np.log(max_res * scale / min_res) / (n_levels - 1)))


# qf_grid_desc_init arguments (log2_T, base_resolution, per_level_scale) of the configs under test.  "edges": every
# level dense, resolutions 100 .. 117: res 100 is exactly 50 partitions, res 108 is 63 (LDS walk), res 109 is 65
# (quad atomics) -- qf_grid_desc_init cannot produce exactly 64.
def init_args(name):
    from oracle import fields as ofields
    return {"ngp19": (19, 16, ofields.ngp_per_level_scale(4096, 16, 16)),
            "ngp21": (21, 16, ofields.ngp_per_level_scale(4096, 16, 16)),
            "field19": (19, 16, field_per_level_scale()),
            "field24": (24, 16, field_per_level_scale()),
            "edges": (21, 100, 1.01)}[name]


# The hand-edited desc: dense levels the level rule cannot produce.  (res, rows, hashed): exactly 64 x LDS_ROWS rows
# (the last size the walk takes), 64 x LDS_ROWS + 8 (65 partitions, the last of 8 rows: quad atomics) and 50 x LDS_ROWS
# + 8 (51 partitions, the last of 8 rows: walk); res 109 over 64 x LDS_ROWS rows has res^3 > rows, so its upper corner
# rows wrap.  fill_grid_args only asks res^2 <= rows of a dense level and power-of-two rows of a hashed one.
HAND_LEVELS = [(16, 4096, False), (24, 13824, False), (32, 32768, False), (52, 140608, False), (64, 262144, False),
               (100, 50 * LDS_ROWS + 8, False), (109, 64 * LDS_ROWS, False), (109, 64 * LDS_ROWS + 8, False),
               (108, 64 * LDS_ROWS, False), (98, 941192, False), (160, 1 << 19, True), (200, 1 << 19, True),
               (256, 1 << 18, True), (320, 1 << 19, True), (400, 1 << 20, True), (512, 1 << 19, True)]


def hand_desc(GridDesc):
    """A GridDesc (the ctypes class) built from HAND_LEVELS, scale = res - 1."""
    d = GridDesc()
    d.n_levels, d.n_features, d.log2_hashmap_size, d.base_resolution, d.per_level_scale = N_LEVELS, 2, 20, 16, 1.0
    off, mask = 0, 0
    for l, (res, rows, hashed) in enumerate(HAND_LEVELS):
        mask |= int(hashed) << l
        d.offset[l] = off
        d.resolution[l] = res
        d.scale[l] = float(res - 1)
        off += rows
    d.offset[N_LEVELS] = off
    d.hashed_mask = mask
    return d


def parts(rows):
    return -(-rows // LDS_ROWS)


def scatter_plan(lvs, cu_count):
    """table_scatter_ws's plan: per level (walk?, partitions, point chunks per partition)."""
    per_level = max(16, 3 * cu_count // 8)
    out = []
    for lv in lvs:
        p = parts(lv.rows)
        if p > MAX_LDS_PARTS:
            out.append((False, p, 1))
        else:
            out.append((True, p, max(1, (per_level + p // 2) // p)))
    return out
