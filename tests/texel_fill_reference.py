"""numpy restatement of the texel-position map, the yardstick of qf_texel_positions.

Written from the five rules, vectorised over candidate texels instead of looping over faces:
  1. s = clip(uv * (H, W), 0, (H-1, W-1)) in fp64, q = trunc(s); uv[:,0] is the row.
  2. face f covers the texels (r, c) of q[f]'s bounding box for which (x=c, y=r) passes ``inside``;
  3. owner(p) = the largest covering f; tri_size[f] = the size of f's cover;
  4. edges 0->1, 1->2, 2->0 sampled at linspace(0, 1, 100) on s; line_owner(p) = the largest touching f;
  5. owned: fp64 Cramer barycentrics of (r, c, 0) in q[owner] (centroid for a degenerate face); otherwise the centroid
     of line_owner(p), of face F-1 (untouched="last_face") or 0 (untouched="zero"); rounded once to fp32.
"""
import numpy as np

W_SAMPLES = np.linspace(0.0, 1.0, 100)


def scaled_corners(uv, H, W):
    s = np.empty_like(np.asarray(uv, dtype=np.float64))
    s[:, 0] = np.clip(uv[:, 0] * H, 0, H - 1)
    s[:, 1] = np.clip(uv[:, 1] * W, 0, W - 1)
    return s, s.astype(np.int64)


def inside(x, y, xs, ys):
    """Even-odd test of points (x, y) against triangles with corners (xs, ys) [n, 3]; corners and edges are inside."""
    hit = np.zeros(x.shape, dtype=bool)
    par = np.zeros(x.shape, dtype=bool)
    for i in range(3):
        j = (i + 2) % 3
        xi, yi, xj, yj = xs[:, i], ys[:, i], xs[:, j], ys[:, j]
        hit |= (x == xi) & (y == yi)
        hit |= (yi == yj) & (yi == y) & (((xi < x) & (x < xj)) | ((xj < x) & (x < xi)))
        cross = (yi > y) != (yj > y)
        den = np.where(cross, yj - yi, 1)
        lx = (xj - xi) * (y - yi) / den + xi                   # fp64, exact enough for integer corners (see DESIGN)
        hit |= cross & (x == lx)
        par ^= cross & (x < lx)
    return hit | par


def _candidates(q, face_ids, window):
    """Candidate texels (face, r, c) of the faces ``face_ids`` (ascending), restricted to ``window`` = (r0, c0, h, w)."""
    qf = q[face_ids]                                                     # [n, 3, 2]
    r0, r1 = qf[:, :, 0].min(1), qf[:, :, 0].max(1)
    c0, c1 = qf[:, :, 1].min(1), qf[:, :, 1].max(1)
    if window is not None:
        wr, wc, wh, ww = window
        r0, r1 = np.maximum(r0, wr), np.minimum(r1, wr + wh - 1)
        c0, c1 = np.maximum(c0, wc), np.minimum(c1, wc + ww - 1)
    bh, bw = np.maximum(r1 - r0 + 1, 0), np.maximum(c1 - c0 + 1, 0)
    area = bh * bw
    idx = np.repeat(np.arange(len(face_ids)), area)
    k = np.arange(idx.shape[0]) - np.repeat(np.cumsum(area) - area, area)
    r = r0[idx] + k // bw[idx]
    c = c0[idx] + k % bw[idx]
    keep = inside(c, r, qf[idx, :, 1], qf[idx, :, 0])
    return idx, r, c, keep


def cover_counts(faces, uv, H, W, chunk=1 << 16):
    """tri_size of every face (rule 3), chunked over faces."""
    _, q = scaled_corners(uv, H, W)
    q = q[faces]
    out = np.zeros(len(faces), dtype=np.int64)
    for b in range(0, len(faces), chunk):
        ids = np.arange(b, min(b + chunk, len(faces)))
        idx, _, _, keep = _candidates(q, ids, None)
        out[ids] = np.bincount(idx[keep], minlength=len(ids))
    return out


def _last_by_texel(p, f, n):
    """out[p] = the largest f written to p (-1 where none)."""
    out = np.full(n, -1, dtype=np.int64)
    if p.size:
        order = np.lexsort((f, p))
        p, f = p[order], f[order]
        last = np.r_[p[1:] != p[:-1], True]
        out[p[last]] = f[last]
    return out


def texel_positions(vertices, faces, uv, H, W, untouched="last_face", window=None, face_ids=None):
    """(V [h, w, 3] fp32, tri_size [F] int64) of the map, or of ``window`` = (r0, c0, h, w) of it.  ``face_ids``
    restricts the drawn faces (ascending global ids; face F-1 still fills untouched texels)."""
    vertices = np.asarray(vertices, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64)
    F = len(faces)
    s, q = scaled_corners(np.asarray(uv, dtype=np.float64), H, W)
    sf, qf = s[faces], q[faces]                                          # [F, 3, 2]
    ids = np.arange(F) if face_ids is None else np.asarray(face_ids, dtype=np.int64)
    wr, wc, wh, ww = (0, 0, H, W) if window is None else window

    idx, r, c, keep = _candidates(qf, ids, window)
    tri_size = np.zeros(F, dtype=np.int64)
    if window is None:
        tri_size[ids] = np.bincount(idx[keep], minlength=len(ids))
    owner = _last_by_texel((r[keep] - wr) * ww + (c[keep] - wc), ids[idx[keep]], wh * ww)

    ls_p, ls_f = [], []
    for a, b in ((0, 1), (1, 2), (2, 0)):
        pts = (sf[ids, b][:, None, :] * W_SAMPLES[None, :, None]
               + sf[ids, a][:, None, :] * (1 - W_SAMPLES[None, :, None])).astype(np.int64)      # [n, 100, 2]
        rr, cc = pts[..., 0].ravel(), pts[..., 1].ravel()
        ff = np.repeat(ids, 100)
        m = (rr >= wr) & (rr < wr + wh) & (cc >= wc) & (cc < wc + ww)
        ls_p.append((rr[m] - wr) * ww + (cc[m] - wc))
        ls_f.append(ff[m])
    line_owner = _last_by_texel(np.concatenate(ls_p), np.concatenate(ls_f), wh * ww)

    tri = vertices[faces]                                                # [F, 3, 3]
    centroid = tri.mean(1)
    V = np.zeros((wh * ww, 3), dtype=np.float64)
    fill = np.where(owner >= 0, owner, line_owner)
    if untouched == "last_face":
        fill = np.where(fill >= 0, fill, F - 1)
    has = fill >= 0
    V[has] = centroid[fill[has]]

    own = np.nonzero(owner >= 0)[0]
    o = owner[own]
    qq = np.concatenate([qf[o].astype(np.float64), np.zeros((len(o), 3, 1))], axis=2)
    p = np.stack([(own // ww + wr).astype(np.float64), (own % ww + wc).astype(np.float64), np.zeros(len(o))], 1)
    e0, e1, w = qq[:, 1] - qq[:, 0], qq[:, 2] - qq[:, 0], p - qq[:, 0]

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    d00, d01, d02, d11, d12 = dot(e0, e0), dot(e0, e1), dot(e0, w), dot(e1, e1), dot(e1, w)
    den = d00 * d11 - d01 * d01
    ok = den != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / den
        b2 = (d00 * d12 - d01 * d02) * inv
        b1 = (d11 * d02 - d01 * d12) * inv
    b0 = (1 - b1) - b2
    t = tri[o]
    blend = (b0[:, None] * t[:, 0] + b1[:, None] * t[:, 1]) + b2[:, None] * t[:, 2]
    V[own[ok]] = blend[ok]
    return V.astype(np.float32).reshape(wh, ww, 3), tri_size


def faces_reaching(uv, faces, H, W, window):
    """Ids of the faces whose bounding box (which holds their cover and their edge samples) meets ``window``."""
    _, q = scaled_corners(np.asarray(uv, dtype=np.float64), H, W)
    qf = q[np.asarray(faces)]
    wr, wc, wh, ww = window
    m = ((qf[:, :, 0].max(1) >= wr) & (qf[:, :, 0].min(1) < wr + wh) & (qf[:, :, 1].max(1) >= wc)
         & (qf[:, :, 1].min(1) < wc + ww))
    return np.nonzero(m)[0]
