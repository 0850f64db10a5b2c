"""A literal numpy restatement of the device BVH build (``csrc/bvh_build_device.hip``): keys,
sort, split, node construction, level order, boxes and the stack bound.  Every fp32 operation is one numpy fp32
operation, so the device build can be compared with it byte for byte."""
import numpy as np

LEAF_MAX = 8
EMPTY = np.int32(-2 ** 31)
AXIS_BITS = 21
AXIS_MAX = (1 << AXIS_BITS) - 1
MAX_LEVELS = 96
F32 = np.float32


def scene_eps(tri):
    """``qf_bvh_eps_from_bounds`` over the vertices of ``tri`` [n,3,3] fp32."""
    v = tri.reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = F32(max(F32(0), (hi - lo).max()))
    mag = F32(max(np.abs(lo).max(), np.abs(hi).max()))
    if not np.isfinite(ext):
        ext = F32(0)
    return F32(F32(F32(2e-5) * max(ext, mag)) + F32(1e-30))


def centroids(tri):
    lo, hi = tri.min(axis=1), tri.max(axis=1)
    return (F32(0.5) * (lo + hi)).astype(F32)


def morton_codes(cent, clo=None, chi=None):
    """63-bit codes of fp32 centroids [n,3] over the bounds ``clo`` / ``chi`` (default: their own)."""
    cent = np.asarray(cent, dtype=F32)
    clo = cent.min(axis=0) if clo is None else np.asarray(clo, dtype=F32)
    chi = cent.max(axis=0) if chi is None else np.asarray(chi, dtype=F32)
    code = np.zeros(cent.shape[0], dtype=np.uint64)
    for k in range(3):
        with np.errstate(over="ignore", invalid="ignore"):
            ext = F32(chi[k] - clo[k])
            scale = F32(F32(2 ** AXIS_BITS) / ext) if (ext > 0 and np.isfinite(ext)) else F32(0)
            t = ((cent[:, k] - clo[k]).astype(F32) * scale).astype(F32)
        q = np.zeros(cent.shape[0], dtype=np.uint64)
        ok = t >= 0                                           # NaN -> 0
        q[ok] = np.where(t[ok] >= F32(AXIS_MAX), AXIS_MAX, np.minimum(t[ok], F32(AXIS_MAX)).astype(np.int64)).astype(np.uint64)
        for b in range(AXIS_BITS):
            code |= ((q >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + (2 - k))
    return code


def split_range(code, l, r):
    """Last position of the left half of [l, r], l < r."""
    a, b = int(code[l]), int(code[r])
    if a == b:
        return l + (r - l) // 2
    shift = (a ^ b).bit_length() - 1
    lo, hi = l, r
    for _ in range(32):
        if hi - lo <= 1:
            break
        mid = lo + (hi - lo) // 2
        if (int(code[mid]) ^ a) >> shift == 0:
            lo = mid
        else:
            hi = mid
    return lo


def node_children(code, l, r):
    """Boundaries s[0] < .. < s[h] of the children of the node over [l, r]."""
    if r - l + 1 <= LEAF_MAX:
        return [l, r + 1]
    s = [l, split_range(code, l, r) + 1, r + 1]
    while len(s) - 1 < 8:
        sizes = [s[i + 1] - s[i] for i in range(len(s) - 1)]
        best = int(np.argmax(sizes))                          # first of the largest
        if sizes[best] <= LEAF_MAX:
            break
        s.insert(best + 1, split_range(code, s[best], s[best + 1] - 1) + 1)
    return s


def leaf_token(first, count):
    return np.int32(~((first << 3) | (count - 1)))


def build(tri):
    """``tri`` [n,3,3] fp32 -> dict(nodes [N,64] fp32 with the tokens' bits in float 6 of each child, tri_ids [n] int32,
    level_start, max_stack, codes (sorted), eps)."""
    tri = np.ascontiguousarray(tri, dtype=F32).reshape(-1, 3, 3)
    n = tri.shape[0]
    if n == 0:
        return dict(nodes=np.zeros((0, 64), F32), tri_ids=np.zeros(0, np.int32), level_start=[], max_stack=1,
                    codes=np.zeros(0, np.uint64), eps=F32(0))
    eps = scene_eps(tri)
    code = morton_codes(centroids(tri))
    order = np.argsort(code, kind="stable")
    code = code[order]
    tris = tri[order]
    tokens, level_start = [], [0]
    ranges = [(0, n - 1)]
    for level in range(MAX_LEVELS + 1):
        assert level < MAX_LEVELS
        base = level_start[-1]
        next_base = base + len(ranges)
        nxt = []
        for (l, r) in ranges:
            s = node_children(code, l, r)
            tok = np.full(8, EMPTY, dtype=np.int32)
            for j in range(len(s) - 1):
                a, size = s[j], s[j + 1] - s[j]
                if size <= LEAF_MAX:
                    tok[j] = leaf_token(a, size)
                else:
                    tok[j] = next_base + len(nxt)
                    nxt.append((a, a + size - 1))
            tokens.append(tok)
        level_start.append(next_base)
        if not nxt:
            break
        ranges = nxt
    tokens = np.stack(tokens)
    N = tokens.shape[0]
    nodes = np.zeros((N, 8, 8), dtype=F32)
    nodes[:, :, 0:3] = np.inf
    nodes[:, :, 3:6] = -np.inf
    nodes[:, :, 6] = tokens.view(F32)
    need = np.zeros(N, dtype=np.int64)
    for node in range(N - 1, -1, -1):                         # children have larger indices
        h, deepest = 0, 0
        for j in range(8):
            t = int(tokens[node, j])
            if t == int(EMPTY):
                continue
            h += 1
            if t < 0:
                first, cnt = (~t) >> 3, ((~t) & 7) + 1
                p = tris[first:first + cnt].reshape(-1, 3)
                nodes[node, j, 0:3] = p.min(axis=0) - eps
                nodes[node, j, 3:6] = p.max(axis=0) + eps
            else:
                live = tokens[t] != EMPTY
                nodes[node, j, 0:3] = nodes[t, live, 0:3].min(axis=0)
                nodes[node, j, 3:6] = nodes[t, live, 3:6].max(axis=0)
                deepest = max(deepest, int(need[t]))
        need[node] = max(h, h - 1 + deepest)
    return dict(nodes=nodes.reshape(N, 64), tri_ids=order.astype(np.int32), level_start=level_start,
                max_stack=max(1, int(need[0])) + 1, codes=code, eps=eps)
