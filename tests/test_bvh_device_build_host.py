"""CPU: the numpy restatement of the device BVH build (tests/bvh_device_build_reference.py) builds a valid 8-wide tree,
and its key and split rules give the hand-worked values."""
import functools

import numpy as np

from tests import bvh_device_build_reference as ref

EMPTY = int(ref.EMPTY)


@functools.lru_cache(maxsize=None)
def _built():
    from quadraturefields_amd import synthetic
    mesh = synthetic.shell_mesh(n_shells=3, subdivisions=3)
    tri = np.ascontiguousarray(mesh.vertices.astype(np.float32)[mesh.faces])
    return tri, ref.build(tri)


def _walk(nodes):
    """(node, slot, token, lo, hi) of every live child."""
    n = nodes.reshape(-1, 8, 8)
    tok = n[:, :, 6].view(np.int32)
    for i in range(n.shape[0]):
        for j in range(8):
            if int(tok[i, j]) != EMPTY:
                yield i, j, int(tok[i, j]), n[i, j, 0:3], n[i, j, 3:6]


def test_every_triangle_sits_in_exactly_one_leaf_of_1_to_8():
    tri, b = _built()
    seen = np.zeros(tri.shape[0], dtype=np.int64)
    for _, _, tok, _, _ in _walk(b["nodes"]):
        if tok < 0:
            first, cnt = (~tok) >> 3, ((~tok) & 7) + 1
            assert 1 <= cnt <= 8 and first + cnt <= tri.shape[0]
            seen[first:first + cnt] += 1
    assert np.array_equal(seen, np.ones_like(seen))
    assert np.array_equal(np.sort(b["tri_ids"]), np.arange(tri.shape[0]))
    assert bool((b["codes"][1:] >= b["codes"][:-1]).all())


def test_boxes_enclose_their_subtrees_and_children_follow_their_parents():
    tri, b = _built()
    tris = tri[b["tri_ids"]]
    nodes = b["nodes"].reshape(-1, 8, 8)
    tok_all = nodes[:, :, 6].view(np.int32)
    N = nodes.shape[0]
    referenced = np.zeros(N, dtype=np.int64)
    level_of = np.searchsorted(np.asarray(b["level_start"]), np.arange(N), side="right") - 1
    assert b["level_start"][0] == 0 and b["level_start"][-1] == N
    for i, j, tok, lo, hi in _walk(b["nodes"]):
        assert bool((lo <= hi).all())
        if tok < 0:
            first, cnt = (~tok) >> 3, ((~tok) & 7) + 1
            p = tris[first:first + cnt].reshape(-1, 3)
            assert bool((p >= lo).all() and (p <= hi).all())
        else:
            assert i < tok < N and level_of[tok] == level_of[i] + 1
            referenced[tok] += 1
            live = tok_all[tok] != EMPTY
            assert bool((nodes[tok, live, 0:3] >= lo).all() and (nodes[tok, live, 3:6] <= hi).all())
        # live children fill the first slots
        assert bool((tok_all[i, :j] != EMPTY).all())
    assert referenced[0] == 0 and np.array_equal(referenced[1:], np.ones(N - 1, dtype=np.int64))
    # inner tokens ascend in (node, slot) order: the level order of the scan
    inner = [tok for _, _, tok, _, _ in _walk(b["nodes"]) if tok >= 0]
    assert inner == list(range(1, N))
    # the derived capacity bound
    assert N <= max(1, (tri.shape[0] - 1) // 7)


def test_stack_bound_covers_the_worst_path():
    """A depth-first walk that pushes every child and pops one: the deepest the stack gets, over all paths."""
    _, b = _built()
    tok_all = b["nodes"].reshape(-1, 8, 8)[:, :, 6].view(np.int32)

    def worst(node, depth_before):
        live = [int(t) for t in tok_all[node] if int(t) != EMPTY]
        peak = depth_before + len(live)
        for t in live:
            if t >= 0:                                # popped: the others stay on the stack
                peak = max(peak, worst(t, depth_before + len(live) - 1))
        return peak

    assert worst(0, 0) + 1 <= b["max_stack"] <= 384


def test_hand_worked_keys():
    cent = np.array([[1.0, -2.0, 5.0], [3.0, 6.0, 5.0], [2.0, 2.0, 5.0], [1.0, 6.0, 5.0]], dtype=np.float32)
    code = ref.morton_codes(cent)
    # z has zero extent: its bits (3b) are 0 everywhere; x sits at 3b + 2, y at 3b + 1
    x_all = sum(1 << (3 * b + 2) for b in range(21))
    y_all = sum(1 << (3 * b + 1) for b in range(21))
    assert int(code[0]) == 0
    assert int(code[1]) == x_all | y_all
    assert int(code[2]) == (1 << 62) | (1 << 61)              # the midpoint: 2^20 on both axes, the top bit of each
    assert int(code[3]) == y_all
    # three live axes: minimum -> 0, maximum -> all 63 bits
    cent = np.array([[-1.0, -1.0, -1.0], [0.25, 7.0, 3.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    code = ref.morton_codes(cent)
    assert int(code[0]) == 0 and int(code[1]) == (1 << 63) - 1
    # a quarter of the x range: 2^19 -> bit 19 of x -> code bit 3 * 19 + 2
    cent = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=np.float32)
    assert int(ref.morton_codes(cent)[2]) == 1 << (3 * 19 + 2)


def test_split_halving_and_prefix_branches():
    # equal end codes: the index range is halved
    same = np.full(10, 5, dtype=np.uint64)
    assert ref.split_range(same, 0, 9) == 4 and ref.split_range(same, 2, 5) == 3 and ref.split_range(same, 3, 4) == 3
    # 0b000, 0b001, 0b010, 0b011 | 0b100, 0b101, 0b111: the first differing bit of the ends is bit 2
    code = np.array([0, 1, 2, 3, 4, 5, 7], dtype=np.uint64)
    assert ref.split_range(code, 0, 6) == 3
    assert ref.split_range(code, 0, 3) == 1                   # bit 1
    assert ref.split_range(code, 4, 6) == 5                   # 100, 101 | 111
    assert ref.split_range(code, 5, 6) == 5
    # lopsided: one code below the split bit, many above
    code = np.array([1] + [8] * 20, dtype=np.uint64)
    assert ref.split_range(code, 0, 20) == 0
    assert ref.split_range(code, 1, 20) == 10
    # a high bit (beyond 32) decides
    code = np.array([1, 2, 1 << 62, (1 << 62) + 1], dtype=np.uint64)
    assert ref.split_range(code, 0, 3) == 1


def test_node_children_replaces_the_largest_leftmost_first():
    # 40 equal codes: halving all the way; 40 -> 20|20 -> 10|10|20 -> 10|10|10|10 -> 5|5|10|10|10 -> ... -> 8 children of 5
    same = np.zeros(40, dtype=np.uint64)
    assert ref.node_children(same, 0, 39) == [0, 5, 10, 15, 20, 25, 30, 35, 40]
    # 20 equal codes: 10|10 -> 5|5|10 -> 5|5|5|5: stops with four children, none above 8
    assert ref.node_children(np.zeros(20, dtype=np.uint64), 0, 19) == [0, 5, 10, 15, 20]
    # at most 8 triangles: one leaf child
    assert ref.node_children(np.zeros(8, dtype=np.uint64), 0, 7) == [0, 8]
    # 100 equal codes: 8 children, the larger ones stay inner
    s = ref.node_children(np.zeros(100, dtype=np.uint64), 0, 99)
    assert len(s) == 9 and s[0] == 0 and s[-1] == 100 and max(np.diff(s)) == 13


def test_tiny_and_empty_meshes():
    tri = np.arange(27, dtype=np.float32).reshape(3, 3, 3)
    b = ref.build(tri)
    tok = b["nodes"].reshape(-1, 8, 8)[:, :, 6].view(np.int32)
    assert b["level_start"] == [0, 1] and b["max_stack"] == 2
    assert int(tok[0, 0]) == ~((0 << 3) | 2) and bool((tok[0, 1:] == EMPTY).all())
    assert ref.build(np.zeros((0, 3, 3), np.float32))["nodes"].shape == (0, 64)
