"""CPU: the host side of ``baking.bake_texture_set`` -- the band size and the argument checks, which raise before any
device work (the tensors here are host tensors and the fields and the texture set are stubs)."""
import pytest
import torch


class _Set:
    def __init__(self, texture_size, num_lobes):
        self.texture_size, self.num_lobes = texture_size, num_lobes
        self.device = torch.device("cpu")

    def texture_set(self):
        raise AssertionError("the texture set was touched before the arguments were checked")


class _SG:
    def __init__(self, lobes):
        self.num_g_lobes = lobes

    def features(self, *a, **k):
        raise AssertionError("the field was evaluated before the arguments were checked")


def test_bake_chunk_rows():
    from quadraturefields_amd.baking import bake_chunk_rows
    for t, lobes in ((64, 3), (4096, 6), (8192, 3), (16384, 8), (70, 1)):
        row_bytes = t * (4 + 12 + 4 * (3 + 7 * lobes + 1) + 4)
        rows = bake_chunk_rows(t, lobes)
        assert 1 <= rows <= t
        assert rows == t or (rows * row_bytes <= 256 << 20 < (rows + 1) * row_bytes)      # the default budget, used in full
        last = 0
        for budget in sorted((row_bytes, 2 * row_bytes + 1, 1 << 20, 1 << 24, 256 << 20, 1 << 32, 1 << 40)):
            if budget < row_bytes:
                continue
            got = bake_chunk_rows(t, lobes, workspace_bytes=budget)
            assert 1 <= got <= t and got >= last and got * row_bytes <= max(budget, row_bytes)
            last = got
        assert last == t                                                                    # 1 TiB holds any map
        assert bake_chunk_rows(t, lobes, workspace_bytes=row_bytes) == 1
        with pytest.raises(ValueError):
            bake_chunk_rows(t, lobes, workspace_bytes=row_bytes - 1)
    with pytest.raises(ValueError):
        bake_chunk_rows(0, 3)
    with pytest.raises(ValueError):
        bake_chunk_rows(64, 0)


def test_bake_texture_set_checks_in_order():
    from quadraturefields_amd.baking import bake_texture_set
    sg, good = _SG(3), torch.zeros(8, 8, 3)
    # 1. V is [T, T, 3] -- raised even when everything else is wrong too
    for bad in (torch.zeros(8, 8), torch.zeros(8, 6, 3), torch.zeros(8, 8, 4), torch.zeros(2, 8, 8, 3), [[0.0]]):
        with pytest.raises(ValueError, match=r"\[T, T, 3\]"):
            bake_texture_set(sg, None, bad, _Set(9, 2), rows_per_chunk=0)
    # 2. T == compressor.texture_size
    with pytest.raises(ValueError, match="texture set is 9 x 9"):
        bake_texture_set(sg, None, good, _Set(9, 2), rows_per_chunk=0)
    # 3. lobe counts
    with pytest.raises(ValueError, match="3 lobes, the texture set 2"):
        bake_texture_set(sg, None, good, _Set(8, 2), rows_per_chunk=0)
    # 4. rows_per_chunk >= 1
    for bad in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="rows_per_chunk"):
            bake_texture_set(sg, None, good, _Set(8, 3), rows_per_chunk=bad)
    # ... and only then the device: a host V is refused without any field or texture-set access
    with pytest.raises(ValueError, match="on the device"):
        bake_texture_set(sg, None, good, _Set(8, 3), rows_per_chunk=4)
    with pytest.raises(ValueError, match="on the device"):
        bake_texture_set(sg, None, good, _Set(8, 3))


def test_bake_texture_set_has_no_host_wait_in_its_body():
    """The launch sequence depends on T and rows_per_chunk alone: no count comes back to the host, no boolean-mask
    indexing or nonzero sizes an array."""
    import inspect
    from quadraturefields_amd import baking
    body = inspect.getsource(baking.bake_texture_set)
    for word in (".item()", ".cpu()", "nonzero", ".tolist()", "[mask]", "synchronize"):
        assert word not in body, word
