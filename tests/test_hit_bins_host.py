"""CPU: the hit-bin entry points refuse NULL / mismatched arguments before any launch (no device is needed to be refused)."""
import ctypes

from quadraturefields_amd import _C

QF_ERR_INVALID_ARGUMENT = -1


def _camera(w=16, h=8):
    cam = _C.Camera()
    cam.c2w[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4]
    cam.fx = cam.fy = 20.0
    cam.cx, cam.cy, cam.width, cam.height = w / 2, h / 2, w, h
    return cam


def test_hit_bins_bytes(lib):
    assert lib.qf_hit_bins_bytes(800, 800, 25) == 100 * 100 * 64 * 25 * 8
    assert lib.qf_hit_bins_bytes(1920, 1080, 25) == 240 * 135 * 64 * 25 * 8      # 1080 rows: 135 tile rows
    assert lib.qf_hit_bins_bytes(9, 1, 1) == 2 * 64 * 8
    for bad in ((0, 8, 25), (8, 0, 25), (8, 8, 0), (8, 8, _C.QF_BVH_MAX_HITS + 1)):
        assert lib.qf_hit_bins_bytes(*bad) == -1


def test_raster_intersect_tiles_refuses_bad_arguments(lib):
    assert lib.qf_status_string(QF_ERR_INVALID_ARGUMENT) == lib.qf_status_string(
        lib.qf_raster_intersect_tiles(None, None, None, None, 0, 0, None, None, None, 0, None, None, None, None))
    cam = _camera()
    p = ctypes.c_void_p(4096)                 # never dereferenced: the handle is NULL
    rc = lib.qf_raster_intersect_tiles(None, ctypes.byref(cam), p, p, 128, 25, p, p, p, 1 << 30, p, p, p, None)
    assert rc == QF_ERR_INVALID_ARGUMENT


def test_pack_tiles_bins_refuses_bad_arguments(lib):
    p = ctypes.c_void_p(4096)
    args = lambda **kw: [kw.get("o", p), p, kw.get("w", 16), 8, kw.get("k", 25), kw.get("tri", p), p, p, p, p, p, p, p, None,
                         0.0, p, p, None, 1, kw.get("cursor", p), kw.get("mask", p), kw.get("bins", p), None, None]
    for bad in (dict(cursor=None), dict(mask=None), dict(bins=None), dict(k=33), dict(k=0), dict(w=0), dict(tri=None),
                dict(o=None)):
        assert lib.qf_pack_tiles_bins(*args(**bad)) == QF_ERR_INVALID_ARGUMENT, bad
