"""GPU: the state the package keeps behind the caller's back, used from more than one stream.

The caller can order their own tensors across streams; they cannot know that a field keeps 16-bit parameter copies, a
texture set its texel records, a mesh its triangle records.  Those are built by kernels on whatever stream is current at
first use and read by whatever stream is current later: here the first use happens on a side stream BEHIND A DELAY
(``stream_harness.delay``) and the second on another stream at once, with no synchronisation by the caller -- the caller's
own tensors were ready long before.  The result must be the fully synchronised run's, bit for bit (the same kernels on
the same data).  Then the intersector's per-stream scratch with two frames in flight, and bench.py's front / back
pipeline against its own sequential frames.
"""
import numpy as np
import pytest
import torch

from tests import stream_harness as sh

pytestmark = pytest.mark.gpu

DELAY_MS = 60.0          # every cached build below is issued in well under 6 ms of host time (stream_harness.ISSUE_FACTOR)
N_POINTS = 4101
SIZE = 64


# ------------------------------------------------------------------------------------------------ the cache owners
def _ngp(device, dtype, lobes=0):
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField, NGPRadianceFieldSGNew
    from tests.test_gpu_fp16 import _make
    f = _make(NGPRadianceFieldSGNew, device, use_viewdirs=False, num_g_lobes=lobes) if lobes else _make(NGPRadianceField, device)
    f.compute_dtype = dtype
    return f


def _points(device, seed=3):
    from tests import helpers
    x, d = helpers.random_points(N_POINTS, seed=seed)
    return x.to(device), d.to(device)


class _Owner:
    """make() -> a new cache owner with the same contents every time; use(obj) -> tuple of tensors; cached(obj) -> has
    the hidden state been built?  ``host_wait``: the first use reads something back (the cache is host data), so the host
    sits out the delay and the building stream cannot be caught busy."""
    host_wait = False


class _NGPOwner(_Owner):
    def __init__(self, device, dtype, lobes=0):
        self.device, self.dtype, self.lobes = device, dtype, lobes
        self.host_wait = dtype == "fp32"
        self.x, self.d = _points(device)

    def make(self):
        f = _ngp(self.device, self.dtype, self.lobes)
        if self.dtype != "fp32":
            # the host copy of the aabb is read with a blocking copy at the first evaluation: taken now, or the host
            # would sit out the delay before it enqueues the 16-bit copies, and nothing would be in flight any more
            f._field_desc(0)
            torch.cuda.synchronize()
        return f

    def use(self, f):
        rgb, sigma = f(self.x, self.d)
        return rgb, sigma

    def cached(self, f):
        if self.dtype == "fp32":
            return f._desc_cache is not None             # the host copy of the aabb
        return getattr(f, "_half_cache", None) is not None

    def params(self, f):
        return [p for p in f.parameters()]


class _DeformOwner(_Owner):
    def __init__(self, device):
        self.device = device
        self.x = (_points(device, seed=5)[0] * 0.9).contiguous()

    def make(self):
        from tests.test_gpu_deform_fp16 import _field
        f = _field(self.device, log2_T=14)[0]
        f.compute_dtype = "fp16"
        return f

    def use(self, f):
        return (f(self.x, return_grad=False)[0],)

    def cached(self, f):
        return getattr(f, "_half_cache", None) is not None

    def params(self, f):
        return [p for p in f.parameters()]


class _TextureOwner(_Owner):
    def __init__(self, device):
        from quadraturefields_amd import synthetic
        self.device = device
        self.tex = synthetic.random_textures(SIZE, 2, seed=1)
        g = torch.Generator().manual_seed(9)
        self.texel = torch.randint(0, SIZE, (N_POINTS, 2), generator=g).to(device)
        self.dirs = _points(device, seed=7)[1]

    def make(self):
        from quadraturefields_amd.texture_utils import FeatureCompression
        t = self.tex
        return FeatureCompression.from_arrays(t["alpha"], t["diffuse"], t["colors"], t["lambdas"], compression_type="sigma",
                                              lambda_thres=7.5, device=self.device)

    def use(self, comp):
        return comp.shade(self.texel, self.dirs)

    def cached(self, comp):
        return getattr(comp, "_records", None) is not None


class _TriangleRecordOwner(_Owner):
    """``utils._triangle_records``.  Only ``texel_indices`` is run on it: the kernel's addresses come from ``index_tri``
    (ours, valid), never from the records' contents, so a read of records that are not built yet stays in bounds."""

    def __init__(self, device):
        from quadraturefields_amd import synthetic
        self.device = device
        self.mesh = synthetic.shell_mesh(n_shells=3, subdivisions=2)
        # fp32 and contiguous: the cache is keyed by the tensor the lookup receives, a converted copy would be a new key
        self.uv = torch.from_numpy(synthetic.scaled_uv(self.mesh, SIZE)).to(torch.float32).contiguous().to(device)
        self.uv_other = (self.uv * 0.5).contiguous()
        g = torch.Generator().manual_seed(11)
        n_faces = int(self.mesh.faces.shape[0])
        self.tri = torch.randint(0, n_faces, (N_POINTS,), generator=g)
        v = torch.from_numpy(np.asarray(self.mesh.vertices, dtype=np.float32))
        f = torch.from_numpy(np.asarray(self.mesh.faces, dtype=np.int64))
        w = torch.rand((N_POINTS, 3), generator=g) + 0.05
        w = w / w.sum(dim=1, keepdim=True)
        self.points = (v[f[self.tri]] * w[:, :, None]).sum(dim=1).contiguous().to(device)
        self.tri = self.tri.to(device)

    def make(self):
        from quadraturefields_amd import utils
        from quadraturefields_amd.mesh_utils import MeshIntersection
        mi = MeshIntersection(self.mesh, simplify_mesh=False, scale=1.0, num_intersections=5)
        # the mesh's vertices and faces go up with blocking copies at the first lookup: done now, with ANOTHER uv set, so
        # that the first lookup with ``uv`` only packs the records -- behind the delay, without the host waiting it out
        utils._triangle_records(mi, self.uv_other)
        torch.cuda.synchronize()
        return mi

    def use(self, mi):
        from quadraturefields_amd import utils
        return (utils.texel_indices(mi, self.uv, self.points, self.tri, SIZE),)

    def cached(self, mi):
        cache = getattr(mi, "_texel_cache", None)
        return cache is not None and cache[3] is not None and cache[3][0] == self.uv.data_ptr()


class _EstimatorOwner(_Owner):
    """``OccGridEstimator._host_geometry``: a host copy of the aabb and the resolution (read back with a wait on the
    current stream)."""
    host_wait = True

    def __init__(self, device):
        from tests.test_gpu_occgrid import _grid
        self.device = device
        self.binaries = torch.from_numpy(_grid(32, seed=32))[None].to(device)
        o, d = _points(device, seed=13)
        self.o = (o / o.norm(dim=1, keepdim=True) * 4.0).contiguous()
        self.d = (d * 0.2 - self.o)
        self.d = (self.d / self.d.norm(dim=1, keepdim=True)).contiguous()

    def make(self):
        from quadraturefields_amd.estimators import OccGridEstimator
        est = OccGridEstimator(roi_aabb=[-1.5] * 3 + [1.5] * 3, resolution=32, levels=1).to(self.device)
        est.binaries.copy_(self.binaries)
        return est

    def use(self, est):
        return est.sampling(self.o, self.d, render_step_size=0.02)

    def cached(self, est):
        return getattr(est, "_geo_cache", None) is not None


OWNERS = {
    "ngp-fp16-copies": lambda dev: _NGPOwner(dev, "fp16"),
    "ngp-bf16-copies": lambda dev: _NGPOwner(dev, "bf16"),
    "sg-fp16-copies": lambda dev: _NGPOwner(dev, "fp16", lobes=2),
    "ngp-fp32-aabb": lambda dev: _NGPOwner(dev, "fp32"),
    "deform-fp16-table": _DeformOwner,
    "texel-records": _TextureOwner,
    "triangle-records": _TriangleRecordOwner,
    "estimator-geometry": _EstimatorOwner,
}


def _equal(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert sh.same_bits(g, w), f"{what}: output {i} differs from the synchronised run " \
                                   f"({int((g != w).sum())} of {g.numel()} elements)"


def _synchronised(owner):
    """(a reference owner, its result), fully synchronised.  ``ref`` stays alive and the allocator's free blocks go back
    to the driver: a block that an earlier test freed with the right bytes still in it, handed to the object under test,
    would make an unordered read come out right."""
    ref = owner.make()
    want = tuple(t.clone() for t in owner.use(ref))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return ref, want


@pytest.mark.parametrize("name", list(OWNERS))
def test_cache_built_on_a_side_stream_is_ordered_for_the_default_stream(device, name):
    owner = OWNERS[name](device)
    ref, want = _synchronised(owner)
    obj = owner.make()
    assert not owner.cached(obj)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=device)
    with torch.cuda.stream(s):
        sh.delay(DELAY_MS)
        on_side = owner.use(obj)                       # the hidden state is built here, behind the delay
    assert owner.cached(obj)
    at_once = owner.use(obj)                           # default stream, no synchronisation by the caller
    busy = not s.query()
    torch.cuda.synchronize()
    assert busy or owner.host_wait, "delay too short: the build had finished before the other stream was asked"
    _equal(on_side, want, f"{name}, building stream")
    _equal(at_once, want, f"{name}, default stream right after the build was enqueued elsewhere")


@pytest.mark.parametrize("name", list(OWNERS))
def test_cache_built_on_the_default_stream_is_ordered_for_a_side_stream(device, name):
    owner = OWNERS[name](device)
    ref, want = _synchronised(owner)
    obj = owner.make()
    torch.cuda.synchronize()
    sh.delay(DELAY_MS)
    on_default = owner.use(obj)
    s = torch.cuda.Stream(device=device)
    with torch.cuda.stream(s):
        at_once = owner.use(obj)
    busy = not torch.cuda.default_stream().query()
    torch.cuda.synchronize()
    assert busy or owner.host_wait, "delay too short: the build had finished before the other stream was asked"
    _equal(on_default, want, f"{name}, building (default) stream")
    _equal(at_once, want, f"{name}, side stream right after the build was enqueued on the default stream")


def _adam_step(owner, obj, seed=21):
    from quadraturefields_amd.optim import Adam
    params = owner.params(obj)
    g = torch.Generator(device=params[0].device).manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device=p.device, dtype=p.dtype) * 1e-2
    Adam(params, lr=1e-2, eps=1e-15).step()


@pytest.mark.parametrize("name", ["ngp-fp16-copies", "sg-fp16-copies", "deform-fp16-table"])
def test_cache_rebuilt_after_an_adam_step_on_another_stream(device, name):
    """``optim.Adam.step`` on stream A changes the parameters in place; the evaluation on stream B (which the caller has
    made wait for A: the parameters are the caller's) rebuilds the copies there; the default stream (made to wait for A
    too, not for B) then evaluates at once.  The old copy set is dropped while nothing orders B and the default stream."""
    owner = OWNERS[name](device)
    ref = owner.make()
    owner.use(ref)
    _adam_step(owner, ref)
    want = tuple(t.clone() for t in owner.use(ref))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()              # see _synchronised

    obj = owner.make()
    before = owner.use(obj)                             # copies of the OLD parameters exist, built on the default stream
    torch.cuda.synchronize()
    assert not sh.same_bits(before[0], want[0]), "the step changes nothing: the case has no power"
    a, b = torch.cuda.Stream(device=device), torch.cuda.Stream(device=device)
    with torch.cuda.stream(a):
        sh.delay(DELAY_MS)
        _adam_step(owner, obj)
    with torch.cuda.stream(b):
        b.wait_stream(a)
        sh.delay(DELAY_MS)                              # the rebuild is still far off when the default stream asks
        on_b = owner.use(obj)                           # rebuilt here
    torch.cuda.current_stream().wait_stream(a)
    at_once = owner.use(obj)
    busy = not b.query()
    torch.cuda.synchronize()
    assert busy, "delay too short: the rebuild had finished before the default stream was asked"
    _equal(on_b, want, f"{name}, rebuilding stream")
    _equal(at_once, want, f"{name}, default stream right after the rebuild was enqueued elsewhere")


# ------------------------------------------------------------------------------------------------ scratch per stream
W, H, K = 40, 24, 25


@pytest.fixture(scope="module")
def frame_scene(device):
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from tests.test_gpu_hit_bins import _field
    mesh = synthetic.shell_mesh(n_shells=4, subdivisions=3)
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=K)
    focal = synthetic.lego_focal(800) * W / 800.0
    views = []
    for c2w in synthetic.orbit_cameras(4, seed=11):
        o, d = synthetic.camera_rays(c2w, focal, W, H, device=device)
        views.append((o, d, make_camera(c2w, focal, W, H)))
    return mi, _field(device), views


def _frame_out(ri, r):
    rgb, alpha, depth, frame = r
    return (rgb.clone(), alpha.clone(), depth.clone(), frame.hit_count.clone(), frame.tile_base.clone()), frame


@pytest.mark.parametrize("route", ["lists", "bins"])
def test_two_frames_in_flight_on_two_streams_share_no_scratch(device, frame_scene, route):
    from quadraturefields_amd.render import FrameRenderer
    mi, field, views = frame_scene
    ri = mi.rayintersector
    fr = FrameRenderer(mi, field)
    ri._raster_backoff = 0
    ri.hit_bins = route == "bins"
    try:
        want = []
        for o, d, cam in views[:2]:
            assert ri.fused_frame_ready(cam, K)
            if route == "bins":
                assert ri._hit_bins_ready(K, cam)
            out, frame = _frame_out(ri, fr.render_async(o, d, cam))
            torch.cuda.synchronize()
            want.append((out, ri.frame_samples(frame)))
        assert not sh.same_bits(want[0][0][0], want[1][0][0]), "the two cameras give the same frame"
        streams = [torch.cuda.Stream(device=device), torch.cuda.Stream(device=device)]
        in_flight = []
        for (o, d, cam), s in zip(views[:2], streams):
            with torch.cuda.stream(s):
                sh.delay(DELAY_MS)
                in_flight.append(fr.render_async(o, d, cam))
        busy = [not s.query() for s in streams]
        got = []
        for r, s in zip(in_flight, streams):
            s.synchronize()
            out, frame = _frame_out(ri, r)
            got.append((out, ri.frame_samples(frame)))
        torch.cuda.synchronize()
        assert all(busy), "delay too short: a frame had finished before the other was enqueued"
        for i in range(2):
            _equal(got[i][0], want[i][0], f"frame {i} ({route})")
            assert got[i][1] == want[i][1], (i, got[i][1], want[i][1])
    finally:
        ri.hit_bins = True
        ri._settle_fused_policy(0)


# ------------------------------------------------------------------------------------------------ front / back pipeline
def test_front_back_pipeline_equals_the_sequential_frames(device, frame_scene):
    """bench.py's ``--pipeline 2`` loop at 40x24: ``Stages.begin`` on a front stream, ``Stages.finish`` on a back stream,
    ``scratch_slot`` alternating -- four consecutive frames, each bit-equal to ``Stages.frame`` run on its own."""
    import bench
    mi, field, views = frame_scene
    ri = mi.rayintersector
    assert bench.MAX_HITS == K
    stages = bench.Stages(mi, field, width=W)
    ri._raster_backoff = 0
    want = []
    for o, d, cam in views:
        rgb, alpha, depth, n = stages.frame(o, d, cam)
        torch.cuda.synchronize()
        want.append(((rgb.clone(), alpha.clone(), depth.clone()), n))
    front, back = torch.cuda.Stream(device=device), torch.cuda.Stream(device=device)
    got, prev = [], None

    def complete(begun):
        rgb, alpha, depth, n = stages.finish(begun)
        got.append(((rgb, alpha, depth), n))

    try:
        with torch.cuda.stream(front):
            sh.delay(DELAY_MS)
        for i, (o, d, cam) in enumerate(views):
            ri.scratch_slot = i & 1
            with torch.cuda.stream(front):
                begun = stages.begin(o, d, cam)
            if prev is not None:
                with torch.cuda.stream(back):
                    complete(prev)
            prev = begun
        with torch.cuda.stream(back):
            complete(prev)
    finally:
        ri.scratch_slot = 0
    back.synchronize()
    front.synchronize()
    torch.cuda.synchronize()
    assert len(got) == len(want) == 4
    for i in range(4):
        _equal(got[i][0], want[i][0], f"pipelined frame {i}")
        assert got[i][1] == want[i][1], (i, got[i][1], want[i][1])
