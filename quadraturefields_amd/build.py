"""In-tree build of libqf_hip.so for gfx950 (hipcc, no cmake): ``python -m quadraturefields_amd.build``.

The shared library is the C-ABI drop-in boundary declared in ``include/qf_hip.h``; it links only
against the HIP runtime.  The built ``.so`` stays inside the package directory so it travels with the
source snapshot to the GPU box.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
OBJ_DIR = os.path.join(CSRC, "_obj")
LIB_PATH = os.path.join(PKG_DIR, "libqf_hip.so")
ARCH = "gfx950"

# (source, extra flags).  No FMA contraction in the index-exact stages (exact_common.h: bvh_traverse, raster, sample_pack,
# texture, baked_frame, vertex_baked, vertex_train, vertex_quant, front_frame, grid_march and volumetric carry every integer-deciding comparison), bake.hip (the fp32 codecs), texel_fill.hip (the fp64 rules of the texel-position
# map), marching_cubes.hip (the fp32 vertex rule and the fp64 face decider), vertex_clustering.hip (the fp64 cell, mean
# and quadric rules), mesh_compact.hip (integer rules only; the flag keeps it with its neighbour), mesh_subdivide.hip (the
# fp64 midpoint is one add and one multiply, never a fused one), mesh_decimate.hip (the fp64 quadric, point, cost and
# side rules), uv_atlas.hip (the fp64 measure, class and corner rules) and bvh_build_device.hip (the fp32 Morton
# keys of the device BVH build) and closest_point.hip (the fp64 region walk, point and distance rules).  mesh_manifold.hip has no arithmetic at all and carries no flag;
# mesh_weld.hip carries it for the fp64 cell quotient and distance test of the weld, mesh_sample.hip for the fp64 measure,
# quotient, position and point rules of surface sampling, vertex_fit.hip for the fp64 sums, products and quotients of the
# surface fit of the vertex table, each rounded on its own.
SOURCES = [
    ("field_eval.hip", []),
    ("field_eval_bf16.hip", []),
    ("grid_extract.hip", []),
    ("grid_backward.hip", []),
    ("mlp_train.hip", []),
    ("field_train.hip", []),
    ("scan.hip", []),
    ("composite.hip", []),
    ("distortion.hip", []),
    ("optim.hip", []),
    ("frame_metrics.hip", []),
    ("bvh_traverse.hip", ["-ffp-contract=off"]),
    ("raster.hip", ["-ffp-contract=off"]),
    ("sample_pack.hip", ["-ffp-contract=off"]),
    ("texture.hip", ["-ffp-contract=off"]),
    ("baked_frame.hip", ["-ffp-contract=off"]),
    ("vertex_baked.hip", ["-ffp-contract=off"]),
    ("vertex_train.hip", ["-ffp-contract=off"]),
    ("vertex_quant.hip", ["-ffp-contract=off"]),
    ("front_frame.hip", ["-ffp-contract=off"]),
    ("bake.hip", ["-ffp-contract=off"]),
    ("grid_march.hip", ["-ffp-contract=off"]),
    ("volumetric.hip", ["-ffp-contract=off"]),
    ("texel_fill.hip", ["-ffp-contract=off"]),
    ("marching_cubes.hip", ["-ffp-contract=off"]),
    ("vertex_clustering.hip", ["-ffp-contract=off"]),
    ("mesh_compact.hip", ["-ffp-contract=off"]),
    ("mesh_subdivide.hip", ["-ffp-contract=off"]),
    ("mesh_decimate.hip", ["-ffp-contract=off"]),
    ("mesh_manifold.hip", []),     # no -ffp-contract flag: the file has no floating-point operation to contract
    ("mesh_weld.hip", ["-ffp-contract=off"]),      # the fp64 cell quotient and distance test of the weld
    ("mesh_sample.hip", ["-ffp-contract=off"]),    # the fp64 measure, position, barycentric and point rules
    ("vertex_fit.hip", ["-ffp-contract=off"]),     # the fp64 gram, right-hand side, operator, dot and update rules
    ("uv_atlas.hip", ["-ffp-contract=off"]),
    ("bvh_build_device.hip", ["-ffp-contract=off"]),
    ("closest_point.hip", ["-ffp-contract=off"]),
    ("bvh_build.cpp", ["-x", "hip"]),
    ("misc.cpp", ["-x", "hip"]),
    ("frame.cpp", ["-x", "hip"]),
]
COMMON = os.environ.get("QF_EXTRA_HIPCC_FLAGS", "").split() + ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-I" + os.path.join(ROOT, "include"),
          "-I" + CSRC, "-Wall", "-Wno-unused-function"]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def _deps(src: str):
    deps = [os.path.join(CSRC, src), os.path.join(ROOT, "include", "qf_hip.h"),
            os.path.join(ROOT, "include", "qf_vertex_baked.h"), os.path.join(ROOT, "include", "qf_vertex_train.h"),
            os.path.join(ROOT, "include", "qf_vertex_quant.h"), os.path.join(ROOT, "include", "qf_mesh_compact.h"),
            os.path.join(ROOT, "include", "qf_mesh_subdivide.h"), os.path.join(ROOT, "include", "qf_mesh_decimate.h"),
            os.path.join(ROOT, "include", "qf_mesh_decimate_open.h"), os.path.join(ROOT, "include", "qf_mesh_manifold.h"),
            os.path.join(ROOT, "include", "qf_closest_point.h"), os.path.join(ROOT, "include", "qf_mesh_weld.h"),
            os.path.join(ROOT, "include", "qf_mesh_sample.h"), os.path.join(ROOT, "include", "qf_vertex_fit.h"),
            os.path.abspath(__file__)]
    deps += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return deps


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _obj(src: str) -> str:
    return os.path.join(OBJ_DIR, os.path.splitext(src)[0] + ".o")


def _compile(item):
    src, extra = item
    obj = _obj(src)
    if not _stale(obj, _deps(src)):
        return obj, False
    cmd = [_hipcc()] + COMMON + extra + ["-c", os.path.join(CSRC, src), "-o", obj]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (src, " ".join(cmd), proc.stderr))
    if proc.stderr.strip():
        sys.stderr.write(proc.stderr)
    return obj, True


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 and link libqf_hip.so; returns its path."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    # --force clears every object; otherwise only those of sources that are gone (tools that link _obj/*.o would pick
    # up their symbols a second time)
    keep = set() if force else {_obj(src) for src, _ in SOURCES}
    for f in os.listdir(OBJ_DIR):
        if os.path.join(OBJ_DIR, f) not in keep:
            os.remove(os.path.join(OBJ_DIR, f))
    with ThreadPoolExecutor(max_workers=4) as pool:
        results = list(pool.map(_compile, SOURCES))
    objs = [o for o, _ in results]
    if any(changed for _, changed in results) or _stale(LIB_PATH, objs):
        cmd = [_hipcc(), "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", LIB_PATH] + objs
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError("link failed:\n%s\n%s" % (" ".join(cmd), proc.stderr))
        if verbose:
            print("linked", LIB_PATH)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
