"""Every launch of ``quadraturefields_amd/csrc`` whose grid is capped by the CU count, so that a workgroup loops over the
work (``for (...; i += gridDim.x * blockDim.x)``, or per chunk, per tile, per block of rays): one row per launch, the size
above which the second trip of that loop runs, and the test that runs it.  No tests in here, no device.

The rows are the hits of ``grep -n "qf_grid_1d(\\|QF_SIMPLE_LAUNCH(" csrc/*`` and the launches capped by
``qf_cu_count_cached()`` directly.  Left out: the field kernels dealt by ``qf_group_range`` (``qf_field_blocks`` in
field_eval.hip, field_eval_bf16.hip, field_train.hip, grid_extract.hip), which ``test_dealing_routes_agree`` and the
``sweep`` tests own.

``cap_items(row, cu)`` is the number of items one sweep of the capped grid covers; ``past(row, cu)`` is a size with which
some workgroups take two trips, others one, and the last trip is ragged.  ``launch`` is the launch expression as written
in ``file``: ``tests/test_grid_caps_host.py`` fails when it no longer appears there ``times`` times, which names the row to
revisit.  ``verdict`` says which test exceeds the cap (``covered by <test id> (<size>)``) or why no valid input can
(``unreachable because ...``)."""
from collections import namedtuple

import numpy as np

Row = namedtuple("Row", "key entry kernel file launch unit per_trip wg_per_cu verdict times")

NEW = "tests/test_gpu_grid_caps.py"


def _row(key, entry, kernel, file, launch, unit, per_trip, wg_per_cu, verdict, times=1):
    return Row(key, entry, kernel, file, launch, unit, per_trip, wg_per_cu, verdict, times)


def _simple(key, entry, kernel, file, count, unit, verdict, times=1):
    """QF_SIMPLE_LAUNCH(kernel, count, ...): qf_grid_1d(count, 256), 8 workgroups per CU."""
    return _row(key, entry, kernel, file, f"QF_SIMPLE_LAUNCH({kernel}, {count},", unit, 256, 8, verdict, times)


def _g256(key, entry, kernel, file, count, unit, verdict, block="256", times=1):
    """hipLaunchKernelGGL(kernel, dim3(qf_grid_1d(count, 256)), ...): 8 workgroups per CU."""
    return _row(key, entry, kernel, file, f"hipLaunchKernelGGL({kernel}, dim3(qf_grid_1d({count}, {block}))", unit, 256, 8,
                verdict, times)


_MLP = "covered by tests/test_gpu_mlp_backward.py (sizes 3*S+7 and 2^20+5 with S = 64 CU: 49 159 and 1 048 581 points)"
_GRIDB = "covered by tests/test_gpu_grid_backward.py (n = 2^15+8193 and 2^20+5 on every scatter route)"

ROWS = [
    # ------------------------------------------------------------------------------------------------- composite.hip
    _simple("mark_boundaries", "qf_mark_pack_boundaries", "mark_boundaries_kernel", "composite.hip", "n", "samples",
            f"covered by {NEW}::test_whole_equals_pieces[mark_pack_boundaries]"),
    _simple("exp_integration", "qf_exponential_integration", "exp_integration_kernel", "composite.hip", "n_seg * c",
            "segments x channels", f"covered by {NEW}::test_whole_equals_pieces[exponential_integration]"),
    _simple("sum_reduce", "qf_sum_reduce", "sum_reduce_kernel", "composite.hip", "n_seg * c", "segments x channels",
            f"covered by {NEW}::test_segment_sums_against_reduceat"),
    _simple("fill_background", "qf_derive_properties", "fill_background_kernel", "composite.hip", "n_rays", "rays",
            f"covered by {NEW}::test_derive_properties_fills_every_ray"),
    _row("derive_properties", "qf_derive_properties", "derive_properties_kernel", "composite.hip",
         "hipLaunchKernelGGL(derive_properties_kernel, dim3((unsigned)(n_chunks < 65536 ? n_chunks : 65536))",
         "samples (chunks of 1024; 65 536 chunks whatever the CU count)", 1024, None,
         "unreachable because the cap is 65 536 chunks = 67 108 864 samples, seventeen 800x800 frames of 25 hits in one call; "
         "the callers window a frame at 160 000 rays (4 M samples)"),
    _simple("pack_info", "qf_pack_info", "pack_info_kernel", "composite.hip", "n_rays", "rays",
            f"covered by {NEW}::test_segment_sums_against_reduceat"),
    _simple("exclusive_scan", "qf_exclusive_scan", "exclusive_scan_kernel", "composite.hip", "n_rays", "rays",
            f"covered by {NEW}::test_whole_equals_pieces[exclusive_scan]"),
    _simple("accumulate", "qf_accumulate_along_rays", "accumulate_kernel", "composite.hip", "n_rays * c", "rays x channels",
            f"covered by {NEW}::test_segment_sums_against_reduceat"),
    _simple("render_from_density", "qf_render_from_density", "render_from_density_kernel", "composite.hip", "n_rays", "rays",
            f"covered by {NEW}::test_whole_equals_pieces[render_from_density]"),
    _simple("apply_deformation", "qf_apply_deformation", "apply_deformation_kernel", "composite.hip", "n", "samples",
            f"covered by {NEW}::test_whole_equals_pieces[apply_deformation]"),
    _g256("generate_rays", "qf_generate_rays", "generate_rays_kernel", "composite.hip", "n", "pixels",
          f"covered by {NEW}::test_generate_rays_past_the_cap"),
    _g256("scatter_max", "qf_scatter_max", "scatter_max_kernel", "composite.hip", "n", "values",
          f"covered by {NEW}::test_scatter_max_past_the_cap"),
    _g256("split_rays", "qf_split_layout", "split_rays_kernel", "composite.hip", "n_rays + 1", "rays",
          f"covered by {NEW}::test_split_layout_past_the_cap"),
    _row("update_d_merged", "qf_mesh_update_d (n >= 8192)", "mesh_update_d_merged_kernel", "composite.hip",
         "const int64_t cap = (int64_t)qf_cu_count_cached() * 8;\n        const unsigned grid = (unsigned)(chunks < cap ? chunks : cap);",
         "samples (chunks of 1024)", 1024, 8, f"covered by {NEW}::test_mesh_update_d_past_the_cap"),
    _g256("update_d_plain", "qf_mesh_update_d (n < 8192)", "mesh_update_d_kernel", "composite.hip", "d ? 4 * n : n",
          "threads (4 per sample with d)",
          "unreachable because the route takes n < 8192 samples, at most 32 764 threads, and the cap is 2048 CU >= 32 768 "
          "threads from 16 CUs on (the other way in, n_faces >= 2^31, needs a 32 GiB cache)"),
    _g256("derive_properties_backward", "qf_derive_properties_backward", "derive_properties_backward_kernel", "composite.hip",
          "n", "samples", "covered by tests/test_gpu_composite_backward.py::test_backward_vs_fp64[big-*] (2048 CU + 18 samples)"),
    # ----------------------------------------------------------------------------------------------- the tile compositors
    _row("vertex_tiles", "qf_vertex_composite_tiles / qf_frame_render_vertex_baked", "vertex_composite_tiles_kernel",
         "vertex_baked.hip", "hipLaunchKernelGGL(vertex_composite_tiles_kernel, dim3(qf_grid_1d(n_tiles * 64, 64 * kTileWaves))",
         "tiles", 4, 8, f"covered by {NEW}::test_tile_compositors_past_the_cap[vertex]"),
    _row("quant_tiles", "qf_vertex_quant_composite_tiles / qf_frame_render_vertex_quant", "vertex_quant_composite_tiles_kernel",
         "vertex_quant.hip",
         "hipLaunchKernelGGL(vertex_quant_composite_tiles_kernel, dim3(qf_grid_1d(n_tiles * 64, 64 * kTileWaves))",
         "tiles", 4, 8, f"covered by {NEW}::test_tile_compositors_past_the_cap[quant]"),
    _row("texture_tiles", "qf_texture_composite_tiles / qf_frame_render_baked", "texture_composite_tiles_kernel",
         "baked_frame.hip", "hipLaunchKernelGGL(texture_composite_tiles_kernel, dim3(qf_grid_1d(n_tiles * 64, 64 * kTileWaves))",
         "tiles", 4, 8, f"covered by {NEW}::test_tile_compositors_past_the_cap[texture]"),
    # ------------------------------------------------------------------------------------- vertex table, quantised table
    _simple("vertex_records", "qf_vertex_records_pack", "vertex_records_kernel", "vertex_baked.hip", "n_faces", "faces",
            f"covered by {NEW}::test_whole_equals_pieces[vertex_records_pack]"),
    _simple("vertex_shade32", "qf_vertex_shade_points (int32 ids)", "vertex_shade_points_kernel<int32_t>", "vertex_baked.hip",
            "n", "samples", f"covered by {NEW}::test_whole_equals_pieces[vertex_shade_points-int32]"),
    _simple("vertex_shade64", "qf_vertex_shade_points (int64 ids)", "vertex_shade_points_kernel<int64_t>", "vertex_baked.hip",
            "n", "samples", f"covered by {NEW}::test_whole_equals_pieces[vertex_shade_points-int64]"),
    _row("vertex_train", "qf_vertex_shade_points_backward", "vertex_shade_points_backward_kernel", "vertex_train.hip",
         "const dim3 grid(qf_grid_1d(n, kTrainThreads)), block(kTrainThreads);", "samples", 256, 8,
         f"covered by {NEW}::test_vertex_backward_past_the_cap"),
    _simple("quant_decode", "qf_vertex_quant_decode", "vertex_quant_decode_kernel", "vertex_quant.hip", "n_vertices",
            "vertices", f"covered by {NEW}::test_whole_equals_pieces[vertex_quant_decode]"),
    _simple("quant_shade32", "qf_vertex_quant_shade_points (int32 ids)", "vertex_quant_shade_points_kernel<int32_t>",
            "vertex_quant.hip", "n", "samples", f"covered by {NEW}::test_whole_equals_pieces[vertex_quant_shade_points-int32]"),
    _simple("quant_shade64", "qf_vertex_quant_shade_points (int64 ids)", "vertex_quant_shade_points_kernel<int64_t>",
            "vertex_quant.hip", "n", "samples", f"covered by {NEW}::test_whole_equals_pieces[vertex_quant_shade_points-int64]"),
    # ---------------------------------------------------------------------------------------------------- baked textures
    _simple("texel_records", "qf_texel_records_pack", "texel_records_kernel", "texture.hip", "n_faces", "faces",
            f"covered by {NEW}::test_whole_equals_pieces[texel_records_pack]"),
    _simple("texel_indices", "qf_texel_indices_packed", "texel_indices_packed_kernel", "texture.hip", "n", "samples",
            f"covered by {NEW}::test_whole_equals_pieces[texel_indices_packed]"),
    _simple("texture_fetch", "qf_texture_fetch", "texture_fetch_kernel", "texture.hip", "n", "samples",
            f"covered by {NEW}::test_whole_equals_pieces[texture_fetch]"),
    _simple("texture_pack", "qf_texture_pack", "texture_pack_kernel", "texture.hip", "(int64_t)t.size * t.size", "texels",
            f"covered by {NEW}::test_texture_pack_past_the_cap"),
    _simple("texture_shade_packed", "qf_texture_shade_packed", "(texture_shade_packed_kernel<false, int64_t>)", "texture.hip",
            "n", "samples", f"covered by {NEW}::test_whole_equals_pieces[texture_shade_packed]"),
    _simple("texture_shade32", "qf_texture_shade_points (int32 ids)", "(texture_shade_packed_kernel<true, int32_t>)",
            "texture.hip", "n", "samples", f"covered by {NEW}::test_whole_equals_pieces[texture_shade_points-int32]"),
    _simple("texture_shade64", "qf_texture_shade_points (int64 ids)", "(texture_shade_packed_kernel<true, int64_t>)",
            "texture.hip", "n", "samples", f"covered by {NEW}::test_whole_equals_pieces[texture_shade_points-int64]"),
    _simple("bake_encode", "qf_bake_encode_texels", "bake_encode_kernel", "bake.hip", "capacity", "texel slots",
            f"covered by {NEW}::test_whole_equals_pieces[bake_encode_texels]"),
    # ---------------------------------------------------------------------------------------- occupancy and volumetric
    _row("grid_march", "qf_grid_march_count, qf_grid_march_write", "grid_march_kernel", "grid_march.hip",
         "hipLaunchKernelGGL(grid_march_kernel, dim3(qf_grid_1d(n_rays, 64, 64))", "rays", 64, 64,
         f"covered by {NEW}::test_occupancy_march_past_the_cap", 2),
    _row("march_round_count", "qf_grid_march_round_count", "march_round_kernel<false>", "volumetric.hip",
         "hipLaunchKernelGGL(march_round_kernel<false>, dim3(qf_grid_1d(n_rays, 64, 64))", "rays", 64, 64,
         f"covered by {NEW}::test_volumetric_round_past_the_cap"),
    _row("march_round_write", "qf_grid_march_round_write", "march_round_kernel<true>", "volumetric.hip",
         "hipLaunchKernelGGL(march_round_kernel<true>, dim3(qf_grid_1d(n_rays, 64, 64))", "rays", 64, 64,
         f"covered by {NEW}::test_volumetric_round_past_the_cap"),
    _simple("volumetric_accumulate", "qf_volumetric_accumulate", "volumetric_accumulate_kernel", "volumetric.hip", "n_rays",
            "rays", f"covered by {NEW}::test_volumetric_round_past_the_cap"),
    _simple("mark_visited", "qf_mark_visited_cells", "mark_visited_kernel", "volumetric.hip", "n", "points",
            f"covered by {NEW}::test_mark_visited_cells_past_the_cap"),
    # -------------------------------------------------------------------------------------------------- fields, training
    _g256("grid_encode", "qf_grid_encode", "grid_encode_kernel", "field_eval.hip", "n * 16", "threads (16 per point)",
          f"covered by {NEW}::test_whole_equals_pieces[grid_encode]"),
    _g256("sg_features_to_rgb", "qf_sg_features_to_rgb", "sg_features_to_rgb_kernel", "field_eval.hip", "n", "samples",
          f"covered by {NEW}::test_whole_equals_pieces[sg_features_to_rgb]"),
    _g256("sg_features_to_rgb_backward", "qf_sg_features_to_rgb_backward", "sg_features_to_rgb_backward_kernel",
          "mlp_train.hip", "n", "samples", _MLP),
    _row("ngp_sg_mlp_backward", "qf_ngp_mlp_backward, qf_sg_mlp_backward", "ngp_mlp_backward_kernel, sg_mlp_backward_kernel",
         "mlp_train.hip", "const int64_t cap = (int64_t)qf_cu_count_cached();", "points (groups of 16, one per wave)", 64, 1,
         _MLP, 2),
    _row("deform_mlp_backward", "qf_deform_mlp_backward", "deform_mlp_backward_kernel", "mlp_train.hip",
         "const int64_t cap = (int64_t)qf_cu_count_cached() * 2;", "points (groups of 16, one per wave)", 64, 2, _MLP),
    _row("grid_backward_table", "qf_grid_encode_backward", "grid_backward_table_kernel", "grid_backward.hip",
         "hipLaunchKernelGGL(grid_backward_table_kernel, dim3(qf_grid_1d(n * 64, 256, 32))", "threads (64 per point)", 256, 32,
         _GRIDB),
    _g256("grid_backward_input", "qf_grid_encode_backward, qf_grid_encode_backward_ws", "grid_backward_input_kernel",
          "grid_backward.hip", "n", "points", _GRIDB, times=2),
    _row("grid_double_backward_table_ws", "qf_grid_encode_double_backward (workspace route)",
         "grid_double_backward_table_kernel", "grid_backward.hip",
         "hipLaunchKernelGGL(grid_double_backward_table_kernel, dim3(qf_grid_1d(n * atomics.n * 4, 256, 32))",
         "threads (4 per point and atomic level)", 256, 32, _GRIDB),
    _row("grid_backward_table_ws", "qf_grid_encode_backward_ws", "grid_backward_table_kernel", "grid_backward.hip",
         "hipLaunchKernelGGL(grid_backward_table_kernel, dim3(qf_grid_1d(n * atomics.n * 4, 256, 32))",
         "threads (4 per point and atomic level)", 256, 32, _GRIDB),
    _row("grid_sorted_levels", "qf_grid_encode_backward_ws (sorted levels)", "the per-level scatter kernels", "grid_backward.hip",
         "const int per_level = 3 * qf_cu_count_cached() / 8 > 16 ? 3 * qf_cu_count_cached() / 8 : 16;",
         "workgroups per sorted level", None, None, _GRIDB + "; tests/test_grid_backward_reference.py pins the expression"),
    _g256("grid_double_backward", "qf_grid_encode_double_backward", "grid_double_backward_kernel", "grid_backward.hip", "n",
          "points", _GRIDB),
    _row("grid_double_backward_table", "qf_grid_encode_double_backward", "grid_double_backward_table_kernel",
         "grid_backward.hip", "hipLaunchKernelGGL(grid_double_backward_table_kernel, dim3(qf_grid_1d(n * 64, 256, 32))",
         "threads (64 per point)", 256, 32, _GRIDB),
    _row("adam", "qf_adam_step", "adam_kernel", "optim.hip",
         "hipLaunchKernelGGL(adam_kernel, dim3(qf_grid_1d((n + 3) / 4, 256, 16))", "floats (4 per thread)", 1024, 16,
         f"covered by {NEW}::test_adam_past_the_cap"),
    # ------------------------------------------------------------------------------------------- frames, meshes, baking
    _simple("frame_images_u8", "qf_frame_images_u8", "frame_images_u8_kernel", "frame_metrics.hip", "3 * n_pixels",
            "pixel channels", f"covered by {NEW}::test_whole_equals_pieces[frame_images_u8]"),
    _simple("mark_hit_faces", "qf_mark_hit_faces", "mark_hit_faces_kernel", "mesh_compact.hip", "n_slots", "hit slots",
            f"covered by {NEW}::test_whole_equals_pieces[mark_hit_faces]"),
    _simple("resort", "qf_resort_by_depth", "resort_kernel", "sample_pack.hip", "n", "samples",
            f"covered by {NEW}::test_whole_equals_pieces[resort_by_depth]"),
    _row("resort_samples", "qf_resort_samples", "resort_samples_kernel", "sample_pack.hip",
         "hipLaunchKernelGGL(resort_samples_kernel, dim3((unsigned)(n_chunks < 65536 ? n_chunks : 65536))",
         "samples (chunks; 65 536 chunks whatever the CU count)", 1024, None,
         "unreachable because the cap is 65 536 chunks, 67 M samples: the same bound as derive_properties_kernel's"),
    _g256("camera_rays_check", "qf_bvh_intersect_camera and the frame entry points", "camera_rays_check_kernel", "raster.hip",
          "n_rays", "rays", f"covered by {NEW}::test_camera_passes_past_the_cap[plain]"),
    _g256("slab_ray_records", "qf_bvh_intersect_camera (depth slabs)", "slab_ray_records_kernel", "raster.hip", "n_rays",
          "rays", f"covered by {NEW}::test_camera_passes_past_the_cap[slabs]"),
    _row("raster_chunk_grid", "qf_bvh_intersect_camera (culled and slab passes)", "raster_culled_kernel, raster_slab_kernel",
         "raster.hip", "const int64_t cap = (int64_t)qf_cu_count_cached() * 8;\n    return (unsigned)(items < cap ? items : cap);",
         "workgroups over the chunk list", None, 8,
         f"covered by {NEW}::test_camera_passes_past_the_cap[culled] and [slabs] (a mesh whose chunk list is longer than 8 CU)"),
    _g256("bvh_morton_keys", "qf_bvh_build_device", "morton_keys_kernel", "bvh_build_device.hip", "n_tri", "triangles",
          f"covered by {NEW}::test_device_bvh_past_the_cap", block="kBlock"),
    _g256("bvh_gather_tris", "qf_bvh_build_device", "gather_tris_kernel", "bvh_build_device.hip", "n_tri", "triangles",
          f"covered by {NEW}::test_device_bvh_past_the_cap", block="kBlock"),
    _g256("bvh_refit_tris", "qf_bvh_refit_device", "refit_tris_kernel", "bvh_build.cpp", "n_tri", "triangles",
          f"covered by {NEW}::test_device_bvh_past_the_cap"),
    _g256("texel_face_setup", "qf_texel_positions", "face_setup_kernel", "texel_fill.hip", "F", "faces",
          "covered by tests/test_gpu_texel_fill.py::test_bench_mesh_at_4096 (983 040 faces, 2 949 120 edges, 4096^2 texels)", block="kBlock"),
    _g256("texel_scan_add", "qf_texel_positions", "scan_add_kernel", "texel_fill.hip", "F", "faces",
          "covered by tests/test_gpu_texel_fill.py::test_bench_mesh_at_4096 (983 040 faces, 2 949 120 edges, 4096^2 texels)", block="kBlock"),
    _g256("texel_edges", "qf_texel_positions", "edges_kernel", "texel_fill.hip", "3 * F", "edges",
          "covered by tests/test_gpu_texel_fill.py::test_bench_mesh_at_4096 (983 040 faces, 2 949 120 edges, 4096^2 texels)", block="kBlock"),
    _row("texel_resolve", "qf_texel_positions", "resolve_kernel", "texel_fill.hip",
         "hipLaunchKernelGGL(resolve_kernel, dim3(qf_grid_1d(qf_div_up(hw, kResolveTexels), kBlock))", "texels (4 per thread)",
         1024, 8, "covered by tests/test_gpu_texel_fill.py::test_bench_mesh_at_4096 (983 040 faces, 2 949 120 edges, 4096^2 texels)"),
    _row("texel_cover", "qf_texel_positions", "cover_kernel", "texel_fill.hip",
         "hipLaunchKernelGGL(cover_kernel, dim3(qf_cu_count_cached() * 8), dim3(kBlock)", "workgroups (always 8 per CU)", None, 8,
         "covered by tests/test_gpu_texel_fill.py::test_bench_mesh_at_4096 (983 040 faces, 2 949 120 edges, 4096^2 texels)"),
    _g256("uv_histogram", "qf_uv_atlas", "histogram_kernel", "uv_atlas.hip", "F", "faces",
          f"covered by {NEW}::test_uv_atlas_histogram_past_the_cap", block="kBlock"),
]

BY_KEY = {r.key: r for r in ROWS}
assert len(BY_KEY) == len(ROWS)


def cap_items(row, cu):
    """Items one sweep of the row's capped grid covers on ``cu`` compute units."""
    if isinstance(row, str):
        row = BY_KEY[row]
    if row.per_trip is None:
        raise ValueError(f"{row.key}: the cap is not a count of items")
    if row.wg_per_cu is None:                      # capped at 65 536 workgroups whatever the chip
        return row.per_trip * 65536
    return row.per_trip * row.wg_per_cu * cu


def past(row, cu, tail=77):
    """cap + cap // 3 + an odd tail: some workgroups take two trips, others one, and the last trip is ragged."""
    assert tail % 2 == 1
    cap = cap_items(row, cu)
    return cap + cap // 3 + tail


# ---------------------------------------------------------------------------------- the ids of the qf_mesh_update_d tests
UPDATE_D_KINDS = ("seven", "distinct", "wrap")
UD_CHUNK, UD_SLOTS = 1024, 2048


def update_d_hash(keys) -> np.ndarray:
    """The home slot of a key in mesh_update_d_merged_kernel's table: ((uint32)key * 2654435761) >> 21."""
    return ((np.asarray(keys).astype(np.uint32) * np.uint32(2654435761)) >> np.uint32(21)).astype(np.int64)


def update_d_ids(kind, n):
    """(ids int64 [n], n_faces, number of ids out of range) of one id set:

    * ``seven``: 7 faces, every sample of a chunk lands in seven slots;
    * ``distinct``: 2^22 faces, a random injection with one repeat in 997: at least 1000 distinct keys in every full chunk;
    * ``wrap``: 50 000 faces; every chunk starts with eight distinct keys whose home slot is 2047, the last one, so that
      seven of them wrap to the slots 0..6, and eight keys of the home slots 2040..2046 in front of them.

    Five ids out of range (below 0, n_faces, beyond, +-2^40) sit in the first, a middle and the last chunks."""
    rng = np.random.default_rng(1000 + n % 997)
    if kind == "seven":
        n_faces = 7
        ids = rng.integers(0, n_faces, n)
    elif kind == "distinct":
        n_faces = 1 << 22
        assert n < n_faces
        ids = rng.permutation(n_faces)[:n].astype(np.int64)
        ids[5::997] = ids[4::997][:ids[5::997].shape[0]]
    elif kind == "wrap":
        n_faces = 50000
        ids = rng.integers(0, n_faces, n)
        h = update_d_hash(np.arange(n_faces))
        last, near = np.flatnonzero(h == UD_SLOTS - 1)[:8], np.flatnonzero((h >= UD_SLOTS - 8) & (h < UD_SLOTS - 1))[:8]
        assert last.shape[0] == 8 and near.shape[0] == 8
        for c0 in range(0, n - 16, UD_CHUNK):
            ids[c0:c0 + 8], ids[c0 + 8:c0 + 16] = last, near
    else:
        raise KeyError(kind)
    ids = ids.astype(np.int64)
    chunks = (n - 1) // UD_CHUNK
    at = sorted({17, min(3 * UD_CHUNK + 100, n - 1), (chunks // 2) * UD_CHUNK + 500, max(chunks - 1, 0) * UD_CHUNK + 724, n - 1})
    bad = np.array([-1, n_faces, n_faces + 12345, -2 ** 40, 2 ** 40], dtype=np.int64)
    for k, pos in enumerate(at):
        ids[pos] = bad[k]
    return ids, n_faces, len(at)


# ------------------------------------------------------------------------------------------------- fp64 references
def update_d_reference(d, w, ids, n_faces):
    """(sums fp64 [n_faces, 4], bound fp64 [n_faces, 4], samples per row) of qf_mesh_update_d into a zeroed cache: the fp64
    ``np.bincount`` of the fp32 products ``float32(d * w)`` (contraction is off in the kernel) and of ``w``; ids out of range
    are skipped.  ``bound`` = (k + 1) * 2^-24 * sum|term| for a row of k terms: any order of k fp32 additions."""
    d, w, ids = np.asarray(d, dtype=np.float32), np.asarray(w, dtype=np.float32), np.asarray(ids)
    ok = (ids >= 0) & (ids < n_faces)
    terms = np.concatenate([d * w[:, None], w[:, None]], axis=1)
    assert terms.dtype == np.float32
    k = np.bincount(ids[ok], minlength=n_faces)
    cols = range(4)
    ref = np.stack([np.bincount(ids[ok], weights=terms[ok, c].astype(np.float64), minlength=n_faces) for c in cols], axis=1)
    mag = np.stack([np.bincount(ids[ok], weights=np.abs(terms[ok, c]).astype(np.float64), minlength=n_faces) for c in cols], axis=1)
    return ref, (k[:, None] + 1) * 2.0 ** -24 * mag, k


def scatter_max_reference(fill, n_out, index, values):
    """``np.fmax.at`` into ``np.full(n_out, fill)``: NaN values and ids out of range are skipped."""
    index, values = np.asarray(index), np.asarray(values, dtype=np.float32)
    out = np.full(n_out, fill, dtype=np.float32)
    ok = (index >= 0) & (index < n_out)
    np.fmax.at(out, index[ok], values[ok])
    return out


def segment_sums(x, starts, counts):
    """fp64 sums of the rows of ``x`` [n, ...] over the segments (starts, counts) by ``np.add.reduceat``; empty segments 0."""
    x, starts, counts = np.asarray(x, dtype=np.float64), np.asarray(starts), np.asarray(counts)
    out = np.add.reduceat(np.concatenate([x, np.zeros((1,) + x.shape[1:])]), starts, axis=0)
    out[counts == 0] = 0.0
    return out
