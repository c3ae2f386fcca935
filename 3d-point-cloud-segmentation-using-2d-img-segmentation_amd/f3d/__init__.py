"""ctypes binding of libf3d_hip.so (include/f3d.h) -- the only way Python reaches the kernels.

There is deliberately no CPU fallback here: if the library is missing or no HIP
device is usable, every compute call raises ``F3DUnavailable``.

Two call styles, mirroring the C-ABI:
* NumPy in / NumPy out (host-pointer entry points) -- what the drop-in modules
  ``Fusion3DSeg.*`` use;
* ``*_dev`` methods taking raw device pointers (``tensor.data_ptr()``) and a
  stream handle -- what ``bench.py`` and device-resident pipelines use.
"""
import ctypes as C
import os
from pathlib import Path

import numpy as np

from f3d.tensors import depth_code, dtype_code, host_csr, index_code

__all__ = ['F3DError', 'F3DUnavailable', 'Context', 'default_context', 'library', 'library_path',
           'views_build', 'frustum_data', 'quat_inverse', 'VIEW_DOUBLES', 'F64', 'F32', 'FUSE_SORT', 'FUSE_GATHER']

F64, F32 = 0, 1
FUSE_SORT, FUSE_GATHER = 2, 4
OK, ERR_INVALID, ERR_HIP, ERR_INDEX, ERR_ZERO_QUAT, ERR_NOMEM = 0, -1, -2, -3, -4, -5
VIEW_DOUBLES = 88            # sizeof(f3d_view) / 8
OBB_DOUBLES = 15             # sizeof(f3d_obb) / 8
MAX_OBB = 4096
OBB_OK, OBB_FEW, OBB_DEFERRED = 0, 1, 2
NORM_PLAIN, NORM_FMA, NORM_HOST = 0, 1, 2   # how the fusion kernels take sqrt(v.dot(v)) (f3d.h F3D_NORM_*)
NORMALS_MAX_NN = 64          # F3D_NORMALS_MAX_NN: the largest max_nn of estimate_normals
QUAD_OK, QUAD_HORIZONTAL, QUAD_NO_CANDIDATE = 0, 1, 2   # per-instance status of door_window_quads (f3d.h F3D_QUAD_*)
QUADS_MAX_INST = 65535       # F3D_QUADS_MAX_INST
I64, I32 = 0, 1              # f3d_itype: the index type of mesh triangles
FEAT_F16, FEAT_F32 = 0, 1    # f3d_ftype: the element type of feature maps
FEAT_MAX_D = 4096            # the most channels of a feature row (f3d.h f3d_fuse_features)
VOTES_F64, VOTES_U16 = 0, 1  # f3d_vtype: the element type of a vote matrix handed to smooth_votes / smooth_segment
SMOOTH_MAX_COLS = 256        # the widest vote matrix smooth_votes / smooth_segment take
KNN_MAX_K = 32               # F3D_KNN_MAX_K: the largest k of knn_query / transfer_labels
TSDF_SCAN_TILE = 2048        # F3D_TSDF_SCAN_TILE: counts per tile of the extract scans (scanned by blocks of 256 threads)
ICP_CHUNK = 256              # F3D_ICP_CHUNK: source pixels per chunk of the ICP sums (one wave per chunk)
ICP_NSUMS = 29               # F3D_ICP_NSUMS: 21 J J^T products, 6 J r, r r and the pair count
ICP_NSUMS_COLOR = 58         # F3D_ICP_NSUMS_COLOR: the 29 geometric sums, then the 29 of the photometric pairs
ICP_PIVOT_EPS = 1e-10        # F3D_ICP_PIVOT_EPS: the smallest Cholesky pivot, as a fraction of the largest diagonal entry
ICP_OK, ICP_LOST = 0, 1      # status of an icp round (f3d.h F3D_ICP_*)
ICP_MAX_LEVELS = 6           # F3D_ICP_MAX_LEVELS: the most levels of one icp_levels call
CLOUD_ICP_PLANE, CLOUD_ICP_POINT = 0, 1   # mode of cloud_icp_sums / cloud_icp (f3d.h F3D_CLOUD_ICP_*)


class IcpLevel(C.Structure):
    """f3d_icp_level (f3d.h): the source frame, the model and the rounds of one level of icp_levels."""
    _fields_ = [('depth', C.c_void_p), ('depth_type', C.c_int), ('h', C.c_int), ('w', C.c_int), ('K', C.c_double * 9), ('depth_scale', C.c_double),
                ('model_vertex', C.c_void_p), ('model_normal', C.c_void_p), ('model_intensity', C.c_void_p), ('hm', C.c_int), ('wm', C.c_int),
                ('model_view', C.c_void_p), ('max_dist', C.c_double), ('iterations', C.c_int), ('min_pairs', C.c_int)]


class F3DError(RuntimeError):
    pass


class F3DUnavailable(F3DError):
    """libf3d_hip.so is not built/loadable or there is no HIP device."""


_lib = None


def library_path():
    """The in-tree build.  F3D_LIBRARY names another build of the same library (the A/B timing scripts under scripts/ point the
    loader at a variant this way instead of overwriting the product's file)."""
    alt = os.environ.get('F3D_LIBRARY')
    return Path(alt).resolve() if alt else Path(__file__).resolve().parent / 'libf3d_hip.so'


def library():
    """Load libf3d_hip.so once and declare every prototype of include/f3d.h."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not path.is_file():
        raise F3DUnavailable(f'{path} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                             f'(or `make -C {path.parent.parent / "csrc"}`); there is no CPU fallback')
    try:                         # share torch's HIP runtime when torch is in the process (same SONAME)
        import torch  # noqa: F401
    except Exception:            # torch is plumbing, not a requirement of the binding
        pass
    try:
        lib = C.CDLL(str(path), mode=getattr(os, 'RTLD_NOW', 2))
    except OSError as exc:
        raise F3DUnavailable(f'cannot load {path}: {exc}') from exc

    vp, i32, i64, dbl, flt = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_float
    protos = {
        'f3d_version': (i32, []),
        'f3d_ctx_create': (vp, [i32]),
        'f3d_ctx_destroy': (None, [vp]),
        'f3d_last_error': (C.c_char_p, [vp]),
        'f3d_ctx_synchronize': (i32, [vp]),
        'f3d_ctx_stream': (vp, [vp]),
        'f3d_ctx_reserve': (i32, [vp, i64, i32, i32, i32]),
        'f3d_ctx_set_strict': (i32, [vp, i32]),
        'f3d_ctx_alloc_count': (C.c_longlong, [vp]),
        'f3d_quat_inverse': (i32, [vp, vp]),
        'f3d_frustum_data': (i32, [vp, dbl, dbl, vp, vp, i32, vp, vp, vp]),
        'f3d_views_build': (i32, [vp, dbl, dbl, vp, vp, i32, dbl, vp]),
        'f3d_rotate_f64': (i32, [vp, vp, i64, vp, vp]),
        'f3d_rotate_f64_dev': (i32, [vp, vp, i64, vp, vp, vp]),
        'f3d_points2pixel_f64': (i32, [vp, vp, i64, vp, vp, vp, vp]),
        'f3d_points2pixel_dev': (i32, [vp, vp, i32, i64, vp, vp, vp, vp, vp]),
        'f3d_inside_polyhedra_f64': (i32, [vp, vp, i64, vp, vp, i32, vp]),
        'f3d_inside_polyhedra_dev': (i32, [vp, vp, i32, i64, vp, vp, i32, vp, vp]),
        'f3d_project_view_f64': (i32, [vp, vp, i64, vp, vp, vp]),
        'f3d_project_view_dev': (i32, [vp, vp, i32, i64, vp, vp, vp, vp]),
        'f3d_project_vote_argmax': (i32, [vp, vp, i32, i64, vp, i32, vp, i32, i32, i32, vp, i32, dbl, vp, vp]),
        'f3d_project_vote_argmax_dev': (i32, [vp, vp, i32, i64, vp, i32, vp, i32, i32, i32, vp, i32, dbl, vp, vp, C.c_uint, vp, vp]),
        'f3d_mask_presence_dev': (i32, [vp, vp, i32, i32, i32, vp, vp]),
        'f3d_fuse_chunked_begin_dev': (i32, [vp, vp, i64, i32, i32, i32, i32, vp, i32, vp]),
        'f3d_fuse_chunk_dev': (i32, [vp, vp, i32, i64, vp, i32, i32, i32, vp, i32, i32, i32, vp, i32, dbl, vp, C.c_uint, vp, vp]),
        'f3d_coded_plane_bytes': (C.c_size_t, [i32, i32]),
        'f3d_code_planes_dev': (i32, [vp, vp, i32, i32, i32, vp, vp]),
        'f3d_fuse_chunk_coded_dev': (i32, [vp, vp, i32, i64, vp, i32, i32, i32, vp, i32, i32, i32, vp, i32, dbl, vp, C.c_uint, vp, vp]),
        'f3d_debug_fastpath_audit': (i32, [vp, vp, i32, i64, vp, i32, i32, i32, vp]),
        'f3d_debug_fuse_deferred': (i32, [vp, vp, vp]),
        'f3d_debug_fuse_decided': (i32, [vp, vp, vp]),
        'f3d_cloud_sort_cells_dev': (i32, [vp, vp, i32, i64, vp, vp, vp]),
        'f3d_take_device_error': (i32, [vp, vp]),
        'f3d_vote_uv2pt': (i32, [vp, vp, vp, i64, vp, i64, i32]),
        'f3d_vote_uv2pt_dev': (i32, [vp, vp, vp, i64, vp, i64, i32, vp]),
        'f3d_vote_uv2pt_batch': (i32, [vp, vp, vp, i64, i32, i32, vp, i64, i32]),
        'f3d_vote_uv2pt_batch_dev': (i32, [vp, vp, vp, i64, i32, i32, vp, i64, i32, vp]),
        'f3d_segment_votes': (i32, [vp, vp, i64, i32, i32, dbl, vp, i32, vp]),
        'f3d_segment_votes_dev': (i32, [vp, vp, i64, i32, i32, dbl, vp, i32, vp, vp]),
        'f3d_segment_votes_lastcol': (i32, [vp, vp, i64, i32, i32, dbl, vp, i32, vp]),
        'f3d_segment_votes_lastcol_dev': (i32, [vp, vp, i64, i32, i32, dbl, vp, i32, vp, vp]),
        'f3d_point_vote_frames': (i32, [vp, vp, i32, i64, vp, i32, vp, i64, i64, dbl, vp, i32]),
        'f3d_point_vote_frames_dev': (i32, [vp, vp, i32, i64, vp, i32, vp, i64, i64, dbl, vp, i32, vp]),
        'f3d_ctx_reserve_point_vote': (i32, [vp, i64, i32]),
        'f3d_render_lookups': (i32, [vp, vp, i32, i64, vp, i32, i32, i32, i32, vp, vp]),
        'f3d_render_lookups_dev': (i32, [vp, vp, i32, i64, vp, i32, i32, i32, i32, vp, vp, vp]),
        'f3d_vote_visible': (i32, [vp, vp, i32, i64, vp, i32, vp, i32, i32, i32, dbl, vp, i32, i32]),
        'f3d_vote_visible_dev': (i32, [vp, vp, i32, i64, vp, i32, vp, i32, i32, i32, dbl, vp, i32, i32, vp]),
        'f3d_ctx_reserve_render': (i32, [vp, i64, i32, i32, i32]),
        'f3d_debug_render_counts': (i32, [vp, vp, i32, i64, vp, i32, i32, i32, i32, vp, vp, vp]),
        'f3d_render_mesh_lookups': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, i32, i32, dbl, vp, vp, vp]),
        'f3d_render_mesh_lookups_dev': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, i32, i32, dbl, vp, vp, vp, vp]),
        'f3d_vote_faces': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, vp, i32, i32, dbl, vp, i32, i32]),
        'f3d_vote_faces_dev': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, vp, i32, i32, dbl, vp, i32, i32, vp]),
        'f3d_vote_visible_mesh': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, i64, vp, i32, vp, i32, i32, dbl, dbl, vp, i32, i32]),
        'f3d_vote_visible_mesh_dev': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, i64, vp, i32, vp, i32, i32, dbl, dbl, vp, i32, i32, vp]),
        'f3d_ctx_reserve_mesh_render': (i32, [vp, i32, i32, i32]),
        'f3d_debug_raster_counts': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, i32, i32, dbl, i64, vp, vp, vp, vp, vp]),
        'f3d_sem_logits_to_mask': (i32, [vp, vp, i32, i64, flt, i32, vp]),
        'f3d_sem_logits_to_mask_dev': (i32, [vp, vp, i32, i64, flt, i32, vp, vp]),
        'f3d_sem_logits_to_masks_dev': (i32, [vp, vp, i32, i32, i64, flt, i32, vp, vp]),
        'f3d_points_in_obb': (i32, [vp, vp, i32, i64, vp, i32, vp, vp]),
        'f3d_points_in_obb_dev': (i32, [vp, vp, i32, i64, vp, i32, vp, vp, vp]),
        'f3d_group_by_id': (i32, [vp, vp, i64, i64, vp, vp]),
        'f3d_obb_extremes': (i32, [vp, vp, i32, i64, vp]),
        'f3d_obb_hull_filter': (i32, [vp, i64, vp, vp, vp, vp, vp]),
        'f3d_group_by_id_dev': (i32, [vp, vp, i64, i64, vp, vp, vp, vp]),
        'f3d_obb_extremes_dev': (i32, [vp, vp, i32, i64, vp, vp, i64, vp, vp]),
        'f3d_obb_hull_filter_dev': (i32, [vp, vp, i32, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]),
        'f3d_obb_fit': (i32, [vp, vp, vp, i32, vp, vp, vp, vp]),
        'f3d_obb_fit_dev': (i32, [vp, vp, vp, i32, i64, vp, vp, vp, vp, vp]),
        'f3d_obb_candidates_dev': (i32, [vp, vp, i32, i64, vp, vp, vp, i64, i32, vp, vp, vp]),
        'f3d_gather_points_dev': (i32, [vp, vp, i32, vp, i64, vp, vp]),
        'f3d_relabel': (i32, [vp, vp, i64, i64, i64, vp]),
        'f3d_relabel_dev': (i32, [vp, vp, i64, i64, i64, vp, vp]),
        'f3d_ray_x_lines': (i32, [vp, vp, vp, vp, vp, i64, vp, vp]),
        'f3d_rays_x_plane': (i32, [vp, vp, vp, vp, vp, i64, vp, vp]),
        'f3d_lines_x_planes': (i32, [vp, vp, vp, i64, vp, vp, i32, vp, vp]),
        'f3d_point_inside_polygon': (i32, [vp, vp, i64, vp, i32, vp, vp]),
        'f3d_points_plane_projection': (i32, [vp, vp, i64, vp, vp, vp]),
        'f3d_lines_plane_projection': (i32, [vp, vp, vp, i64, vp, vp, vp, vp, vp]),
        'f3d_components_same_class': (i32, [vp, vp, i64, vp, vp, vp]),
        'f3d_components_same_class_dev': (i32, [vp, vp, i64, vp, vp, vp, vp, vp]),
        'f3d_flood_order': (i32, [vp, vp, i64, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        'f3d_flood_order_dev': (i32, [vp, vp, i64, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        'f3d_color_segment': (i32, [vp, vp, i32, i64, vp, vp, vp, vp, i64, vp, vp, i32, i32, vp]),
        'f3d_color_segment_dev': (i32, [vp, vp, i32, i64, vp, vp, vp, vp, i64, vp, vp, i32, i32, vp, vp]),
        'f3d_ctx_reserve_cvseg': (i32, [vp, i64]),
        'f3d_region_grow': (i32, [vp, vp, i32, i32, i64, vp, vp, vp, i64, vp, i64, i32, vp, i32, vp, vp]),
        'f3d_region_grow_dev': (i32, [vp, vp, i32, i32, i64, vp, vp, vp, i64, vp, i64, i32, vp, i32, vp, vp, vp]),
        'f3d_plane_distance': (i32, [vp, vp, i64, vp, vp, vp]),
        'f3d_plane_distance_dev': (i32, [vp, vp, i64, vp, vp, vp, vp]),
        'f3d_ctx_reserve_refine': (i32, [vp, i64]),
        'f3d_door_window_quads': (i32, [vp, vp, i64, vp, vp, i32, vp, i64, vp, i64, vp, vp, vp, vp]),
        'f3d_door_window_quads_dev': (i32, [vp, vp, i64, vp, vp, i32, vp, i64, vp, i64, vp, vp, vp, vp, vp]),
        'f3d_ctx_reserve_quads': (i32, [vp, i64, i32, i64]),
        'f3d_mesh_vertex_map': (i32, [vp, vp, i32, i64, i64, vp, vp, vp, vp]),
        'f3d_mesh_vertex_map_dev': (i32, [vp, vp, i32, i64, i64, vp, vp, vp, vp, vp]),
        'f3d_mesh_remove_faces': (i32, [vp, vp, i32, i64, i64, vp, vp, vp, vp, vp]),
        'f3d_mesh_remove_faces_dev': (i32, [vp, vp, i32, i64, i64, vp, vp, vp, vp, vp, vp]),
        'f3d_mesh_keep_faces': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, vp, vp, vp]),
        'f3d_mesh_keep_faces_dev': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, vp, vp, vp, vp]),
        'f3d_mesh_triangle_clusters': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, vp, vp, vp, vp]),
        'f3d_mesh_triangle_clusters_dev': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, vp, vp, vp, vp, vp]),
        'f3d_mesh_clean': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i64, dbl, vp, vp, vp, vp, vp]),
        'f3d_mesh_clean_dev': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i64, dbl, vp, vp, vp, vp, vp, vp]),
        'f3d_mesh_face_frames': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, vp, vp, vp]),
        'f3d_mesh_face_frames_dev': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, vp, vp, vp, vp]),
        'f3d_mesh_face_graph': (i32, [vp, vp, i32, i64, vp, i32, i64, i32, dbl, vp, vp, i64, vp]),
        'f3d_mesh_face_graph_dev': (i32, [vp, vp, i32, i64, vp, i32, i64, i32, dbl, vp, vp, i64, vp, vp]),
        'f3d_ctx_reserve_mesh': (i32, [vp, i64, i64]),
        'f3d_extract_planes': (i32, [vp, vp, i32, i64, vp, vp, vp, dbl, dbl, dbl, dbl, i64, i64, i64, vp, vp, vp, vp, vp]),
        'f3d_extract_planes_dev': (i32, [vp, vp, i32, i64, vp, vp, vp, dbl, dbl, dbl, dbl, i64, i64, i64, vp, vp, vp, vp, vp, vp]),
        'f3d_ctx_reserve_planes': (i32, [vp, i64]),
        'f3d_smooth_votes': (i32, [vp, vp, i32, i64, i32, vp, vp, vp, dbl, vp, i32, dbl, dbl, i32, vp]),
        'f3d_smooth_votes_dev': (i32, [vp, vp, i32, i64, i32, vp, vp, vp, dbl, vp, i32, dbl, dbl, i32, vp, vp]),
        'f3d_smooth_segment': (i32, [vp, vp, i32, i64, i32, vp, vp, vp, dbl, vp, i32, dbl, dbl, i32, i32, dbl, vp, i32, i32, vp]),
        'f3d_smooth_segment_dev': (i32, [vp, vp, i32, i64, i32, vp, vp, vp, dbl, vp, i32, dbl, dbl, i32, i32, dbl, vp, i32, i32, vp, vp]),
        'f3d_ctx_reserve_smooth': (i32, [vp, i64, i32, i32]),
        'f3d_lift_overlaps': (i32, [vp, vp, vp, i32, i64, i64, i32, vp, vp, vp, i64, vp]),
        'f3d_lift_overlaps_dev': (i32, [vp, vp, vp, i32, i64, i64, i32, vp, vp, vp, i64, vp, vp]),
        'f3d_lift_instances': (i32, [vp, vp, vp, i32, i64, i64, i32, dbl, i64, vp, i64, vp, vp, vp, vp, vp, vp]),
        'f3d_lift_instances_dev': (i32, [vp, vp, vp, i32, i64, i64, i32, dbl, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        'f3d_ctx_reserve_lift': (i32, [vp, i32, i64, i64, i32, i64]),
        'f3d_patch_owner': (i32, [vp, vp, i64, i32, i32, i32, dbl, dbl, vp, vp, vp, vp, vp, vp]),
        'f3d_patch_owner_dev': (i32, [vp, vp, i64, i32, i32, i32, dbl, dbl, vp, vp, vp, vp, vp, vp, vp]),
        'f3d_patch_match': (i32, [vp, vp, i64, i32, i32, i32, dbl, dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        'f3d_patch_seeds_sums': (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, dbl, dbl, vp, vp, vp, vp]),
        'f3d_patch_match_dev': (i32, [vp, vp, i64, i32, i32, i32, dbl, dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        'f3d_patch_seeds_sums_dev': (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, dbl, dbl, vp, vp, vp, vp, vp]),
        'f3d_fusion_hits_dev': (i32, [vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]),
        'f3d_fusion_seed_update_dev': (i32, [vp, vp, i64, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        'f3d_fusion_lookup_dev': (i32, [vp, vp, vp, i64, vp, vp, vp]),
        'f3d_fusion_frame_check_dev': (i32, [vp, vp, vp, vp, i64, dbl, dbl, vp, vp]),
        'f3d_fusion_prio_dev': (i32, [vp, vp, i64, vp, vp]),
        'f3d_fusion_new_seeds_dev': (i32, [vp, vp, vp, vp, vp, i64, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
        'f3d_unproject_depth': (i32, [vp, vp, i32, i32, i32, vp, dbl, vp, vp, vp]),
        'f3d_unproject_depth_dev': (i32, [vp, vp, i32, i32, i32, vp, dbl, vp, vp, vp, vp]),
        'f3d_unproject_depth_batch_dev': (i32, [vp, vp, i32, i32, i32, i32, vp, dbl, vp, vp, vp, vp]),
        'f3d_radius_graph_count': (i32, [vp, vp, i32, i64, dbl, vp, vp]),
        'f3d_radius_graph_fill': (i32, [vp, i64, vp]),
        'f3d_radius_graph_count_dev': (i32, [vp, vp, i32, i64, dbl, vp, vp, vp]),
        'f3d_radius_graph_fill_dev': (i32, [vp, i64, vp, vp, vp]),
        'f3d_radius_query_count': (i32, [vp, vp, i32, i64, vp, i32, i64, dbl, vp, vp]),
        'f3d_radius_query_fill': (i32, [vp, i64, vp]),
        'f3d_radius_query_count_dev': (i32, [vp, vp, i32, i64, vp, i32, i64, dbl, vp, vp, vp]),
        'f3d_radius_query_fill_dev': (i32, [vp, vp, i32, i64, vp, vp, vp]),
        'f3d_knn_query': (i32, [vp, vp, i32, i64, vp, i32, i64, i32, dbl, vp, vp, vp]),
        'f3d_knn_query_dev': (i32, [vp, vp, i32, i64, vp, i32, i64, i32, dbl, vp, vp, vp, vp]),
        'f3d_transfer_labels': (i32, [vp, vp, i32, i64, vp, vp, i32, i64, i32, dbl, i64, vp, vp]),
        'f3d_transfer_labels_dev': (i32, [vp, vp, i32, i64, vp, vp, i32, i64, i32, dbl, i64, vp, vp, vp]),
        'f3d_ctx_reserve_knn': (i32, [vp, i64]),
        'f3d_estimate_normals': (i32, [vp, vp, i64, vp, dbl, i32, i32, vp, vp, vp]),
        'f3d_estimate_normals_batch_dev': (i32, [vp, vp, i32, i64, vp, dbl, i32, i32, vp, vp, vp, vp]),
        'f3d_tsdf_integrate': (i32, [vp, vp, vp, i32, i32, i32, vp, dbl, dbl, flt, vp, i32, i32, i32, i32, dbl, dbl, vp]),
        'f3d_tsdf_integrate_dev': (i32, [vp, vp, vp, i32, i32, i32, vp, dbl, dbl, flt, vp, i32, i32, i32, i32, dbl, dbl, vp, vp]),
        'f3d_tsdf_extract_count': (i32, [vp, vp, vp, i32, i32, i32, flt, vp, vp]),
        'f3d_tsdf_extract_fill': (i32, [vp, i32, i32, i32, vp, dbl, vp, vp]),
        'f3d_tsdf_extract_count_dev': (i32, [vp, vp, vp, i32, i32, i32, flt, vp, vp, vp]),
        'f3d_tsdf_extract_fill_dev': (i32, [vp, vp, i32, i32, i32, vp, dbl, vp, vp, vp]),
        'f3d_tsdf_integrate_color': (i32, [vp, vp, vp, vp, i32, i32, i32, vp, dbl, dbl, flt, vp, i32, vp, i32, i32, i32, i32, i32, dbl, dbl, vp]),
        'f3d_tsdf_integrate_color_dev': (i32, [vp, vp, vp, vp, i32, i32, i32, vp, dbl, dbl, flt, vp, i32, vp, i32, i32, i32, i32, i32, dbl, dbl, vp, vp]),
        'f3d_tsdf_extract_colors': (i32, [vp, vp, i32, i32, i32, vp, vp]),
        'f3d_tsdf_extract_colors_dev': (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        'f3d_ctx_reserve_tsdf': (i32, [vp, i64]),
        'f3d_debug_tsdf_grid_cap': (i32, [vp, i32]),
        'f3d_debug_grid_cap': (i32, [vp, i32]),
        'f3d_debug_grid_cap_stats': (i32, [vp, vp]),
        'f3d_debug_poison': (i32, [vp, i32, vp]),
        'f3d_fuse_features': (i32, [vp, vp, i32, i64, vp, i32, i32, i32, vp, i32, i32, i32, i32, i32, dbl, vp, vp, i32]),
        'f3d_fuse_features_dev': (i32, [vp, vp, i32, i64, vp, i32, i32, i32, vp, i32, i32, i32, i32, i32, dbl, vp, vp, i32, vp]),
        'f3d_features_finalize': (i32, [vp, vp, vp, i64, i32, i32, vp]),
        'f3d_features_finalize_dev': (i32, [vp, vp, vp, i64, i32, i32, vp, vp]),
        'f3d_tsdf_raycast': (i32, [vp, vp, vp, i32, i32, i32, vp, dbl, flt, vp, vp, vp, i32, i32, dbl, dbl, i32, vp, vp, vp]),
        'f3d_tsdf_raycast_dev': (i32, [vp, vp, vp, i32, i32, i32, vp, dbl, flt, vp, vp, vp, i32, i32, dbl, dbl, i32, vp, vp, vp, vp]),
        'f3d_icp_sums': (i32, [vp, vp, i32, i32, i32, vp, dbl, dbl, vp, vp, vp, vp, i32, i32, vp, dbl, vp]),
        'f3d_icp_sums_dev': (i32, [vp, vp, i32, i32, i32, vp, dbl, dbl, vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp]),
        'f3d_icp': (i32, [vp, vp, i32, i32, i32, vp, dbl, dbl, vp, vp, vp, vp, i32, i32, vp, dbl, i32, i32, vp, vp, vp]),
        'f3d_icp_dev': (i32, [vp, vp, i32, i32, i32, vp, dbl, dbl, vp, vp, vp, vp, i32, i32, vp, dbl, i32, i32, vp, vp, vp, vp]),
        'f3d_ctx_reserve_icp': (i32, [vp, i64]),
        'f3d_tsdf_raycast_color': (i32, [vp, vp, vp, vp, i32, i32, i32, vp, dbl, flt, vp, vp, vp, i32, i32, dbl, dbl, i32, vp, vp, vp, vp, vp]),
        'f3d_tsdf_raycast_color_dev': (i32, [vp, vp, vp, vp, i32, i32, i32, vp, dbl, flt, vp, vp, vp, i32, i32, dbl, dbl, i32, vp, vp, vp, vp, vp, vp]),
        'f3d_icp_color_sums': (i32, [vp, vp, i32, i32, i32, vp, dbl, dbl, vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp, i32, i32, dbl, vp]),
        'f3d_icp_color_sums_dev': (i32, [vp, vp, i32, i32, i32, vp, dbl, dbl, vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp, i32, i32, dbl, vp, vp]),
        'f3d_icp_color': (i32, [vp, vp, i32, i32, i32, vp, dbl, dbl, vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp, i32, i32, dbl, i32, i32, vp, vp, vp]),
        'f3d_icp_color_dev': (i32, [vp, vp, i32, i32, i32, vp, dbl, dbl, vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp, i32, i32, dbl, i32, i32, vp, vp, vp,
                                    vp]),
        'f3d_ctx_reserve_icp_color': (i32, [vp, i64]),
        'f3d_depth_half': (i32, [vp, vp, i32, i32, i32, dbl, dbl, dbl, vp]),
        'f3d_depth_half_dev': (i32, [vp, vp, i32, i32, i32, dbl, dbl, dbl, vp, vp]),
        'f3d_maps_half': (i32, [vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp, vp]),
        'f3d_maps_half_dev': (i32, [vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp, vp, vp]),
        'f3d_icp_levels': (i32, [vp, vp, i32, dbl, vp, vp, vp, i32, i32, dbl, vp, vp, vp]),
        'f3d_icp_levels_dev': (i32, [vp, vp, i32, dbl, vp, vp, vp, i32, i32, dbl, vp, vp, vp, vp]),
        'f3d_cloud_icp_sums': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, vp, vp, dbl, vp, vp]),
        'f3d_cloud_icp_sums_dev': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, vp, vp, dbl, vp, vp, vp]),
        'f3d_cloud_icp': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, vp, vp, dbl, i32, i32, vp, vp, vp]),
        'f3d_cloud_icp_dev': (i32, [vp, vp, i32, i64, vp, i32, i64, vp, i32, vp, vp, dbl, i32, i32, vp, vp, vp, vp]),
        'f3d_ctx_reserve_cloud_icp': (i32, [vp, i64, i64]),
    }
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = res, args
    lib._f3d_symbols = tuple(protos)
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f'expected shape {tuple(shape)}, got {a.shape}')
    return a


def _n3(a, message='expected [N,3], got {}'):
    a = _f64(a)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(message.format(a.shape))
    return a


def _raise(code, msg):
    if code == ERR_INDEX:
        raise IndexError(msg)
    if code == ERR_ZERO_QUAT:
        raise ZeroDivisionError(msg)
    if code == ERR_INVALID:
        raise ValueError(msg)
    if code == ERR_NOMEM:
        raise MemoryError(msg)
    if code == ERR_HIP:
        raise F3DUnavailable(msg)
    raise F3DError(f'f3d error {code}: {msg}')


# ------------------------------------------------------------------ host geometry (no device)
def quat_inverse(q_wxyz):
    q = _f64(q_wxyz, (4,))
    out = np.empty(4)
    rc = library().f3d_quat_inverse(_ptr(q), _ptr(out))
    if rc:
        _raise(rc, 'a zero quaternion cannot be inverted')
    return out


def frustum_data(K, w, h, wxyzs, translations):
    """eyes [V,3], lookats [V,3], face_normals [V,4,3] of Fusion._get_frustum_data (fusion.py:119-132)."""
    K = _f64(K, (3, 3))
    q = _f64(np.atleast_2d(wxyzs))
    t = _f64(np.atleast_2d(translations))
    V = len(t)
    if q.shape != (V, 4) or t.shape != (V, 3):
        raise ValueError('wxyzs must be [V,4] and translations [V,3]')
    eyes, look, nrm = np.empty((V, 3)), np.empty((V, 3)), np.empty((V, 4, 3))
    rc = library().f3d_frustum_data(_ptr(K), float(w), float(h), _ptr(q), _ptr(t), V, _ptr(eyes), _ptr(look), _ptr(nrm))
    if rc:
        _raise(rc, 'f3d_frustum_data failed')
    return eyes, look, nrm


def views_build(K, w, h, wxyzs, translations, max_depth):
    """Packed per-view records (704 bytes each, viewed as float64 [V, 88]) consumed by the fused kernels."""
    K = _f64(K, (3, 3))
    q = _f64(np.atleast_2d(wxyzs))
    t = _f64(np.atleast_2d(translations))
    V = len(t)
    if q.shape != (V, 4) or t.shape != (V, 3):
        raise ValueError('wxyzs must be [V,4] and translations [V,3]')
    out = np.zeros((V, VIEW_DOUBLES))
    rc = library().f3d_views_build(_ptr(K), float(w), float(h), _ptr(q), _ptr(t), V, float(max_depth), _ptr(out))
    if rc:
        _raise(rc, 'a zero quaternion cannot be inverted' if rc == ERR_ZERO_QUAT else 'f3d_views_build failed')
    return out


def view_fields(views):
    """Named sub-arrays of a [V,88] view table (for tests and debugging)."""
    v = np.asarray(views)
    return {'M': v[:, 0:9].reshape(-1, 3, 3), 't': v[:, 9:12], 'mnorm': v[:, 12:15],
            'K': v[:, 40:49].reshape(-1, 3, 3), 'qinv': v[:, 49:53],
            'plane_pt': v[:, 53:68].reshape(-1, 5, 3), 'plane_n': v[:, 68:83].reshape(-1, 5, 3), 'plane_off': v[:, 83:88]}


def _views(views):
    views = _f64(views)
    if views.ndim != 2 or views.shape[1] != VIEW_DOUBLES:
        raise ValueError(f'views must be [V,{VIEW_DOUBLES}]')
    return views


def features_check(sums, counts, feats=None, nviews=None, npoints=None):
    """The array checks of fuse_features / features_finalize (f3d.h "feature fusion"), for NumPy arrays and torch tensors alike, with
    no device call: sums C-contiguous float32 [N, d], 1 <= d <= 4096; counts C-contiguous int32 [N]; feats C-contiguous float16 /
    float32 [V, hf, wf, d] with one map per view.  TypeError for a wrong dtype, ValueError for a wrong shape.  -> FEAT_F16 / FEAT_F32
    (None without feats)."""
    name = lambda a: str(a.dtype).replace('torch.', '')                      # noqa: E731
    contiguous = lambda a: a.is_contiguous() if hasattr(a, 'is_contiguous') else a.flags.c_contiguous   # noqa: E731
    for a, what in ((sums, 'sums'), (counts, 'counts'), (feats, 'feats')):
        if a is not None and not (hasattr(a, 'dtype') and hasattr(a, 'shape')):
            raise TypeError(f'{what} must be an array or a tensor, got {type(a).__name__}')
    if name(sums) != 'float32':
        raise TypeError(f'sums must be float32, got {sums.dtype}')
    if name(counts) != 'int32':
        raise TypeError(f'counts must be int32, got {counts.dtype}')
    if len(sums.shape) != 2 or not contiguous(sums):
        raise ValueError('sums must be a C-contiguous float32 [N, d] array')
    n, d = (int(x) for x in sums.shape)
    if not 1 <= d <= FEAT_MAX_D:
        raise ValueError(f'd must be in [1, {FEAT_MAX_D}], got {d}')
    if tuple(counts.shape) != (n,) or not contiguous(counts):
        raise ValueError(f'counts must be a C-contiguous int32 [{n}] array, got {tuple(counts.shape)}')
    if npoints is not None and n != int(npoints):
        raise ValueError(f'sums has {n} rows, the cloud {int(npoints)} points')
    if feats is None:
        return None
    if name(feats) not in ('float16', 'float32'):
        raise TypeError(f'feats must be float16 or float32, got {feats.dtype}')
    if len(feats.shape) != 4 or not contiguous(feats):
        raise ValueError('feats must be a C-contiguous [V, hf, wf, d] array (channel-last)')
    if int(feats.shape[3]) != d:
        raise ValueError(f'feats has {int(feats.shape[3])} channels, sums {d}')
    if int(feats.shape[1]) < 1 or int(feats.shape[2]) < 1:
        raise ValueError(f'feature maps must have at least one pixel, got {tuple(feats.shape[1:3])}')
    if nviews is not None and int(feats.shape[0]) != int(nviews):
        raise ValueError(f'{int(nviews)} views for {int(feats.shape[0])} feature maps')
    return FEAT_F16 if name(feats) == 'float16' else FEAT_F32


def _mesh(vertices, triangles):
    """(vertices float64 / float32 [V,3], F64 / F32, triangles int64 / int32 [M,3], I64 / I32), C-contiguous."""
    vx, vdt = _xyz(vertices)
    tr = np.asarray(triangles)
    if tr.dtype not in (np.int32, np.int64):
        raise TypeError(f'triangles must be int32 or int64, got {tr.dtype}')
    if tr.ndim != 2 or tr.shape[1] != 3:
        raise ValueError(f'triangles must be [M,3], got {tr.shape}')
    return vx, vdt, np.ascontiguousarray(tr), I32 if tr.dtype == np.int32 else I64


def _xyz(points):
    p = np.asarray(points)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f'points must be [N,3], got {p.shape}')
    if p.dtype == np.float32:
        return np.ascontiguousarray(p), F32
    return np.ascontiguousarray(p, dtype=np.float64), F64


def _tsdf_state(tsdf, weight):
    """(nz, ny, nx) of the two state arrays of a TSDF volume: C-contiguous float32 [nz, ny, nx] NumPy arrays, written in place."""
    for a in (tsdf, weight):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 3 or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError('tsdf and weight must be writeable C-contiguous float32 [nz, ny, nx] arrays')
    if tsdf.shape != weight.shape:
        raise ValueError(f'tsdf {tsdf.shape} and weight {weight.shape} differ in shape')
    return tsdf.shape


def _tsdf_frames(lo, depths, views):
    """(lo float64 [3], depths [F, h, w] contiguous, its depth code, views [F, 88]) of a tsdf_integrate call."""
    d = np.ascontiguousarray(depths)
    if d.ndim != 3:
        raise ValueError(f'depths must be [F, h, w], got {d.shape}')
    views = _views(views)
    if len(views) != len(d):
        raise ValueError(f'{len(views)} views for {len(d)} depth frames')
    return _f64(lo, (3,)), d, depth_code(d), views


def _tsdf_color(color, shape, writeable=True):
    """The colour state of a TSDF volume whose tsdf has `shape`: a C-contiguous float32 [nz, ny, nx, 4] NumPy array."""
    if not isinstance(color, np.ndarray) or color.dtype != np.float32:
        raise TypeError('color must be a float32 NumPy array')
    if color.shape != tuple(shape) + (4,) or not color.flags.c_contiguous or (writeable and not color.flags.writeable):
        raise ValueError(f'color must be a writeable C-contiguous float32 {tuple(shape) + (4,)} array, got {color.shape}')
    return color


def _tsdf_rgb(rgb, nframes):
    """The colour images of a tsdf_integrate_color call: uint8 [F, hc, wc, 3], C-contiguous, one per depth frame."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8:
        raise TypeError(f'colour images must be uint8, got {rgb.dtype}')
    if rgb.ndim != 4 or rgb.shape[3] != 3 or rgb.shape[1] < 1 or rgb.shape[2] < 1:
        raise ValueError(f'colour images must be [F, hc, wc, 3] with pixels, got {rgb.shape}')
    if rgb.shape[0] != nframes:
        raise ValueError(f'{rgb.shape[0]} colour images for {nframes} depth frames')
    return np.ascontiguousarray(rgb)


def _icp_arrays(depth, K, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view):
    """The host arrays of icp_sums / icp as the C entry reads them: (depth [h, w], its depth code, K, q, t, the two model maps [hm*wm, 3],
    the model view [88])."""
    d = np.ascontiguousarray(depth)
    if d.ndim != 2 or d.size == 0:
        raise ValueError(f'depth must be one [h, w] frame with pixels, got {d.shape}')
    hm, wm = int(hm), int(wm)
    if hm < 1 or wm < 1:
        raise ValueError('the model image must have pixels')
    mv, mn = _f64(model_vertex), _f64(model_normal)
    if mv.size != hm * wm * 3 or mn.size != hm * wm * 3:
        raise ValueError(f'the model maps must be [{hm} * {wm}, 3], got {mv.shape} and {mn.shape}')
    return d, depth_code(d), _f64(K, (3, 3)), _f64(q_wxyz, (4,)), _f64(t, (3,)), mv, mn, _f64(np.asarray(model_view).reshape(-1), (VIEW_DOUBLES,))


def icp_color_check(model_intensity, rgb, color_weight, hm, wm):
    """The checks of the colour arguments of icp_color_sums / icp_color (f3d.h "colour in registration"), for NumPy arrays and torch
    tensors alike, with no device call: model_intensity float64 with hm * wm values, rgb one uint8 [hc, wc, 3] image with pixels,
    color_weight finite and >= 0.  TypeError for a wrong dtype, ValueError otherwise.  -> (hc, wc, color_weight)."""
    name = lambda a: str(a.dtype).replace('torch.', '')                      # noqa: E731
    if name(model_intensity) != 'float64':
        raise TypeError(f'model_intensity must be float64, got {name(model_intensity)}')
    if name(rgb) != 'uint8':
        raise TypeError(f'the colour image must be uint8, got {name(rgb)}')
    size = 1
    for x in model_intensity.shape:
        size *= int(x)
    if size != int(hm) * int(wm):
        raise ValueError(f'model_intensity must hold {hm} * {wm} values, got {tuple(model_intensity.shape)}')
    shape = tuple(int(x) for x in rgb.shape)
    if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1 or shape[0] * shape[1] >= 1 << 31:
        raise ValueError(f'the colour image must be [hc, wc, 3] with pixels, fewer than 2^31, got {shape}')
    color_weight = float(color_weight)
    if not (color_weight >= 0.0 and color_weight < float('inf')):
        raise ValueError(f'color_weight must be finite and not negative, got {color_weight}')
    return shape[0], shape[1], color_weight


def _icp_color_arrays(model_intensity, rgb, color_weight, hm, wm):
    """The host arrays of the colour arguments as the C entry reads them -> (model_intensity [hm*wm], rgb [hc, wc, 3], color_weight)."""
    mi, rgb = np.asarray(model_intensity), np.asarray(rgb)
    _, _, color_weight = icp_color_check(mi, rgb, color_weight, hm, wm)
    return np.ascontiguousarray(mi).reshape(-1), np.ascontiguousarray(rgb), color_weight


def _half_check(what, shape, gate):
    """The checks depth_half / maps_half make before any device call: a 2D image of at least 2 x 2 pixels and a finite positive
    gate -> gate as a float."""
    shape = tuple(int(x) for x in shape)
    if len(shape) != 2 or shape[0] < 2 or shape[1] < 2:
        raise ValueError(f'{what} must be [h, w] with at least 2 rows and 2 columns, got {shape}')
    gate = float(gate)
    if not (gate > 0.0 and gate < float('inf')):
        raise ValueError(f'gate must be finite and positive, got {gate}')
    return gate


def _half_intensity(model_intensity, hm, wm):
    mi = np.asarray(model_intensity)
    if mi.dtype != np.float64:
        raise TypeError(f'model_intensity must be float64, got {mi.dtype}')
    if mi.size != hm * wm:
        raise ValueError(f'model_intensity must hold {hm} * {wm} values, got {mi.shape}')
    return np.ascontiguousarray(mi).reshape(-1)


ICP_LEVEL_KEYS = ('depth', 'K', 'model_vertex', 'model_normal', 'hm', 'wm', 'model_view', 'max_dist', 'iterations', 'min_pairs')


def _icp_levels_check(levels, rgb, color_weight):
    """The checks of an icp_levels call that need no array: 1 .. ICP_MAX_LEVELS levels with every key, iterations >= 1 and
    min_pairs >= 6 on each, and colour on every level with rgb and color_weight, or on none without -> the levels as a list."""
    levels = list(levels)
    if not 1 <= len(levels) <= ICP_MAX_LEVELS:
        raise ValueError(f'icp_levels takes 1 to {ICP_MAX_LEVELS} levels, got {len(levels)}')
    if (rgb is None) != (color_weight is None):
        raise ValueError('rgb and color_weight go together: pass both or none')
    for lv in levels:
        missing = [k for k in ICP_LEVEL_KEYS if k not in lv]
        if missing:
            raise ValueError(f'a level lacks {missing}')
        if int(lv['iterations']) < 1 or int(lv['min_pairs']) < 6:
            raise ValueError(f'a level needs iterations >= 1 and min_pairs >= 6, got {lv["iterations"]} and {lv["min_pairs"]}')
        if (lv.get('model_intensity') is None) != (rgb is None):
            raise ValueError('either every level has a model_intensity and rgb is given, or none has and rgb is None')
    return levels


def _fill_level(rec, depth_ptr, depth_type, h, w, K, depth_scale, vertex_ptr, normal_ptr, intensity_ptr, hm, wm, view_ptr, max_dist, iterations,
                min_pairs):
    """One IcpLevel record from raw pointers (host or device) and the level's numbers."""
    rec.depth, rec.depth_type, rec.h, rec.w = depth_ptr, int(depth_type), int(h), int(w)
    rec.K[:] = [float(x) for x in np.asarray(K, np.float64).reshape(9)]
    rec.depth_scale = float(depth_scale)
    rec.model_vertex, rec.model_normal, rec.model_intensity = vertex_ptr, normal_ptr, intensity_ptr
    rec.hm, rec.wm, rec.model_view = int(hm), int(wm), view_ptr
    rec.max_dist, rec.iterations, rec.min_pairs = float(max_dist), int(iterations), int(min_pairs)


def _quat_matrix(q_wxyz):
    """The rotation matrix float64 [3, 3] of a (not necessarily unit) quaternion; ValueError for a zero or non-finite one.  Host
    bookkeeping of the cloud ICP callers (the centre folded into and out of t), no part of the contract's arithmetic."""
    q = np.asarray(q_wxyz, np.float64).reshape(4)
    norm = np.sqrt((q * q).sum())
    if not (0.0 < norm < np.inf):
        raise ValueError('the quaternion must be finite and not zero')
    w, x, y, z = q / norm
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _cloud_icp_check(mode, has_normals, q_wxyz, t, max_dist, iterations=None, min_pairs=None):
    """The numbers of a cloud_icp_sums / cloud_icp call as the C entry reads them -> (mode, q float64 [4], t float64 [3], max_dist), or
    ValueError for what f3d.h refuses: an unknown mode, plane mode without normals, a max_dist that is not finite, positive and below
    1e300, a zero or non-finite quaternion, a non-finite t, iterations < 1, min_pairs < 6."""
    if mode not in (CLOUD_ICP_PLANE, CLOUD_ICP_POINT):
        raise ValueError(f'mode must be CLOUD_ICP_PLANE or CLOUD_ICP_POINT, got {mode!r}')
    if mode == CLOUD_ICP_PLANE and not has_normals:
        raise ValueError('CLOUD_ICP_PLANE needs the normals of the target')
    q, t, max_dist = _f64(q_wxyz, (4,)), _f64(t, (3,)), float(max_dist)
    if not (0.0 < max_dist < 1e300):
        raise ValueError(f'max_dist must be finite, positive and below 1e300, got {max_dist}')
    if not (np.isfinite(q).all() and np.isfinite(t).all() and 0.0 < float(np.sqrt((q * q).sum())) < np.inf):
        raise ValueError('the pose must be a finite non-zero quaternion and a finite translation')
    if iterations is not None and int(iterations) < 1:
        raise ValueError(f'iterations must be at least 1, got {iterations}')
    if min_pairs is not None and int(min_pairs) < 6:
        raise ValueError(f'min_pairs must be at least 6, got {min_pairs}')
    return int(mode), q, t, max_dist


def _cloud_icp_arrays(source, target, target_normals, mode):
    """The host arrays of cloud_icp_sums / cloud_icp: (source [n, 3], its dtype code, target [m, 3], its dtype code, the normals float64
    [m, 3] or None in point mode)."""
    s, sdt = _xyz(source)
    g, gdt = _xyz(target)
    if len(g) == 0:
        raise ValueError('the target is empty')
    nrm = None
    if mode == CLOUD_ICP_PLANE:
        nrm = _f64(target_normals)
        if nrm.shape != g.shape:
            raise ValueError(f'the normals must be {g.shape} like the target, got {nrm.shape}')
    return s, sdt, g, gdt, nrm


def _knn_k(k):
    """k of knn_query / transfer_labels, checked before anything is launched."""
    k = int(k)
    if k < 1 or k > KNN_MAX_K:
        raise ValueError(f'k must be in [1, {KNN_MAX_K}], got {k}')
    return k


def _filter(filter_classes):
    if filter_classes is None:
        return None, 0
    f = np.ascontiguousarray(np.asarray(list(filter_classes)), dtype=np.int32)
    return f, len(f)


def _vtype(votes):
    """VOTES_F64 / VOTES_U16 of a float64 / uint16 vote matrix (array or tensor)."""
    return VOTES_U16 if votes.dtype.itemsize == 2 else VOTES_F64


def _smooth_arrays(votes, offsets, neighbours, normals, colors):
    """The host arrays of smooth_votes / smooth_segment as the C entry reads them: (offsets, neighbours, normals, colors)."""
    if not isinstance(votes, np.ndarray) or votes.ndim != 2 or votes.dtype not in (np.float64, np.uint16) or not votes.flags.c_contiguous:
        raise ValueError('votes must be a C-contiguous float64 or uint16 [n, ncols] array')
    n = len(votes)
    offsets, neighbours = host_csr(offsets, neighbours, n)
    if normals is not None:
        normals = _f64(normals, (n, 3))
    if colors is not None:
        colors = np.ascontiguousarray(colors, dtype=np.float32 if np.asarray(colors).dtype == np.float32 else np.float64)
        if colors.shape != (n, 3):
            raise ValueError(f'expected shape {(n, 3)}, got {colors.shape}')
    return offsets, neighbours, normals, colors


def _flood_stats(stats):
    return {'clusters': int(stats[0]), 'points': int(stats[1]), 'levels': int(stats[2]), 'readbacks': int(stats[3])}


def _threshold3(threshold):
    """color_segment's threshold as float64 [3]: a scalar is repeated (cv.py:387); comparisons with it happen in float64."""
    t = np.asarray(threshold, dtype=np.float64)
    return np.ascontiguousarray(np.broadcast_to(t, (3,)) if t.ndim == 0 else t.reshape(3))


def _grow_params(nchan, sma0, threshold):
    """region_grow's running mean at the start and its threshold as float64 [nchan] (a scalar threshold is repeated)."""
    sma = np.ascontiguousarray(np.asarray(sma0, dtype=np.float64).reshape(-1))
    thr = np.asarray(threshold, dtype=np.float64)
    thr = np.ascontiguousarray(np.broadcast_to(thr, (nchan,)) if thr.ndim == 0 else thr.reshape(-1))
    if len(sma) != nchan or len(thr) != nchan:
        raise ValueError(f'region_grow: sma0 and threshold must have {nchan} entries')
    return sma, thr


class Context:
    """One f3d_ctx (device ordinal, stream, scratch arena).  Not thread-safe."""

    def __init__(self, device=0):
        self._lib = library()
        self._h = self._lib.f3d_ctx_create(int(device))
        if not self._h:
            raise F3DUnavailable(self._lib.f3d_last_error(None).decode() or 'f3d_ctx_create failed')
        self.device = int(device)

    def close(self):
        if getattr(self, '_h', None):
            self._lib.f3d_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            _raise(rc, self._lib.f3d_last_error(self._h).decode())

    @property
    def stream(self):
        return self._lib.f3d_ctx_stream(self._h)

    def synchronize(self):
        self._check(self._lib.f3d_ctx_synchronize(self._h))

    def reserve(self, n=0, nviews=0, h=0, w=0):
        """Size the scratch of the fused path / cell sort / uv2pt vote beforehand: later _dev calls do not allocate."""
        self._check(self._lib.f3d_ctx_reserve(self._h, int(n), int(nviews), int(h), int(w)))

    def reserve_cvseg(self, n):
        """Size the scratch of flood_order / color_segment for clouds of up to n points (strict contexts then do not allocate)."""
        self._check(self._lib.f3d_ctx_reserve_cvseg(self._h, int(n)))

    def reserve_quads(self, n, k, ntriangles):
        """Size the scratch of door_window_quads for n points, k instances and that many triangles."""
        self._check(self._lib.f3d_ctx_reserve_quads(self._h, int(n), int(k), int(ntriangles)))

    def reserve_mesh(self, nvertices, ntriangles):
        """Size the scratch of the mesh_*_dev calls for meshes of up to that many vertices and triangles."""
        self._check(self._lib.f3d_ctx_reserve_mesh(self._h, int(nvertices), int(ntriangles)))

    def reserve_planes(self, n):
        """Size the scratch of extract_planes_dev for clouds of up to n points, for any max_planes."""
        self._check(self._lib.f3d_ctx_reserve_planes(self._h, int(n)))

    def reserve_smooth(self, n, ncols, iterations):
        """Size the scratch of smooth_votes_dev / smooth_segment_dev for [n, ncols] vote matrices and that many iterations (one
        iteration needs none)."""
        self._check(self._lib.f3d_ctx_reserve_smooth(self._h, int(n), int(ncols), int(iterations)))

    def reserve_lift(self, nframes, hw, npoints, max_ids, max_pairs=0):
        """Size the scratch of lift_overlaps_dev / lift_instances_dev for nframes frames of hw pixels, npoints points, max_ids ids per
        frame and a pair table (and pair output) of up to max_pairs distinct overlapping segment pairs."""
        self._check(self._lib.f3d_ctx_reserve_lift(self._h, int(nframes), int(hw), int(npoints), int(max_ids), int(max_pairs)))

    def reserve_refine(self, n):
        """Size the scratch of region_grow_dev for clouds of up to n points."""
        self._check(self._lib.f3d_ctx_reserve_refine(self._h, int(n)))

    def reserve_point_vote(self, m, ncols):
        """Size the scratch of point_vote_frames_dev for clouds of up to m points and ncols vote columns, at any radius."""
        self._check(self._lib.f3d_ctx_reserve_point_vote(self._h, int(m), int(ncols)))

    def reserve_knn(self, m):
        """Size the scratch of knn_query_dev / transfer_labels_dev for data clouds of up to m points, at any radius."""
        self._check(self._lib.f3d_ctx_reserve_knn(self._h, int(m)))

    def reserve_render(self, n, nviews, h, w):
        """Size the depth keys of render_lookups_dev / vote_visible_dev / fuse_features_dev (automatic pass size) for nviews views of
        h x w pixels."""
        self._check(self._lib.f3d_ctx_reserve_render(self._h, int(n), int(nviews), int(h), int(w)))

    def set_strict(self, strict=True):
        self._check(self._lib.f3d_ctx_set_strict(self._h, int(bool(strict))))

    @property
    def alloc_count(self):
        return int(self._lib.f3d_ctx_alloc_count(self._h))

    # ---------------------------------------------------------------- NumPy (host pointer) calls
    def rotate(self, points, q_wxyz):
        p = _n3(points, 'points must be [N,3]')
        q = _f64(q_wxyz, (4,))
        out = np.empty_like(p)
        self._check(self._lib.f3d_rotate_f64(self._h, _ptr(p), len(p), _ptr(q), _ptr(out)))
        return out

    def points2pixel(self, points, intrinsic, quat, translation):
        p = _n3(points, 'points must be [N,3]')
        K, q, t = _f64(intrinsic, (3, 3)), _f64(quat, (4,)), _f64(translation, (3,))
        uv = np.empty((2, len(p)), np.int32)
        self._check(self._lib.f3d_points2pixel_f64(self._h, _ptr(p), len(p), _ptr(K), _ptr(q), _ptr(t), _ptr(uv)))
        return uv

    def inside_polyhedra(self, points, plane_points, normals):
        p = _n3(points, 'points must be [N,3]')
        pp, nr = _f64(plane_points), _f64(normals)
        if pp.shape != nr.shape or pp.ndim != 2 or pp.shape[1] != 3:
            raise ValueError('plane_points and normals must both be [M,3]')
        out = np.empty(len(p), np.uint8)
        self._check(self._lib.f3d_inside_polyhedra_f64(self._h, _ptr(p), len(p), _ptr(pp), _ptr(nr), len(pp), _ptr(out)))
        return out.view(np.bool_)

    def project_view(self, points, view, want_uv=True, want_inside=True):
        p = _f64(points)
        v = _f64(view, (VIEW_DOUBLES,))
        uv = np.empty((2, len(p)), np.int32) if want_uv else None
        ins = np.empty(len(p), np.uint8) if want_inside else None
        self._check(self._lib.f3d_project_view_f64(self._h, _ptr(p), len(p), _ptr(v), _ptr(uv), _ptr(ins)))
        return uv, (None if ins is None else ins.view(np.bool_))

    def project_vote_argmax(self, points, views, masks, nclasses=133, threshold=0.5, filter_classes=None,
                            return_votes=False):
        p, dt = _xyz(points)
        views = _f64(views)
        masks = np.ascontiguousarray(masks, dtype=np.uint8)
        if masks.ndim != 3 or views.ndim != 2 or views.shape[1] != VIEW_DOUBLES or len(views) != len(masks):
            raise ValueError(f'views must be [V,{VIEW_DOUBLES}] and masks uint8 [V,H,W]')
        V, H, W = masks.shape
        f, nf = _filter(filter_classes)
        cls = np.empty(len(p), np.int64)
        votes = np.empty((len(p), nclasses + 1), np.uint16) if return_votes else None
        self._check(self._lib.f3d_project_vote_argmax(self._h, _ptr(p), dt, len(p), _ptr(views), V, _ptr(masks), H, W,
                                                      int(nclasses), _ptr(f), nf, float(threshold), _ptr(cls), _ptr(votes)))
        return (cls, votes) if return_votes else cls

    def vote_uv2pt(self, votes, uv2pt, mask_flat):
        """In-place on `votes` (float64 [npts, ncols], C-contiguous), like voting.py:98."""
        if votes.dtype != np.float64 or not votes.flags.c_contiguous or votes.ndim != 2:
            raise ValueError('votes must be a C-contiguous float64 [npts, ncols] array')
        lut = np.ascontiguousarray(uv2pt, dtype=np.int32).reshape(-1)
        m = np.ascontiguousarray(mask_flat, dtype=np.uint8).reshape(-1)
        if len(lut) != len(m):
            raise IndexError(f'shape mismatch: uv2pt has {len(lut)} entries, mask {len(m)}')
        self._check(self._lib.f3d_vote_uv2pt(self._h, _ptr(lut), _ptr(m), len(lut), _ptr(votes), votes.shape[0], votes.shape[1]))
        return votes

    def vote_uv2pt_batch(self, votes, luts, masks, h, w):
        """All frames of VotingSegmentation.vote in one call, in place on `votes` (float64 [npts, ncols], C-contiguous);
        luts int32 [F, h*w], masks uint8 [F, h*w]."""
        if votes.dtype != np.float64 or not votes.flags.c_contiguous or votes.ndim != 2:
            raise ValueError('votes must be a C-contiguous float64 [npts, ncols] array')
        lut = np.ascontiguousarray(luts, dtype=np.int32).reshape(-1, h * w)
        m = np.ascontiguousarray(masks, dtype=np.uint8).reshape(-1, h * w)
        if lut.shape != m.shape:
            raise IndexError(f'shape mismatch: lookups {lut.shape}, masks {m.shape}')
        self._check(self._lib.f3d_vote_uv2pt_batch(self._h, _ptr(lut), _ptr(m), len(lut), int(h), int(w), _ptr(votes), votes.shape[0], votes.shape[1]))
        return votes

    def segment_votes(self, votes, nclasses, threshold=0.5, filter_classes=None):
        v = _f64(votes)
        if v.ndim != 2:
            raise ValueError('votes must be [npts, ncols]')
        f, nf = _filter(filter_classes)
        cls = np.empty(len(v), np.int64)
        if v.shape[1] == 0:
            raise ValueError('attempt to get argmax of an empty sequence')
        self._check(self._lib.f3d_segment_votes(self._h, _ptr(v), v.shape[0], v.shape[1], int(nclasses), float(threshold),
                                                _ptr(f), nf, _ptr(cls)))
        return cls

    def segment_votes_lastcol(self, votes, nclasses, threshold, filter_classes=None):
        """PointVotingSegmentation.segment (voting.py:267-299): segment_votes with the last column as the total and, without a
        filter, the columns before it as the candidates."""
        v = _f64(votes)
        if v.ndim != 2:
            raise ValueError('votes must be [npts, ncols]')
        f, nf = _filter(filter_classes)
        cls = np.empty(len(v), np.int64)
        if v.shape[1] == 0:
            raise IndexError('index -1 is out of bounds for axis 1 with size 0')
        self._check(self._lib.f3d_segment_votes_lastcol(self._h, _ptr(v), v.shape[0], v.shape[1], int(nclasses), float(threshold),
                                                        _ptr(f), nf, _ptr(cls)))
        return cls

    def point_vote_frames(self, votes, cloud, queries, masks, radius):
        """The frames of PointVotingSegmentation.vote in one call (f3d.h f3d_point_vote_frames), in place on `votes` (float64
        [M, ncols], C-contiguous): cloud [M, 3], queries [F, hw, 3] (float32 or float64 each), masks uint8 [F, hw]."""
        if votes.dtype != np.float64 or not votes.flags.c_contiguous or votes.ndim != 2:
            raise ValueError('votes must be a C-contiguous float64 [npts, ncols] array')
        c, cdt = _xyz(cloud)
        q = np.asarray(queries)
        if q.ndim != 3 or q.shape[2] != 3:
            raise ValueError(f'queries must be [F, hw, 3], got {q.shape}')
        qq, qdt = _xyz(q.reshape(-1, 3))
        m = np.ascontiguousarray(masks, dtype=np.uint8).reshape(q.shape[0], -1 if q.shape[0] else q.shape[1])
        if m.shape != q.shape[:2]:
            raise ValueError(f'shape mismatch: queries {q.shape[:2]}, masks {m.shape}')
        if len(c) != votes.shape[0]:
            raise ValueError(f'votes has {votes.shape[0]} rows, the cloud {len(c)} points')
        self._check(self._lib.f3d_point_vote_frames(self._h, _ptr(c), cdt, len(c), _ptr(qq), qdt, _ptr(m), q.shape[0], q.shape[1],
                                                    float(radius), _ptr(votes), votes.shape[1]))
        return votes

    def reserve_mesh_render(self, nviews, h, w):
        """Size all scratch of render_mesh_lookups_dev / vote_faces_dev / vote_visible_mesh_dev (automatic pass size)."""
        self._check(self._lib.f3d_ctx_reserve_mesh_render(self._h, int(nviews), int(h), int(w)))

    def render_lookups(self, points, views, h, w, splat=0, want_depth=True, want_uv2pt=True):
        """Point-splat z-buffer of the cloud in every view (f3d.h f3d_render_lookups) -> depth float32 [V, h, w] (+inf = empty),
        uv2pt int32 [V, h*w] (-1 = empty): the nearest point by float32 depth per pixel, ties to the lowest index."""
        p, dt = _xyz(points)
        views = _f64(views)
        if views.ndim != 2 or views.shape[1] != VIEW_DOUBLES:
            raise ValueError(f'views must be [V,{VIEW_DOUBLES}]')
        V, h, w = len(views), int(h), int(w)
        depth = np.empty((V, h, w), np.float32) if want_depth else None
        uv2pt = np.empty((V, h * w), np.int32) if want_uv2pt else None
        self._check(self._lib.f3d_render_lookups(self._h, _ptr(p), dt, len(p), _ptr(views), V, h, w, int(splat), _ptr(depth), _ptr(uv2pt)))
        return depth, uv2pt

    def vote_visible(self, votes, points, views, masks, splat=1, depth_tol=0.05, views_per_pass=0):
        """The forward vote with the visibility test of f3d.h f3d_vote_visible, in place on `votes` (float64 [N, ncols],
        C-contiguous): only samples within depth_tol of the front surface of their pixel vote.  views_per_pass = 0: automatic."""
        if votes.dtype != np.float64 or not votes.flags.c_contiguous or votes.ndim != 2:
            raise ValueError('votes must be a C-contiguous float64 [npts, ncols] array')
        p, dt = _xyz(points)
        views = _f64(views)
        masks = np.ascontiguousarray(masks, dtype=np.uint8)
        if masks.ndim != 3 or views.ndim != 2 or views.shape[1] != VIEW_DOUBLES or len(views) != len(masks):
            raise ValueError(f'views must be [V,{VIEW_DOUBLES}] and masks uint8 [V,H,W]')
        if len(p) != votes.shape[0]:
            raise ValueError(f'votes has {votes.shape[0]} rows, the cloud {len(p)} points')
        V, H, W = masks.shape
        self._check(self._lib.f3d_vote_visible(self._h, _ptr(p), dt, len(p), _ptr(views), V, _ptr(masks), H, W, int(splat), float(depth_tol),
                                               _ptr(votes), votes.shape[1], int(views_per_pass)))
        return votes

    def fuse_features(self, sums, counts, points, views, h, w, feats, splat=1, depth_tol=0.05, views_per_pass=0):
        """Adds the feature rows of the visible samples to `sums` (float32 [N, d]) and their number to `counts` (int32 [N]), both in
        place (f3d.h f3d_fuse_features): feats float16 / float32 [V, hf, wf, d], one map per view; h, w = the image size of the samples
        and the z-buffer.  Callable repeatedly: the views of later calls add to the same sums."""
        p, dt = _xyz(points)
        views = _views(views)
        feats = np.asarray(feats)
        ft = features_check(sums, counts, feats, len(views), len(p))
        V, hf, wf, d = feats.shape
        self._check(self._lib.f3d_fuse_features(self._h, _ptr(p), dt, len(p), _ptr(views), V, int(h), int(w), _ptr(feats), ft, hf, wf, d,
                                                int(splat), float(depth_tol), _ptr(sums), _ptr(counts), int(views_per_pass)))
        return sums, counts

    def features_finalize(self, sums, counts, normalize=True, out=None):
        """Per-point mean rows, unit length with `normalize`, zeros where counts is 0 (f3d.h f3d_features_finalize) -> float32 [N, d];
        out may be `sums` itself."""
        features_check(sums, counts)
        if out is None:
            out = np.empty_like(sums)
        elif out.dtype != np.float32 or out.shape != sums.shape or not out.flags.c_contiguous:
            raise ValueError('out must be a C-contiguous float32 array of the shape of sums')
        self._check(self._lib.f3d_features_finalize(self._h, _ptr(sums), _ptr(counts), sums.shape[0], sums.shape[1], int(bool(normalize)),
                                                    _ptr(out)))
        return out

    def render_mesh_lookups(self, vertices, triangles, views, h, w, z_far=np.inf, want_depth=True, want_uv2tri=True, want_straddling=True):
        """Triangle z-buffer of the mesh in every view (f3d.h f3d_render_mesh_lookups) -> depth float32 [V, h, w] (+inf = empty),
        uv2tri int32 [V, h*w] (-1 = empty), straddling int64 [V] (triangles skipped because they cross the camera plane)."""
        vx, vdt, tr, it = _mesh(vertices, triangles)
        views = _views(views)
        V, h, w = len(views), int(h), int(w)
        depth = np.empty((V, h, w), np.float32) if want_depth else None
        uv2tri = np.empty((V, h * w), np.int32) if want_uv2tri else None
        straddling = np.empty(V, np.int64) if want_straddling else None
        self._check(self._lib.f3d_render_mesh_lookups(self._h, _ptr(vx), vdt, len(vx), _ptr(tr), it, len(tr), _ptr(views), V, h, w, float(z_far),
                                                      _ptr(depth), _ptr(uv2tri), _ptr(straddling)))
        return depth, uv2tri, straddling

    def vote_faces(self, votes, vertices, triangles, views, masks, z_far=np.inf, views_per_pass=0):
        """Every pixel votes for the triangle it sees (f3d.h f3d_vote_faces), in place on `votes` (float64 [nt, ncols], C-contiguous)."""
        if votes.dtype != np.float64 or not votes.flags.c_contiguous or votes.ndim != 2:
            raise ValueError('votes must be a C-contiguous float64 [nt, ncols] array')
        vx, vdt, tr, it = _mesh(vertices, triangles)
        views = _views(views)
        masks = np.ascontiguousarray(masks, dtype=np.uint8)
        if masks.ndim != 3 or len(views) != len(masks):
            raise ValueError(f'views must be [V,{VIEW_DOUBLES}] and masks uint8 [V,H,W]')
        if len(tr) != votes.shape[0]:
            raise ValueError(f'votes has {votes.shape[0]} rows, the mesh {len(tr)} triangles')
        V, H, W = masks.shape
        self._check(self._lib.f3d_vote_faces(self._h, _ptr(vx), vdt, len(vx), _ptr(tr), it, len(tr), _ptr(views), V, _ptr(masks), H, W, float(z_far),
                                             _ptr(votes), votes.shape[1], int(views_per_pass)))
        return votes

    def vote_visible_mesh(self, votes, points, vertices, triangles, views, masks, z_far=np.inf, depth_tol=0.05, views_per_pass=0):
        """The forward vote of the cloud with the mesh as the occluder (f3d.h f3d_vote_visible_mesh), in place on `votes`
        (float64 [N, ncols], C-contiguous)."""
        if votes.dtype != np.float64 or not votes.flags.c_contiguous or votes.ndim != 2:
            raise ValueError('votes must be a C-contiguous float64 [npts, ncols] array')
        p, dt = _xyz(points)
        vx, vdt, tr, it = _mesh(vertices, triangles)
        views = _views(views)
        masks = np.ascontiguousarray(masks, dtype=np.uint8)
        if masks.ndim != 3 or len(views) != len(masks):
            raise ValueError(f'views must be [V,{VIEW_DOUBLES}] and masks uint8 [V,H,W]')
        if len(p) != votes.shape[0]:
            raise ValueError(f'votes has {votes.shape[0]} rows, the cloud {len(p)} points')
        V, H, W = masks.shape
        self._check(self._lib.f3d_vote_visible_mesh(self._h, _ptr(p), dt, len(p), _ptr(vx), vdt, len(vx), _ptr(tr), it, len(tr), _ptr(views), V,
                                                    _ptr(masks), H, W, float(z_far), float(depth_tol), _ptr(votes), votes.shape[1],
                                                    int(views_per_pass)))
        return votes

    def sem_logits_to_mask(self, sem, conf_threshold=0.017, low_label=133):
        s = np.ascontiguousarray(sem, dtype=np.float32)
        if s.ndim != 3:
            raise ValueError('sem must be [C,H,W]')
        c, h, w = s.shape
        out = np.empty((h, w), np.uint8)
        self._check(self._lib.f3d_sem_logits_to_mask(self._h, _ptr(s), c, h * w, float(conf_threshold or 0.0), int(low_label), _ptr(out)))
        return out

    def points_in_obb(self, points, boxes, want_bits=True, want_cooc=True):
        """boxes: float64 [B,15] = center(3), R row-major(9), extent(3).  Returns (inside bool [N,B] or None, cooc bool [B,B] or None)."""
        p, dt = _xyz(points)
        b = _f64(boxes)
        if b.ndim != 2 or b.shape[1] != OBB_DOUBLES:
            raise ValueError('boxes must be [B,15]')
        B = len(b)
        words = (B + 31) // 32
        bits = np.zeros((len(p), words), np.uint32) if want_bits else None
        cooc = np.zeros((B, B), np.uint8) if want_cooc else None
        if B:
            self._check(self._lib.f3d_points_in_obb(self._h, _ptr(p), dt, len(p), _ptr(b), B, _ptr(bits), _ptr(cooc)))
        inside = None
        if want_bits:
            inside = np.unpackbits(bits.view(np.uint8), axis=1, bitorder='little')[:, :B].astype(bool)
        return inside, (None if cooc is None else cooc.astype(bool))

    # ---- per-instance point lists and hull candidates (merge_bb's box fits); host-pointer sequence, state kept in the context
    def group_by_id(self, ids, nids):
        """order int32 [n] (members of id 0, 1, ... in ascending point index; ids outside [0, nids) last), starts int64 [nids + 2]."""
        i = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        order = np.empty(len(i), np.int32)
        starts = np.empty(int(nids) + 2, np.int64)
        self._check(self._lib.f3d_group_by_id(self._h, _ptr(i), len(i), int(nids), _ptr(order), _ptr(starts)))
        self._grp = (len(i), int(nids))
        return order, starts

    def obb_extremes(self, points):
        """int32 [nids, 26]: per id the member extreme along +-x, +-y, +-z and the face / body diagonals (-1: no members).
        Follows group_by_id of the same cloud."""
        p, dt = _xyz(points)
        n, nids = self._grp
        out = np.empty((nids, 26), np.int32)
        self._check(self._lib.f3d_obb_extremes(self._h, _ptr(p), dt, len(p), _ptr(out)))
        return out

    def obb_hull_filter(self, facet_start, facets, margin):
        """Members not strictly inside their id's polytope: (cand int32 [n] grouped like `order`, cand_count int32 [nids]).
        Follows group_by_id and obb_extremes of the same cloud."""
        n, nids = self._grp
        fs = np.ascontiguousarray(facet_start, dtype=np.int32)
        eq = np.ascontiguousarray(facets, dtype=np.float64).reshape(-1, 4)
        mg = np.ascontiguousarray(margin, dtype=np.float64)
        if len(fs) != nids + 1 or len(mg) != nids or fs[-1] != len(eq):
            raise ValueError('facet_start must have nids + 1 entries ending at len(facets); margin one entry per id')
        cand = np.empty(n, np.int32)
        cnt = np.empty(nids, np.int32)
        self._check(self._lib.f3d_obb_hull_filter(self._h, n, _ptr(fs), _ptr(eq), _ptr(mg), _ptr(cand), _ptr(cnt)))
        return cand, cnt

    def obb_fit(self, point_sets, want_vertices=False):
        """Oriented boxes (Open3D's create_from_points recipe) of a list of point sets in ONE launch: boxes float64 [k, 15] (center,
        R row-major with the axes as columns, extent), status int32 [k] (OBB_OK / OBB_FEW / OBB_DEFERRED: fit that one on the host);
        with want_vertices also a list of bool arrays marking every set's hull vertices."""
        sets = [_f64(np.asarray(p).reshape(-1, 3)) for p in point_sets]
        start = np.zeros(len(sets) + 1, np.int64)
        start[1:] = np.cumsum([len(p) for p in sets])
        pts = np.ascontiguousarray(np.concatenate(sets)) if sets and start[-1] else np.zeros((0, 3))
        boxes = np.zeros((len(sets), OBB_DOUBLES))
        status = np.zeros(len(sets), np.int32)
        isvert = np.zeros(len(pts), np.uint8) if want_vertices else None
        self._check(self._lib.f3d_obb_fit(self._h, _ptr(pts), _ptr(start), len(sets), _ptr(boxes), _ptr(status), _ptr(isvert), None))
        if want_vertices:
            return boxes, status, [isvert[start[k]:start[k + 1]].view(np.bool_) for k in range(len(sets))]
        return boxes, status

    def relabel(self, ids, from_id, to_id):
        if ids.dtype != np.int64 or not ids.flags.c_contiguous:
            raise ValueError('ids must be a C-contiguous int64 array')
        cnt = np.zeros(1, np.int64)
        self._check(self._lib.f3d_relabel(self._h, _ptr(ids), ids.size, int(from_id), int(to_id), _ptr(cnt)))
        return int(cnt[0])

    # ---- the other intersections.py primitives (a12)
    def ray_x_lines(self, origin, direction, starts, ends):
        o, d, s, e = _f64(origin, (3,)), _f64(direction, (3,)), _n3(starts), _n3(ends)
        pts, within = np.empty_like(s), np.empty(len(s), np.uint8)
        self._check(self._lib.f3d_ray_x_lines(self._h, _ptr(o), _ptr(d), _ptr(s), _ptr(e), len(s), _ptr(pts), _ptr(within)))
        return pts, within.view(np.bool_)

    def rays_x_plane(self, plane_point, plane_normal, origins, directions):
        pp, pn, o, d = _f64(plane_point, (3,)), _f64(plane_normal, (3,)), _n3(origins), _n3(directions)
        pts, valid = np.empty_like(o), np.empty(len(o), np.uint8)
        self._check(self._lib.f3d_rays_x_plane(self._h, _ptr(pp), _ptr(pn), _ptr(o), _ptr(d), len(o), _ptr(pts), _ptr(valid)))
        return pts, valid.view(np.bool_)

    def lines_x_planes(self, line_origins, line_ends, plane_points, plane_normals):
        lo, le, pp, pn = _n3(line_origins), _n3(line_ends), _n3(plane_points), _n3(plane_normals)
        pts, valid = np.empty((len(lo), len(pp), 3)), np.empty((len(lo), len(pp)), np.uint8)
        self._check(self._lib.f3d_lines_x_planes(self._h, _ptr(lo), _ptr(le), len(lo), _ptr(pp), _ptr(pn), len(pp), _ptr(pts), _ptr(valid)))
        return pts, valid.view(np.bool_)

    def point_inside_polygon(self, points, vertices):
        p, v = _n3(points), _n3(vertices)
        inside, within = np.empty(len(p), np.uint8), np.empty((len(v), len(p)), np.uint8)
        self._check(self._lib.f3d_point_inside_polygon(self._h, _ptr(p), len(p), _ptr(v), len(v), _ptr(inside), _ptr(within)))
        return inside.view(np.bool_), within.view(np.bool_)

    def points_plane_projection(self, points, plane_point, normal):
        p, pp, nr = _n3(points), _f64(plane_point, (3,)), _f64(normal, (3,))
        out = np.empty_like(p)
        self._check(self._lib.f3d_points_plane_projection(self._h, _ptr(p), len(p), _ptr(pp), _ptr(nr), _ptr(out)))
        return out

    def lines_plane_projection(self, starts, ends, plane_point, normal):
        s, e, pp, nr = _n3(starts), _n3(ends), _f64(plane_point, (3,)), _f64(normal, (3,))
        sp, ep, dr = np.empty_like(s), np.empty_like(s), np.empty_like(s)
        self._check(self._lib.f3d_lines_plane_projection(self._h, _ptr(s), _ptr(e), len(s), _ptr(pp), _ptr(nr), _ptr(sp), _ptr(ep), _ptr(dr)))
        return sp, ep, dr

    def components_same_class(self, classes, offsets, neighbours):
        """root[i] = smallest index of point i's same-class connected component (CSR adjacency, symmetric)."""
        cls = np.ascontiguousarray(classes, dtype=np.int64)
        offs, nb = host_csr(offsets, neighbours, len(cls))
        root = np.empty(len(cls), np.int64)
        self._check(self._lib.f3d_components_same_class(self._h, _ptr(cls), len(cls), _ptr(offs), _ptr(nb), _ptr(root)))
        return root

    def flood_order(self, classes, offsets, neighbours, instance_classes):
        """Ordered same-class flood of CVSegmentation.instance_seperate (include/f3d.h f3d_flood_order): the clusters of
        `instance_classes` (processing order), numbered by class rank then ascending seed.  -> (root int64 [n], order int64 [L]
        (the clusters concatenated in the reference's pop order), coffs int64 [M + 1], boundary flags bool [n], stats dict)."""
        cls = np.ascontiguousarray(classes, dtype=np.int64)
        inst = np.ascontiguousarray(np.asarray(instance_classes).reshape(-1), dtype=np.int64)
        n = len(cls)
        offs, nb = host_csr(offsets, neighbours, n)
        root, order, coffs = np.empty(n, np.int64), np.empty(n, np.int64), np.zeros(n + 1, np.int64)
        flags, stats = np.zeros(n, np.uint8), np.zeros(4, np.int64)
        self._check(self._lib.f3d_flood_order(self._h, _ptr(cls), n, _ptr(offs), _ptr(nb), _ptr(inst), len(inst), _ptr(root),
                                              _ptr(order), _ptr(coffs), _ptr(flags), _ptr(stats)))
        m, L = int(stats[0]), int(stats[1])
        return root, order[:L], coffs[:m + 1], flags.view(bool), _flood_stats(stats)

    def color_segment(self, colors, offsets, neighbours, ids, seeds, threshold, neutral_ids=(0,), max_level=10):
        """Running-mean colour growing of CVSegmentation.color_segment (include/f3d.h f3d_color_segment); `ids` (int64, C-contiguous)
        is updated in place and returned with the number of accepted points."""
        clr = np.asarray(colors)
        if clr.dtype not in (np.float64, np.float32):
            raise TypeError(f'color_segment: colours must be float64 or float32, got {clr.dtype}')
        clr = np.ascontiguousarray(clr)
        n = len(ids)
        if clr.shape != (n, 3):
            raise ValueError(f'color_segment: colours must be [{n}, 3], got {clr.shape}')
        if not (isinstance(ids, np.ndarray) and ids.dtype == np.int64 and ids.flags.c_contiguous):
            raise TypeError('color_segment: ids must be a C-contiguous int64 array (it is updated in place)')
        offs, nb = host_csr(offsets, neighbours, n)
        sd = np.ascontiguousarray(np.asarray(seeds).reshape(-1), dtype=np.int64)
        thr = _threshold3(threshold)
        neu = np.ascontiguousarray(np.asarray(list(neutral_ids)).reshape(-1), dtype=np.int64)
        acc = np.zeros(1, np.int64)
        self._check(self._lib.f3d_color_segment(self._h, _ptr(clr), dtype_code(clr), n, _ptr(offs), _ptr(nb),
                                                _ptr(ids), _ptr(sd), len(sd), _ptr(thr), _ptr(neu), len(neu), int(max_level), _ptr(acc)))
        return ids, int(acc[0])

    def region_grow(self, values, offsets, neighbours, seeds, sma0, npts0, threshold, max_level, seeds_given=False):
        """Region growing of segUtils/refinement.py (include/f3d.h f3d_region_grow): values float64 [n] / [n, 1], or float64 / float32
        [n, 3]; seeds = the first queue, distinct.  -> the accepted points int64 [count], in acceptance order."""
        val = np.asarray(values)
        if val.dtype not in (np.float64, np.float32):
            raise TypeError(f'region_grow: values must be float64 or float32, got {val.dtype}')
        val = np.ascontiguousarray(val)
        n = len(val)
        nchan = 1 if val.ndim == 1 else val.shape[1] if val.ndim == 2 else 0
        if nchan not in (1, 3) or (nchan == 1 and val.dtype != np.float64):
            raise ValueError(f'region_grow: values must be float64 [n] or float64 / float32 [n, 3], got {val.dtype} {val.shape}')
        offs, nb = host_csr(offsets, neighbours, n)
        sd = np.ascontiguousarray(np.asarray(seeds).reshape(-1), dtype=np.int64)
        sma, thr = _grow_params(nchan, sma0, threshold)
        cluster, count = np.empty(n, np.int64), np.zeros(1, np.int64)
        self._check(self._lib.f3d_region_grow(self._h, _ptr(val), dtype_code(val), nchan, n, _ptr(offs), _ptr(nb),
                                              _ptr(sd), len(sd), _ptr(sma), int(npts0), int(bool(seeds_given)), _ptr(thr), int(max_level),
                                              _ptr(cluster), _ptr(count)))
        return cluster[:int(count[0])].copy()

    def plane_distance(self, points, plane_point, normal):
        """|((x - px) nx + (y - py) ny) + (z - pz) nz| of float64 points [n, 3] -> float64 [n]."""
        pts = _n3(points, 'plane_distance: points must be [N, 3], got {}')
        pp, nr = _f64(np.asarray(plane_point).reshape(-1), (3,)), _f64(np.asarray(normal).reshape(-1), (3,))
        out = np.empty(len(pts))
        self._check(self._lib.f3d_plane_distance(self._h, _ptr(pts), len(pts), _ptr(pp), _ptr(nr), _ptr(out)))
        return out

    # meshUtils (include/f3d.h f3d_mesh_*): verts float64 / float32 [V, 3], tris int64 / int32 [M, 3], masks bool [V], all C-contiguous
    # NumPy arrays (Fusion3DSeg.segUtils.meshUtils checks them).  An index outside [0, V) raises IndexError.
    def mesh_vertex_map(self, tris, nvertices):
        """-> the CSR of vertex_triangle_mapping: (offsets int64 [V + 1], tri int32 [3M], pos int8 [3M])."""
        nt, nv = len(tris), int(nvertices)
        offsets, tri, pos, counts = np.empty(nv + 1, np.int64), np.empty(3 * nt, np.int32), np.empty(3 * nt, np.int8), np.zeros(4, np.int64)
        self._check(self._lib.f3d_mesh_vertex_map(self._h, _ptr(tris), index_code(tris), nt, nv, _ptr(offsets), _ptr(tri), _ptr(pos), _ptr(counts)))
        return offsets, tri, pos

    def mesh_remove_faces(self, tris, nvertices, mask):
        """-> (not_removed bool [M], remaining [Q, 3] of tris' dtype, oldids2newids int64 [V])."""
        nt, nv = len(tris), int(nvertices)
        nr, rem, o2n, counts = np.empty(nt, bool), np.empty((nt, 3), tris.dtype), np.empty(nv, np.int64), np.zeros(4, np.int64)
        self._check(self._lib.f3d_mesh_remove_faces(self._h, _ptr(tris), index_code(tris), nt, nv, _ptr(mask), _ptr(nr), _ptr(rem), _ptr(o2n),
                                                    _ptr(counts)))
        return nr, rem[:counts[0]], o2n

    def mesh_keep_faces(self, verts, tris, mask):
        """-> (remaining vertices [P, 3] of verts' dtype, remaining triangles [Q, 3] of tris' dtype)."""
        nt, nv = len(tris), len(verts)
        ov, ot, counts = np.empty((min(3 * nt, nv), 3), verts.dtype), np.empty((nt, 3), tris.dtype), np.zeros(4, np.int64)
        self._check(self._lib.f3d_mesh_keep_faces(self._h, _ptr(verts), dtype_code(verts), nv, _ptr(tris), index_code(tris), nt, _ptr(mask), _ptr(ov),
                                                  _ptr(ot), _ptr(counts)))
        return ov[:counts[0]], ot[:counts[1]]

    def mesh_triangle_clusters(self, verts, tris, want_tri_area=False):
        """-> (triangle_clusters int32 [M], cluster_n_triangles int64 [P], cluster_area float64 [P]) (+ the triangle areas [M])."""
        nt, nv = len(tris), len(verts)
        cl, cn, ca, counts = np.empty(nt, np.int32), np.empty(nt, np.int64), np.empty(nt, np.float64), np.zeros(4, np.int64)
        ta = np.empty(nt, np.float64) if want_tri_area else None
        self._check(self._lib.f3d_mesh_triangle_clusters(self._h, _ptr(verts), dtype_code(verts), nv, _ptr(tris), index_code(tris), nt, _ptr(cl), _ptr(cn),
                                                         _ptr(ca), _ptr(ta), _ptr(counts)))
        out = (cl, cn[:counts[0]].copy(), ca[:counts[0]].copy())
        return out + (ta,) if want_tri_area else out

    def mesh_clean(self, verts, tris, remove_mask, min_triangles, min_area):
        """-> (new vertices, new triangles, kept_vertex_mask bool [V], kept_triangle_mask bool [M])."""
        nt, nv = len(tris), len(verts)
        nvs, nts, counts = np.empty((nv, 3), verts.dtype), np.empty((nt, 3), tris.dtype), np.zeros(4, np.int64)
        kv, kt = np.zeros(nv, bool), np.zeros(nt, bool)
        self._check(self._lib.f3d_mesh_clean(self._h, _ptr(verts), dtype_code(verts), nv, _ptr(tris), index_code(tris), nt, _ptr(remove_mask),
                                             int(min_triangles), float(min_area), _ptr(nvs), _ptr(nts), _ptr(kv), _ptr(kt), _ptr(counts)))
        return nvs[:counts[1]].copy(), nts[:counts[0]].copy(), kv, kt

    def mesh_face_frames(self, verts, tris, want_centroids=False, want_areas=False):
        """-> (normals float64 [M, 3], centroids float64 [M, 3] or None, areas float64 [M] or None) (f3d.h f3d_mesh_face_frames)."""
        nt, nv = len(tris), len(verts)
        normals, counts = np.empty((nt, 3), np.float64), np.zeros(4, np.int64)
        centroids = np.empty((nt, 3), np.float64) if want_centroids else None
        areas = np.empty(nt, np.float64) if want_areas else None
        self._check(self._lib.f3d_mesh_face_frames(self._h, _ptr(verts), dtype_code(verts), nv, _ptr(tris), index_code(tris), nt, _ptr(normals),
                                                   _ptr(centroids), _ptr(areas), _ptr(counts)))
        return normals, centroids, areas

    def mesh_face_graph(self, tris, nvertices, verts=None, cos_crease=None, offsets=None, neighbours=None):
        """The face graph (f3d.h f3d_mesh_face_graph), gated when cos_crease is given (it needs verts) -> (offsets int64 [M + 1],
        neighbours int32 [cap], counts int64 [4]).  neighbours (default: 3 M entries) is filled only when counts[0] <= its length."""
        nt = len(tris)
        gate = cos_crease is not None
        if gate and verts is None:
            raise ValueError('mesh_face_graph: a gate needs the vertices')
        if offsets is None:
            offsets = np.empty(nt + 1, np.int64)
        if neighbours is None:
            neighbours = np.empty(3 * nt, np.int32)
        counts = np.zeros(4, np.int64)
        self._check(self._lib.f3d_mesh_face_graph(self._h, _ptr(verts) if gate else None, dtype_code(verts) if gate else F64, int(nvertices), _ptr(tris),
                                                  index_code(tris), nt, int(gate), float(cos_crease) if gate else 0.0, _ptr(offsets),
                                                  _ptr(neighbours) if len(neighbours) else None, len(neighbours), _ptr(counts)))
        return offsets, neighbours, counts

    def lift_overlaps(self, luts, inst, npoints, max_ids, cap):
        """Segment sizes and overlaps (f3d.h f3d_lift_overlaps).  luts int32 [F, HW], inst uint16 [F, HW], C-contiguous -> (sizes int32
        [F * max_ids], pairs int32 [cap, 2], counts int32 [cap], stats int64 [6]); pairs / counts are filled only when stats[0] <= cap."""
        nf, hw = luts.shape
        sizes, pairs, counts = np.zeros(nf * int(max_ids), np.int32), np.zeros((int(cap), 2), np.int32), np.zeros(int(cap), np.int32)
        stats = np.zeros(6, np.int64)
        self._check(self._lib.f3d_lift_overlaps(self._h, _ptr(luts), _ptr(inst), nf, hw, int(npoints), int(max_ids), _ptr(sizes),
                                                _ptr(pairs) if cap else None, _ptr(counts) if cap else None, int(cap), _ptr(stats)))
        return sizes, pairs, counts, stats

    def lift_instances(self, luts, inst, npoints, max_ids, ratio, min_overlap, seg_classes, min_points):
        """3D instances from per-frame ids (f3d.h f3d_lift_instances).  luts int32 [F, HW], inst uint16 [F, HW], seg_classes int32
        [F * max_ids] or None -> (ids int32 [N], support uint16 [N], seen uint16 [N], seg2inst int32 [S], inst_points int64 [S + 1] of
        which the first stats[1] + 1 entries are written, stats int64 [6])."""
        nf, hw = luts.shape
        n, nseg = int(npoints), nf * int(max_ids)
        ids, support, seen = np.zeros(n, np.int32), np.zeros(n, np.uint16), np.zeros(n, np.uint16)
        seg2inst, inst_points, stats = np.zeros(nseg, np.int32), np.zeros(nseg + 1, np.int64), np.zeros(6, np.int64)
        self._check(self._lib.f3d_lift_instances(self._h, _ptr(luts), _ptr(inst), nf, hw, n, int(max_ids), float(ratio), int(min_overlap),
                                                 _ptr(seg_classes), int(min_points), _ptr(ids), _ptr(support), _ptr(seen), _ptr(seg2inst),
                                                 _ptr(inst_points), _ptr(stats)))
        return ids, support, seen, seg2inst, inst_points, stats

    def extract_planes(self, points, offsets, neighbours, normals, cos_angle, offset, dist, max_variation, min_points, max_rounds,
                       max_planes, want_normals=False):
        """Plane table of a cloud over its adjacency (include/f3d.h f3d_extract_planes).  points float64 / float32 [n, 3]; offsets /
        neighbours a checked host CSR; normals float64 [n, 3] or None (PCA of the rows).  -> (labels int32 [n], planes float64
        [P, 8], corners float64 [P, 4, 3], counts int64 [4]) (+ the computed normals [n, 3] with want_normals and normals None)."""
        n, mp = len(points), int(max_planes)
        rows = max(mp, 0)                                           # (a negative max_planes is the library's ValueError)
        labels, planes, corners, counts = np.empty(n, np.int32), np.zeros((rows, 8)), np.zeros((rows, 4, 3)), np.zeros(4, np.int64)
        nout = np.zeros((n, 3)) if want_normals and normals is None else None
        self._check(self._lib.f3d_extract_planes(self._h, _ptr(points), dtype_code(points), n, _ptr(offsets), _ptr(neighbours), _ptr(normals),
                                                 float(cos_angle), float(offset), float(dist), float(max_variation), int(min_points),
                                                 int(max_rounds), mp, _ptr(labels), _ptr(planes), _ptr(corners), _ptr(counts), _ptr(nout)))
        out = (labels, planes[:counts[0]].copy(), corners[:counts[0]].copy(), counts)
        return out + (nout,) if want_normals else out

    def smooth_votes(self, votes, offsets, neighbours, normals=None, cos_angle=0.0, colors=None, max_color_dist=0.0, self_weight=1.0,
                     iterations=1, out=None):
        """Neighbour-summed vote rows (include/f3d.h f3d_smooth_votes).  votes float64 / uint16 [n, ncols], C-contiguous; offsets /
        neighbours a checked host CSR; normals float64 [n, 3] or None; colors float64 / float32 [n, 3] or None.  -> float64 [n, ncols]
        (`out` when given: C-contiguous float64 of that shape, not overlapping votes)."""
        offsets, neighbours, normals, colors = _smooth_arrays(votes, offsets, neighbours, normals, colors)
        if out is None:
            out = np.empty(votes.shape, np.float64)
        elif out.dtype != np.float64 or out.shape != votes.shape or not out.flags.c_contiguous:
            raise ValueError('out must be a C-contiguous float64 array of the shape of votes')
        self._check(self._lib.f3d_smooth_votes(self._h, _ptr(votes), _vtype(votes), votes.shape[0], votes.shape[1], _ptr(offsets),
                                               _ptr(neighbours), _ptr(normals), float(cos_angle), _ptr(colors),
                                               F64 if colors is None else dtype_code(colors), float(max_color_dist), float(self_weight),
                                               int(iterations), _ptr(out)))
        return out

    def smooth_segment(self, votes, offsets, neighbours, nclasses, threshold=0.5, filter_classes=None, lastcol=False, normals=None,
                       cos_angle=0.0, colors=None, max_color_dist=0.0, self_weight=1.0, iterations=1):
        """segment_votes (lastcol: segment_votes_lastcol) of the smoothed matrix, whose last iteration is never written
        (include/f3d.h f3d_smooth_segment).  Arrays as for smooth_votes.  -> classes int64 [n]."""
        offsets, neighbours, normals, colors = _smooth_arrays(votes, offsets, neighbours, normals, colors)
        f, nf = _filter(filter_classes)
        cls = np.empty(votes.shape[0], np.int64)
        self._check(self._lib.f3d_smooth_segment(self._h, _ptr(votes), _vtype(votes), votes.shape[0], votes.shape[1], _ptr(offsets),
                                                 _ptr(neighbours), _ptr(normals), float(cos_angle), _ptr(colors),
                                                 F64 if colors is None else dtype_code(colors), float(max_color_dist), float(self_weight),
                                                 int(iterations), int(nclasses), float(threshold), _ptr(f), nf, int(bool(lastcol)),
                                                 _ptr(cls)))
        return cls

    def door_window_quads(self, points, ids, instance_ids, vertices, triangles):
        """Door / window quads of door_window_bbox.generate_mesh (include/f3d.h f3d_door_window_quads) for the distinct ids
        `instance_ids`.  -> (quads float64 [k, 4, 3], status int32 [k] (QUAD_*), chosen triangle int32 [k], triangle normals
        float64 [T, 3])."""
        pts = _n3(points, 'door_window_quads: points must be [N, 3], got {}')
        ids_ = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if len(ids_) != len(pts):
            raise ValueError(f'door_window_quads: {len(ids_)} ids for {len(pts)} points')
        inst = np.ascontiguousarray(np.asarray(instance_ids).reshape(-1), dtype=np.int64)
        verts = _f64(vertices).reshape(-1, 3)
        tris = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
        k, nt = len(inst), len(tris)
        quads, status, tri = np.empty((k, 4, 3)), np.empty(k, np.int32), np.empty(k, np.int32)
        normals = np.empty((nt, 3))
        self._check(self._lib.f3d_door_window_quads(self._h, _ptr(pts), len(pts), _ptr(ids_), _ptr(inst), k, _ptr(verts), len(verts),
                                                    _ptr(tris), nt, _ptr(quads), _ptr(status), _ptr(tri), _ptr(normals)))
        return quads, status, tri, normals

    def patch_owner(self, uv, seed_pts, seed_normals, frame_pts, frame_normals, free, h, w, half, radius, min_cosine):
        """owner int32 [h*w]: for every free depth pixel the first seed of Fusion.fuse's matching loop (fusion.py:269-298)
        that would take it, -1 if none."""
        uv = np.ascontiguousarray(uv, dtype=np.int32)
        sp, sn = _f64(seed_pts), _f64(seed_normals)
        qp, qn = _f64(frame_pts, (h * w, 3)), _f64(frame_normals, (h * w, 3))
        fr = np.ascontiguousarray(free, dtype=np.uint8).reshape(-1)
        m = len(sp)
        if uv.shape != (2, m) or sn.shape != (m, 3) or len(fr) != h * w:
            raise ValueError('patch_owner: uv must be [2,m], seeds [m,3], free [h*w]')
        owner = np.empty(h * w, np.int32)
        self._check(self._lib.f3d_patch_owner(self._h, _ptr(uv), m, h, w, int(half), float(radius), float(min_cosine), _ptr(sp), _ptr(sn),
                                              _ptr(qp), _ptr(qn), _ptr(fr), _ptr(owner)))
        return owner

    def patch_match(self, uv, seed_pts, seed_normals, frame_pts, frame_normals, frame_colors, free, h, w, half, radius, min_cosine):
        """patch_owner plus, per seed, the ordered sums of the frame rows it takes: (owner int32 [h*w], sums float64 [m, 9] =
        points | normals | colours, counts int32 [m])."""
        uv = np.ascontiguousarray(uv, dtype=np.int32)
        sp, sn = _f64(seed_pts), _f64(seed_normals)
        qp, qn = _f64(frame_pts, (h * w, 3)), _f64(frame_normals, (h * w, 3))
        qc = None if frame_colors is None else _f64(frame_colors, (h * w, 3))
        fr = np.ascontiguousarray(free, dtype=np.uint8).reshape(-1)
        m = len(sp)
        if uv.shape != (2, m) or sn.shape != (m, 3) or len(fr) != h * w:
            raise ValueError('patch_match: uv must be [2,m], seeds [m,3], free [h*w]')
        owner, sums, counts = np.empty(h * w, np.int32), np.zeros((m, 9)), np.zeros(m, np.int32)
        self._check(self._lib.f3d_patch_match(self._h, _ptr(uv), m, h, w, int(half), float(radius), float(min_cosine), _ptr(sp), _ptr(sn),
                                              _ptr(qp), _ptr(qn), _ptr(qc), _ptr(fr), _ptr(owner), _ptr(sums), _ptr(counts)))
        return owner, sums, counts

    def patch_seeds_sums(self, frame_pts, frame_normals, frame_colors, prio, free, h, w, half, radius, min_cosine):
        """Fusion.patch_downsample's seeds, what they take and the ordered sums per seed pixel: (owner int32 [h*w] (seed pixel index,
        -1 = nobody), sums float64 [h*w, 9], counts int32 [h*w], rounds)."""
        qp, qn = _f64(frame_pts, (h * w, 3)), _f64(frame_normals, (h * w, 3))
        qc = None if frame_colors is None else _f64(frame_colors, (h * w, 3))
        pr = np.ascontiguousarray(prio, dtype=np.int32).reshape(-1)
        fr = np.ascontiguousarray(free, dtype=np.uint8).reshape(-1)
        if len(pr) != h * w or len(fr) != h * w:
            raise ValueError('patch_seeds_sums: prio and free must have h*w entries')
        owner, sums, counts = np.empty(h * w, np.int32), np.zeros((h * w, 9)), np.zeros(h * w, np.int32)
        rounds = C.c_int32(0)
        self._check(self._lib.f3d_patch_seeds_sums(self._h, _ptr(qp), _ptr(qn), _ptr(qc), _ptr(pr), _ptr(fr), h, w, int(half), float(radius),
                                                   float(min_cosine), _ptr(owner), _ptr(sums), _ptr(counts), C.byref(rounds)))
        return owner, sums, counts, rounds.value

    def unproject_depth(self, depth, K, q_wxyz, t, depth_scale=1000.0):
        """Depth frame [H,W] (uint16, float32 or float64) -> world points float64 [H*W,3] (ios_rtab.py:171-173,187-192)."""
        d = np.ascontiguousarray(depth)
        if d.ndim != 2:
            raise ValueError('depth must be [H,W]')
        if d.dtype == np.uint16:
            code = 2
        elif d.dtype == np.float32:
            code = 1
        else:
            d, code = np.ascontiguousarray(d, dtype=np.float64), 0
        K, q, t = _f64(K, (3, 3)), _f64(q_wxyz, (4,)), _f64(t, (3,))
        out = np.empty((d.size, 3), np.float64)
        self._check(self._lib.f3d_unproject_depth(self._h, _ptr(d), code, d.shape[0], d.shape[1], _ptr(K), float(depth_scale), _ptr(q), _ptr(t), _ptr(out)))
        return out

    def reserve_tsdf(self, nvoxels):
        """Size the scratch of tsdf_extract_count_dev / tsdf_extract_fill_dev for volumes of up to nvoxels voxels."""
        self._check(self._lib.f3d_ctx_reserve_tsdf(self._h, int(nvoxels)))

    def debug_tsdf_grid_cap(self, blocks):
        """Test hook: at most `blocks` blocks per grid-stride TSDF launch of this context (0 = the library's launch shapes)."""
        self._check(self._lib.f3d_debug_tsdf_grid_cap(self._h, int(blocks)))

    def debug_grid_cap(self, blocks):
        """Test hook: at most `blocks` blocks per grid-stride launch of the library (0 = the library's launch shapes), so that a small
        input takes many passes per block.  The state is per PROCESS, not per context: it holds for every context until it is set
        back to 0.  No result depends on it."""
        self._check(self._lib.f3d_debug_grid_cap(self._h, int(blocks)))

    def debug_grid_cap_stats(self):
        """Test hook: (grids sized while debug_grid_cap was on, grids it made smaller) since the last call; reading resets both.  The
        counters are per PROCESS, not per context.  No result depends on them."""
        out = np.zeros(2, np.int64)
        self._check(self._lib.f3d_debug_grid_cap_stats(self._h, _ptr(out)))
        return int(out[0]), int(out[1])

    def debug_poison(self, byte):
        """Test hook: fill every scratch, staging and kept buffer of this context, and the members that hold nothing between calls,
        with `byte` (0..255) -> (buffers filled, bytes filled).  Counted sequences end: their fill passes ask for the count pass.
        Refused while a view-chunked fused call is in progress.  No result of a later call depends on the byte."""
        out = np.zeros(2, np.int64)
        self._check(self._lib.f3d_debug_poison(self._h, int(byte), _ptr(out)))
        return int(out[0]), int(out[1])

    def tsdf_integrate(self, tsdf, weight, lo, voxel, trunc, max_weight, depths, views, depth_scale=1.0, max_depth=10.0):
        """Integrate depth frames [F, h, w] (uint16, float32 or float64) into the volume IN PLACE (f3d.h f3d_tsdf_integrate): tsdf and
        weight are C-contiguous float32 [nz, ny, nx] arrays, views the [F, 88] table of views_build."""
        nz, ny, nx = _tsdf_state(tsdf, weight)
        lo, d, code, views = _tsdf_frames(lo, depths, views)
        self._check(self._lib.f3d_tsdf_integrate(self._h, _ptr(tsdf), _ptr(weight), nx, ny, nz, _ptr(lo), float(voxel), float(trunc), float(max_weight),
                                                 _ptr(d), code, d.shape[0], d.shape[1], d.shape[2], float(depth_scale), float(max_depth), _ptr(views)))

    def tsdf_extract(self, tsdf, weight, lo, voxel, min_weight=1.0):
        """Surface-nets mesh of the volume (f3d.h f3d_tsdf_extract_count -> _fill) -> (vertices float64 [V, 3], triangles int32 [M, 3])."""
        nz, ny, nx = _tsdf_state(tsdf, weight)
        lo = _f64(lo, (3,))
        nv, nt = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.f3d_tsdf_extract_count(self._h, _ptr(tsdf), _ptr(weight), nx, ny, nz, float(min_weight), C.byref(nv), C.byref(nt)))
        verts, tris = np.empty((nv.value, 3), np.float64), np.empty((nt.value, 3), np.int32)
        self._check(self._lib.f3d_tsdf_extract_fill(self._h, nx, ny, nz, _ptr(lo), float(voxel), _ptr(verts), _ptr(tris)))
        return verts, tris

    def tsdf_integrate_color(self, tsdf, weight, color, lo, voxel, trunc, max_weight, depths, rgb, views, depth_scale=1.0, max_depth=10.0):
        """tsdf_integrate with colour (f3d.h f3d_tsdf_integrate_color): color is the C-contiguous float32 [nz, ny, nx, 4] state
        (r, g, b, wc), updated IN PLACE; rgb the uint8 [F, hc, wc, 3] colour images, one per depth frame, of any size."""
        nz, ny, nx = _tsdf_state(tsdf, weight)
        _tsdf_color(color, (nz, ny, nx))
        lo, d, code, views = _tsdf_frames(lo, depths, views)
        rgb = _tsdf_rgb(rgb, d.shape[0])
        self._check(self._lib.f3d_tsdf_integrate_color(self._h, _ptr(tsdf), _ptr(weight), _ptr(color), nx, ny, nz, _ptr(lo), float(voxel), float(trunc),
                                                       float(max_weight), _ptr(d), code, _ptr(rgb), d.shape[0], d.shape[1], d.shape[2], rgb.shape[1],
                                                       rgb.shape[2], float(depth_scale), float(max_depth), _ptr(views)))

    def tsdf_extract_colors(self, tsdf, weight, color, lo, voxel, min_weight=1.0):
        """tsdf_extract with vertex colours (f3d.h f3d_tsdf_extract_count -> _fill, _colors) -> (vertices float64 [V, 3], triangles
        int32 [M, 3], rgb uint8 [V, 3], colored uint8 [V]: 0 where no end of a crossing edge of the vertex's cell has a colour)."""
        nz, ny, nx = _tsdf_state(tsdf, weight)
        _tsdf_color(color, (nz, ny, nx), writeable=False)
        lo = _f64(lo, (3,))
        nv, nt = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.f3d_tsdf_extract_count(self._h, _ptr(tsdf), _ptr(weight), nx, ny, nz, float(min_weight), C.byref(nv), C.byref(nt)))
        verts, tris = np.empty((nv.value, 3), np.float64), np.empty((nt.value, 3), np.int32)
        rgb, colored = np.empty((nv.value, 3), np.uint8), np.empty(nv.value, np.uint8)
        self._check(self._lib.f3d_tsdf_extract_fill(self._h, nx, ny, nz, _ptr(lo), float(voxel), _ptr(verts), _ptr(tris)))
        self._check(self._lib.f3d_tsdf_extract_colors(self._h, _ptr(color), nx, ny, nz, _ptr(rgb), _ptr(colored)))
        return verts, tris, rgb, colored

    def reserve_icp(self, npixels):
        """Size the scratch of icp_sums_dev / icp_dev for source frames of up to npixels pixels."""
        self._check(self._lib.f3d_ctx_reserve_icp(self._h, int(npixels)))

    def tsdf_raycast(self, tsdf, weight, lo, voxel, min_weight, K, q_wxyz, t, h, w, near, step, nsteps):
        """Model maps of the volume from the camera->world pose (f3d.h f3d_tsdf_raycast) -> (vertex float64 [h*w, 3], normal float64
        [h*w, 3], depth float64 [h*w]); a pixel without a hit has NaN rows and depth 0."""
        nz, ny, nx = _tsdf_state(tsdf, weight)
        lo, K, q, t = _f64(lo, (3,)), _f64(K, (3, 3)), _f64(q_wxyz, (4,)), _f64(t, (3,))
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError('the image must have pixels')
        vertex, normal, depth = np.empty((h * w, 3)), np.empty((h * w, 3)), np.empty(h * w)
        self._check(self._lib.f3d_tsdf_raycast(self._h, _ptr(tsdf), _ptr(weight), nx, ny, nz, _ptr(lo), float(voxel), float(min_weight), _ptr(K),
                                               _ptr(q), _ptr(t), h, w, float(near), float(step), int(nsteps), _ptr(vertex), _ptr(normal),
                                               _ptr(depth)))
        return vertex, normal, depth

    def icp_sums(self, depth, K, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view, max_dist, depth_scale=1.0, max_depth=10.0):
        """The 29 sums of one point-to-plane linearisation (f3d.h f3d_icp_sums): depth [h, w] (uint16, float32 or float64) at the
        camera->world pose against the model maps float64 [hm*wm, 3] seen by model_view (one row of views_build) -> float64 [29]."""
        d, code, K, q, t, mv, mn, view = _icp_arrays(depth, K, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view)
        sums = np.empty(ICP_NSUMS)
        self._check(self._lib.f3d_icp_sums(self._h, _ptr(d), code, d.shape[0], d.shape[1], _ptr(K), float(depth_scale), float(max_depth), _ptr(q),
                                           _ptr(t), _ptr(mv), _ptr(mn), int(hm), int(wm), _ptr(view), float(max_dist), _ptr(sums)))
        return sums

    def icp(self, depth, K, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view, max_dist, depth_scale=1.0, max_depth=10.0, iterations=10,
            min_pairs=100):
        """`iterations` rounds of point-to-plane ICP on the device (f3d.h f3d_icp) -> (pose float64 [7] = wxyz, t; stats float64
        [iterations, 3] = count, sum r^2, status per round; the final status ICP_OK / ICP_LOST)."""
        d, code, K, q, t, mv, mn, view = _icp_arrays(depth, K, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view)
        iterations = int(iterations)
        if iterations < 1:
            raise ValueError(f'iterations must be at least 1, got {iterations}')
        pose, stats, status = np.empty(7), np.empty((iterations, 3)), C.c_int32(0)
        self._check(self._lib.f3d_icp(self._h, _ptr(d), code, d.shape[0], d.shape[1], _ptr(K), float(depth_scale), float(max_depth), _ptr(q), _ptr(t),
                                      _ptr(mv), _ptr(mn), int(hm), int(wm), _ptr(view), float(max_dist), iterations, int(min_pairs), _ptr(pose),
                                      _ptr(stats), C.byref(status)))
        return pose, stats, status.value

    def reserve_cloud_icp(self, m, n):
        """Size the scratch of the cloud_icp_sums_dev / cloud_icp_dev entries (f3d.clouds) for targets of up to m points and sources of
        up to n points, at any max_dist."""
        m, n = int(m), int(n)
        if not (0 <= m < 2 ** 31 and 0 <= n < 2 ** 31):
            raise ValueError(f'm and n must be in [0, 2^31), got {m} and {n}')
        self._check(self._lib.f3d_ctx_reserve_cloud_icp(self._h, m, n))

    def cloud_icp_sums(self, source, target, target_normals, mode, q_wxyz, t, max_dist, pairs=False):
        """The 29 sums of one linearisation of cloud-to-cloud ICP (f3d.h f3d_cloud_icp_sums): source [n, 3] at the pose (q_wxyz, t), which
        maps it into the frame of target [m, 3], each paired with its nearest target within max_dist; mode CLOUD_ICP_PLANE (against
        target_normals float64 [m, 3]) or CLOUD_ICP_POINT (target_normals is not read) -> float64 [29], and with pairs=True
        (sums, int32 [n]: the nearest target of every source point or -1)."""
        mode, q, t, max_dist = _cloud_icp_check(mode, target_normals is not None, q_wxyz, t, max_dist)
        s, sdt, g, gdt, nrm = _cloud_icp_arrays(source, target, target_normals, mode)
        sums = np.empty(ICP_NSUMS)
        out = np.empty(len(s), np.int32) if pairs else None
        self._check(self._lib.f3d_cloud_icp_sums(self._h, _ptr(s), sdt, len(s), _ptr(g), gdt, len(g), _ptr(nrm), mode, _ptr(q), _ptr(t), max_dist,
                                                 _ptr(sums), _ptr(out)))
        return (sums, out) if pairs else sums

    def cloud_icp(self, source, target, target_normals, mode, q_wxyz, t, max_dist, iterations=30, min_pairs=100):
        """`iterations` rounds of cloud-to-cloud ICP on the device (f3d.h f3d_cloud_icp), the target's grid built once -> (pose float64
        [7] = wxyz, t; stats float64 [iterations, 3] = count, sum r^2, status per round; the final status ICP_OK / ICP_LOST)."""
        mode, q, t, max_dist = _cloud_icp_check(mode, target_normals is not None, q_wxyz, t, max_dist, iterations, min_pairs)
        s, sdt, g, gdt, nrm = _cloud_icp_arrays(source, target, target_normals, mode)
        iterations = int(iterations)
        pose, stats, status = np.empty(7), np.empty((iterations, 3)), C.c_int32(0)
        self._check(self._lib.f3d_cloud_icp(self._h, _ptr(s), sdt, len(s), _ptr(g), gdt, len(g), _ptr(nrm), mode, _ptr(q), _ptr(t), max_dist,
                                            iterations, int(min_pairs), _ptr(pose), _ptr(stats), C.byref(status)))
        return pose, stats, status.value

    def reserve_icp_color(self, npixels):
        """Size the scratch of icp_color_sums_dev / icp_color_dev (58-wide chunk rows; it covers icp_sums_dev / icp_dev too) for source
        frames of up to npixels pixels."""
        self._check(self._lib.f3d_ctx_reserve_icp_color(self._h, int(npixels)))

    def tsdf_raycast_color(self, tsdf, weight, color, lo, voxel, min_weight, K, q_wxyz, t, h, w, near, step, nsteps):
        """tsdf_raycast with the volume's colour state float32 [nz, ny, nx, 4] (f3d.h f3d_tsdf_raycast_color) -> (vertex, normal, depth
        as tsdf_raycast gives them, rgb float64 [h*w, 3] on the 0..255 scale, intensity float64 [h*w]); NaN in the last two where a pixel
        has no hit or its hit has no colour."""
        nz, ny, nx = _tsdf_state(tsdf, weight)
        _tsdf_color(color, (nz, ny, nx), writeable=False)
        lo, K, q, t = _f64(lo, (3,)), _f64(K, (3, 3)), _f64(q_wxyz, (4,)), _f64(t, (3,))
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError('the image must have pixels')
        vertex, normal, depth = np.empty((h * w, 3)), np.empty((h * w, 3)), np.empty(h * w)
        rgb, intensity = np.empty((h * w, 3)), np.empty(h * w)
        self._check(self._lib.f3d_tsdf_raycast_color(self._h, _ptr(tsdf), _ptr(weight), _ptr(color), nx, ny, nz, _ptr(lo), float(voxel),
                                                     float(min_weight), _ptr(K), _ptr(q), _ptr(t), h, w, float(near), float(step), int(nsteps),
                                                     _ptr(vertex), _ptr(normal), _ptr(depth), _ptr(rgb), _ptr(intensity)))
        return vertex, normal, depth, rgb, intensity

    def icp_color_sums(self, depth, K, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view, max_dist, model_intensity, rgb, color_weight,
                       depth_scale=1.0, max_depth=10.0):
        """The 58 sums of one linearisation with colour (f3d.h f3d_icp_color_sums): the arguments of icp_sums plus the model's intensity
        map float64 [hm*wm] (NaN = missing), the source colour image uint8 [hc, wc, 3] and color_weight -> float64 [58]."""
        d, code, K, q, t, mv, mn, view = _icp_arrays(depth, K, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view)
        mi, rgb, color_weight = _icp_color_arrays(model_intensity, rgb, color_weight, hm, wm)
        sums = np.empty(ICP_NSUMS_COLOR)
        self._check(self._lib.f3d_icp_color_sums(self._h, _ptr(d), code, d.shape[0], d.shape[1], _ptr(K), float(depth_scale), float(max_depth), _ptr(q),
                                                 _ptr(t), _ptr(mv), _ptr(mn), int(hm), int(wm), _ptr(view), float(max_dist), _ptr(mi), _ptr(rgb),
                                                 rgb.shape[0], rgb.shape[1], color_weight, _ptr(sums)))
        return sums

    def icp_color(self, depth, K, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view, max_dist, model_intensity, rgb, color_weight,
                  depth_scale=1.0, max_depth=10.0, iterations=10, min_pairs=100):
        """`iterations` rounds of ICP with the photometric term (f3d.h f3d_icp_color) -> (pose float64 [7] = wxyz, t; stats float64
        [iterations, 5] = count, sum r^2, status, colour count, sum rc^2 per round; the final status ICP_OK / ICP_LOST)."""
        d, code, K, q, t, mv, mn, view = _icp_arrays(depth, K, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view)
        mi, rgb, color_weight = _icp_color_arrays(model_intensity, rgb, color_weight, hm, wm)
        iterations = int(iterations)
        if iterations < 1:
            raise ValueError(f'iterations must be at least 1, got {iterations}')
        pose, stats, status = np.empty(7), np.empty((iterations, 5)), C.c_int32(0)
        self._check(self._lib.f3d_icp_color(self._h, _ptr(d), code, d.shape[0], d.shape[1], _ptr(K), float(depth_scale), float(max_depth), _ptr(q),
                                            _ptr(t), _ptr(mv), _ptr(mn), int(hm), int(wm), _ptr(view), float(max_dist), _ptr(mi), _ptr(rgb),
                                            rgb.shape[0], rgb.shape[1], color_weight, iterations, int(min_pairs), _ptr(pose), _ptr(stats),
                                            C.byref(status)))
        return pose, stats, status.value

    def depth_half(self, depth, depth_scale=1.0, max_depth=10.0, gate=0.1):
        """One pyramid step of a depth frame [h, w] (f3d.h f3d_depth_half) -> float64 [h // 2, w // 2] in metres: the mean of each
        2 x 2 block's valid samples within `gate` of its nearest one, 0 where it has none."""
        d = np.ascontiguousarray(depth)
        gate = _half_check('depth', d.shape, gate)
        code = depth_code(d)
        out = np.empty((d.shape[0] // 2, d.shape[1] // 2))
        self._check(self._lib.f3d_depth_half(self._h, _ptr(d), code, d.shape[0], d.shape[1], float(depth_scale), float(max_depth), gate, _ptr(out)))
        return out

    def maps_half(self, model_vertex, model_normal, hm, wm, model_view, gate, model_intensity=None):
        """One pyramid step of model maps float64 [hm*wm, 3] seen by model_view (f3d.h f3d_maps_half) -> (vertex, normal float64
        [(hm // 2) * (wm // 2), 3]), and with model_intensity float64 [hm*wm] a third array, the intensity [(hm // 2) * (wm // 2)]."""
        hm, wm = int(hm), int(wm)
        gate = _half_check('the model image', (hm, wm), gate)
        mv, mn = _f64(model_vertex), _f64(model_normal)
        if mv.size != hm * wm * 3 or mn.size != hm * wm * 3:
            raise ValueError(f'the model maps must be [{hm} * {wm}, 3], got {mv.shape} and {mn.shape}')
        mi = None if model_intensity is None else _half_intensity(model_intensity, hm, wm)
        view = _f64(np.asarray(model_view).reshape(-1), (VIEW_DOUBLES,))
        n2 = (hm // 2) * (wm // 2)
        vertex, normal, intensity = np.empty((n2, 3)), np.empty((n2, 3)), None if mi is None else np.empty(n2)
        self._check(self._lib.f3d_maps_half(self._h, _ptr(mv), _ptr(mn), _ptr(mi), hm, wm, _ptr(view), gate, _ptr(vertex), _ptr(normal),
                                            _ptr(intensity)))
        return (vertex, normal) if mi is None else (vertex, normal, intensity)

    def icp_levels(self, levels, q_wxyz, t, max_depth=10.0, rgb=None, color_weight=None):
        """The rounds of icp / icp_color over `levels`, coarsest first, chained on the device (f3d.h f3d_icp_levels).  A level is a dict:
        depth [h, w], K, depth_scale (default 1), model_vertex, model_normal [hm*wm, 3], hm, wm, model_view, max_dist, iterations,
        min_pairs, and with colour model_intensity [hm*wm]; rgb uint8 [hc, wc, 3] and color_weight go with the intensity maps, all or
        none -> (pose float64 [7], stats float64 [sum of iterations, 3 or 5], the final status)."""
        levels = _icp_levels_check(levels, rgb, color_weight)
        q, t = _f64(q_wxyz, (4,)), _f64(t, (3,))
        keep, recs = [], (IcpLevel * len(levels))()
        for rec, lv in zip(recs, levels):
            d, code, K, _, _, mv, mn, view = _icp_arrays(lv['depth'], lv['K'], q, t, lv['model_vertex'], lv['model_normal'], lv['hm'], lv['wm'],
                                                         lv['model_view'])
            mi = None
            if rgb is not None:
                mi, rgb, color_weight = _icp_color_arrays(lv['model_intensity'], rgb, color_weight, lv['hm'], lv['wm'])
            keep += [d, mv, mn, view, mi]
            _fill_level(rec, d.ctypes.data, code, d.shape[0], d.shape[1], K, lv.get('depth_scale', 1.0), mv.ctypes.data, mn.ctypes.data,
                        None if mi is None else mi.ctypes.data, lv['hm'], lv['wm'], view.ctypes.data, lv['max_dist'], lv['iterations'], lv['min_pairs'])
        rounds = sum(int(lv['iterations']) for lv in levels)
        pose, stats, status = np.empty(7), np.empty((rounds, 3 if rgb is None else 5)), C.c_int32(0)
        hc, wc = (0, 0) if rgb is None else rgb.shape[:2]
        self._check(self._lib.f3d_icp_levels(self._h, C.byref(recs), len(levels), float(max_depth), _ptr(q), _ptr(t), _ptr(rgb), hc, wc,
                                             0.0 if rgb is None else color_weight, _ptr(pose), _ptr(stats), C.byref(status)))
        return pose, stats, status.value

    def radius_graph(self, points, radius):
        """KDTree(points).query_radius(points, r=radius) (fusion.py:374-375) as CSR: (offsets int64 [n+1], neighbours int32)."""
        p, dt = _xyz(points)
        offs = np.zeros(len(p) + 1, np.int64)
        nnz = C.c_int64(0)
        self._check(self._lib.f3d_radius_graph_count(self._h, _ptr(p), dt, len(p), float(radius), _ptr(offs), C.byref(nnz)))
        nb = np.empty(nnz.value, np.int32)
        self._check(self._lib.f3d_radius_graph_fill(self._h, len(p), _ptr(nb)))
        return offs, nb

    def radius_query(self, data, queries, radius):
        """KDTree(data).query_radius(queries, r=radius) inverted per query (correspondance.py:234-242) as CSR: (offsets int64 [n+1],
        neighbours int32); row q lists the data indices within radius of query q (inclusive) in ascending order."""
        d, ddt = _xyz(data)
        q, qdt = _xyz(queries)
        offs = np.zeros(len(q) + 1, np.int64)
        nnz = C.c_int64(0)
        self._check(self._lib.f3d_radius_query_count(self._h, _ptr(d), ddt, len(d), _ptr(q), qdt, len(q), float(radius), _ptr(offs),
                                                     C.byref(nnz)))
        nb = np.empty(nnz.value, np.int32)
        self._check(self._lib.f3d_radius_query_fill(self._h, len(q), _ptr(nb)))
        return offs, nb

    def knn_query(self, data, queries, k, radius):
        """At most k nearest data points within radius of every query (f3d.h f3d_knn_query) -> (idx int32 [n, k], dist2 float64
        [n, k], counts int32 [n]); a row is in (distance, index) order, padded with -1 / +inf."""
        k = _knn_k(k)
        d, ddt = _xyz(data)
        q, qdt = _xyz(queries)
        idx = np.empty((len(q), k), np.int32)
        dist2 = np.empty((len(q), k), np.float64)
        counts = np.empty(len(q), np.int32)
        self._check(self._lib.f3d_knn_query(self._h, _ptr(d), ddt, len(d), _ptr(q), qdt, len(q), k, float(radius), _ptr(idx), _ptr(dist2),
                                            _ptr(counts)))
        return idx, dist2, counts

    def transfer_labels(self, data, labels, queries, k, radius, fill=-1):
        """The plurality label of every query's knn_query row (f3d.h f3d_transfer_labels) -> (out int64 [n], support int32 [n]);
        a query without a neighbour gets (fill, 0).  labels: one integer per data point."""
        k = _knn_k(k)
        d, ddt = _xyz(data)
        q, qdt = _xyz(queries)
        lab = np.ascontiguousarray(labels, dtype=np.int64)
        if lab.shape != (len(d),):
            raise ValueError(f'labels must have one entry per data point ({len(d)}), got shape {lab.shape}')
        out = np.empty(len(q), np.int64)
        support = np.empty(len(q), np.int32)
        self._check(self._lib.f3d_transfer_labels(self._h, _ptr(d), ddt, len(d), _ptr(lab), _ptr(q), qdt, len(q), k, float(radius), int(fill),
                                                  _ptr(out), _ptr(support)))
        return out, support

    def estimate_normals(self, points, cam_centre, radius=0.05, max_nn=30, orient=True, want_neighbours=False):
        """Open3D's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) + the flip towards ``cam_centre`` of
        RTAB2Cache.surface_normal_estimation (ios_rtab.py:236-248), one frame: float64 [N,3] (f3d.h f3d_estimate_normals).
        want_neighbours: also (counts int32 [N], neighbours int32 [N, max_nn], -1 padded, in (distance, index) order)."""
        p = _n3(points, 'points must be [N,3], got {}')
        c = _f64(cam_centre, (3,)) if orient else None
        out = np.empty_like(p)
        counts = np.empty(len(p), np.int32) if want_neighbours else None
        nb = np.empty((len(p), max(int(max_nn), 0)), np.int32) if want_neighbours else None
        self._check(self._lib.f3d_estimate_normals(self._h, _ptr(p), len(p), _ptr(c), float(radius), int(max_nn), int(bool(orient)), _ptr(out),
                                                   _ptr(counts), _ptr(nb)))
        return (out, counts, nb) if want_neighbours else out

    # ---------------------------------------------------------------- device-pointer calls
    def project_vote_argmax_dev(self, xyz_ptr, dtype, n, views_ptr, nviews, masks_ptr, h, w, nclasses, threshold,
                                filter_classes, classes_ptr, votes_ptr=None, stream=None, flags=0, perm_ptr=None):
        f, nf = _filter(filter_classes)
        self._check(self._lib.f3d_project_vote_argmax_dev(self._h, xyz_ptr, dtype, n, views_ptr, nviews, masks_ptr, h, w,
                                                          int(nclasses), _ptr(f), nf, float(threshold), classes_ptr,
                                                          votes_ptr, int(flags), perm_ptr, stream))

    # the fused path with the views arriving in chunks (f3d.h: f3d_mask_presence_dev .. f3d_fuse_chunk_dev)
    def mask_presence_dev(self, masks_ptr, nviews, h, w, present256_ptr, stream=None):
        self._check(self._lib.f3d_mask_presence_dev(self._h, masks_ptr, nviews, h, w, present256_ptr, stream))

    def fuse_chunked_begin_dev(self, present256_ptr, n, nviews, h, w, nclasses, filter_classes, stream=None):
        f, nf = _filter(filter_classes)
        self._check(self._lib.f3d_fuse_chunked_begin_dev(self._h, present256_ptr, n, nviews, h, w, int(nclasses), _ptr(f), nf, stream))

    def fuse_chunk_dev(self, xyz_ptr, dtype, n, views_ptr, nviews, v_begin, v_end, masks_ptr, h, w, nclasses, threshold,
                       filter_classes, classes_ptr, stream=None, flags=0, perm_ptr=None):
        f, nf = _filter(filter_classes)
        self._check(self._lib.f3d_fuse_chunk_dev(self._h, xyz_ptr, dtype, n, views_ptr, nviews, int(v_begin), int(v_end), masks_ptr, h, w,
                                                 int(nclasses), _ptr(f), nf, float(threshold), classes_ptr, int(flags), perm_ptr, stream))

    def coded_plane_bytes(self, h, w):
        return int(self._lib.f3d_coded_plane_bytes(int(h), int(w)))

    def code_planes_dev(self, masks_ptr, nplanes, h, w, coded_ptr, stream=None):
        self._check(self._lib.f3d_code_planes_dev(self._h, masks_ptr, int(nplanes), int(h), int(w), coded_ptr, stream))

    def fuse_chunk_coded_dev(self, xyz_ptr, dtype, n, views_ptr, nviews, v_begin, v_end, coded_ptr, h, w, nclasses, threshold,
                             filter_classes, classes_ptr, stream=None, flags=0, perm_ptr=None):
        f, nf = _filter(filter_classes)
        self._check(self._lib.f3d_fuse_chunk_coded_dev(self._h, xyz_ptr, dtype, n, views_ptr, nviews, int(v_begin), int(v_end), coded_ptr, h, w,
                                                       int(nclasses), _ptr(f), nf, float(threshold), classes_ptr, int(flags), perm_ptr, stream))

    def radius_query_dev(self, data_ptr, data_dtype, m, queries_ptr, query_dtype, n, radius, offsets_ptr, stream=None):
        """Count pass of radius_query on device pointers: offsets int64 [n+1] on the device; -> nnz (one blocking readback)."""
        nnz = C.c_int64(0)
        self._check(self._lib.f3d_radius_query_count_dev(self._h, data_ptr, int(data_dtype), int(m), queries_ptr, int(query_dtype), int(n),
                                                         float(radius), offsets_ptr, C.byref(nnz), stream))
        return nnz.value

    def radius_query_fill_dev(self, queries_ptr, query_dtype, n, offsets_ptr, neighbours_ptr, stream=None):
        """Fill pass after radius_query_dev of the same queries: neighbours int32 [nnz] on the device (enqueue only)."""
        self._check(self._lib.f3d_radius_query_fill_dev(self._h, queries_ptr, int(query_dtype), int(n), offsets_ptr, neighbours_ptr, stream))

    def knn_query_dev(self, data_ptr, data_dtype, m, queries_ptr, query_dtype, n, k, radius, idx_ptr, dist2_ptr=None, counts_ptr=None,
                      stream=None):
        """knn_query on device pointers: idx int32 [n, k], dist2 float64 [n, k] and counts int32 [n] on the device (the last two
        may be None); enqueues after one blocking readback."""
        k = _knn_k(k)
        self._check(self._lib.f3d_knn_query_dev(self._h, data_ptr, int(data_dtype), int(m), queries_ptr, int(query_dtype), int(n), k,
                                                float(radius), idx_ptr, dist2_ptr, counts_ptr, stream))

    def transfer_labels_dev(self, data_ptr, data_dtype, m, labels_ptr, queries_ptr, query_dtype, n, k, radius, fill, out_ptr,
                            support_ptr=None, stream=None):
        """transfer_labels on device pointers: labels int64 [m], out int64 [n], support int32 [n] (may be None) on the device;
        enqueues after one blocking readback."""
        k = _knn_k(k)
        self._check(self._lib.f3d_transfer_labels_dev(self._h, data_ptr, int(data_dtype), int(m), labels_ptr, queries_ptr, int(query_dtype),
                                                      int(n), k, float(radius), int(fill), out_ptr, support_ptr, stream))

    def rotate_dev(self, xyz_ptr, n, q_wxyz, out_ptr, stream=None):
        q = _f64(q_wxyz, (4,))
        self._check(self._lib.f3d_rotate_f64_dev(self._h, xyz_ptr, n, _ptr(q), out_ptr, stream))

    def cloud_sort_cells_dev(self, xyz_ptr, dtype, n, sorted_ptr, perm_ptr, stream=None):
        self._check(self._lib.f3d_cloud_sort_cells_dev(self._h, xyz_ptr, dtype, n, sorted_ptr, perm_ptr, stream))

    def fastpath_audit(self, points, views, w=1024, h=1024):
        """(pairs inside, pairs left to the exact kernel, decided-but-different pairs, contradicted culls) on the cell-sorted cloud."""
        p, dt = _xyz(points)
        v = _f64(views)
        stats = np.zeros(4, np.uint64)
        self._check(self._lib.f3d_debug_fastpath_audit(self._h, _ptr(p), dt, len(p), _ptr(v), len(v), int(w), int(h), _ptr(stats)))
        return tuple(int(x) for x in stats)

    def fuse_deferred(self, stream=None):
        """(points the float32 kernel deferred to the float64 tier, points of those that needed the reference's own arithmetic) of the last fused call."""
        c = np.zeros(2, np.uint32)
        self._check(self._lib.f3d_debug_fuse_deferred(self._h, stream, _ptr(c)))
        return int(c[0]), int(c[1])

    def fuse_decided(self, stream=None):
        """Wave-tiles (128 points) of the last fused call that left their view loops early: every point already decided "unlabelled"."""
        c = np.zeros(1, np.uint32)
        self._check(self._lib.f3d_debug_fuse_decided(self._h, stream, _ptr(c)))
        return int(c[0])

    def flood_order_dev(self, classes_ptr, n, offsets_ptr, neighbours_ptr, instance_classes, root_ptr, order_ptr, coffs_ptr, flags_ptr,
                        stream=None):
        """f3d_flood_order_dev: device buffers root/order int64 [n], coffs int64 [n + 1], flags uint8 [n]; synchronises `stream`
        (the frontier length is read back every few levels).  -> stats dict (clusters, points, levels, readbacks)."""
        inst = np.ascontiguousarray(np.asarray(instance_classes).reshape(-1), dtype=np.int64)
        stats = np.zeros(4, np.int64)
        self._check(self._lib.f3d_flood_order_dev(self._h, classes_ptr, int(n), offsets_ptr, neighbours_ptr, _ptr(inst), len(inst), root_ptr,
                                                  order_ptr, coffs_ptr, flags_ptr, _ptr(stats), stream))
        return _flood_stats(stats)

    def color_segment_dev(self, colors_ptr, dtype, n, offsets_ptr, neighbours_ptr, ids_ptr, seeds_ptr, nseeds, threshold, neutral_ids=(0,),
                          max_level=10, accepted_ptr=None, stream=None):
        """f3d_color_segment_dev: enqueue only; an index error is recorded for take_device_error."""
        thr = _threshold3(threshold)
        neu = np.ascontiguousarray(np.asarray(list(neutral_ids)).reshape(-1), dtype=np.int64)
        self._check(self._lib.f3d_color_segment_dev(self._h, colors_ptr, int(dtype), int(n), offsets_ptr, neighbours_ptr, ids_ptr, seeds_ptr,
                                                    int(nseeds), _ptr(thr), _ptr(neu), len(neu), int(max_level), accepted_ptr, stream))

    def region_grow_dev(self, values_ptr, dtype, nchan, n, offsets_ptr, neighbours_ptr, seeds_ptr, nseeds, sma0, npts0, threshold, max_level,
                        cluster_ptr, count_ptr, seeds_given=False, stream=None):
        """f3d_region_grow_dev: cluster int64 [n] and count int64 [1] on the device; enqueue only; an index error is recorded for
        take_device_error."""
        sma, thr = _grow_params(int(nchan), sma0, threshold)
        self._check(self._lib.f3d_region_grow_dev(self._h, values_ptr, int(dtype), int(nchan), int(n), offsets_ptr, neighbours_ptr, seeds_ptr,
                                                  int(nseeds), _ptr(sma), int(npts0), int(bool(seeds_given)), _ptr(thr), int(max_level),
                                                  cluster_ptr, count_ptr, stream))

    def plane_distance_dev(self, points_ptr, n, plane_point, normal, out_ptr, stream=None):
        """f3d_plane_distance_dev: float64 points [n, 3] and out [n] on the device; enqueue only."""
        pp, nr = _f64(np.asarray(plane_point).reshape(-1), (3,)), _f64(np.asarray(normal).reshape(-1), (3,))
        self._check(self._lib.f3d_plane_distance_dev(self._h, points_ptr, int(n), _ptr(pp), _ptr(nr), out_ptr, stream))

    def door_window_quads_dev(self, points_ptr, n, ids_ptr, instance_ids_ptr, k, vertices_ptr, nvertices, triangles_ptr, ntriangles, quads_ptr,
                              status_ptr, tri_ptr, normals_ptr=None, stream=None):
        """f3d_door_window_quads_dev: float64 points / vertices, int64 ids / instance ids / triangles, all on the device; enqueue only
        (a bad vertex index is recorded for take_device_error)."""
        self._check(self._lib.f3d_door_window_quads_dev(self._h, points_ptr, int(n), ids_ptr, instance_ids_ptr, int(k), vertices_ptr,
                                                        int(nvertices), triangles_ptr, int(ntriangles), quads_ptr, status_ptr, tri_ptr,
                                                        normals_ptr, stream))

    # f3d_mesh_*_dev: device pointers throughout (counts int64 [4] too); itype I64 / I32, vdtype F64 / F32; enqueue only.  An index
    # outside [0, V) sets counts[2], writes nothing else and is recorded for take_device_error
    def mesh_vertex_map_dev(self, tris_ptr, itype, nt, nv, offsets_ptr, tri_ptr, pos_ptr, counts_ptr, stream=None):
        self._check(self._lib.f3d_mesh_vertex_map_dev(self._h, tris_ptr, itype, int(nt), int(nv), offsets_ptr, tri_ptr, pos_ptr, counts_ptr, stream))

    def mesh_remove_faces_dev(self, tris_ptr, itype, nt, nv, mask_ptr, not_removed_ptr, remaining_ptr, old2new_ptr, counts_ptr, stream=None):
        self._check(self._lib.f3d_mesh_remove_faces_dev(self._h, tris_ptr, itype, int(nt), int(nv), mask_ptr, not_removed_ptr, remaining_ptr,
                                                        old2new_ptr, counts_ptr, stream))

    def mesh_keep_faces_dev(self, verts_ptr, vdtype, nv, tris_ptr, itype, nt, mask_ptr, out_verts_ptr, out_tris_ptr, counts_ptr, stream=None):
        self._check(self._lib.f3d_mesh_keep_faces_dev(self._h, verts_ptr, vdtype, int(nv), tris_ptr, itype, int(nt), mask_ptr, out_verts_ptr,
                                                      out_tris_ptr, counts_ptr, stream))

    def mesh_triangle_clusters_dev(self, verts_ptr, vdtype, nv, tris_ptr, itype, nt, clusters_ptr, cluster_n_ptr, cluster_area_ptr, tri_area_ptr,
                                   counts_ptr, stream=None):
        self._check(self._lib.f3d_mesh_triangle_clusters_dev(self._h, verts_ptr, vdtype, int(nv), tris_ptr, itype, int(nt), clusters_ptr,
                                                             cluster_n_ptr, cluster_area_ptr, tri_area_ptr, counts_ptr, stream))

    def mesh_clean_dev(self, verts_ptr, vdtype, nv, tris_ptr, itype, nt, remove_mask_ptr, min_triangles, min_area, new_verts_ptr, new_tris_ptr,
                       kept_v_ptr, kept_t_ptr, counts_ptr, stream=None):
        self._check(self._lib.f3d_mesh_clean_dev(self._h, verts_ptr, vdtype, int(nv), tris_ptr, itype, int(nt), remove_mask_ptr, int(min_triangles),
                                                 float(min_area), new_verts_ptr, new_tris_ptr, kept_v_ptr, kept_t_ptr, counts_ptr, stream))

    def mesh_face_frames_dev(self, verts_ptr, vdtype, nv, tris_ptr, itype, nt, normals_ptr, centroids_ptr, areas_ptr, counts_ptr, stream=None):
        """f3d_mesh_face_frames_dev: centroids_ptr / areas_ptr may be None."""
        self._check(self._lib.f3d_mesh_face_frames_dev(self._h, verts_ptr, vdtype, int(nv), tris_ptr, itype, int(nt), normals_ptr, centroids_ptr,
                                                       areas_ptr, counts_ptr, stream))

    def mesh_face_graph_dev(self, verts_ptr, vdtype, nv, tris_ptr, itype, nt, gate, cos_crease, offsets_ptr, neighbours_ptr, cap, counts_ptr,
                            stream=None):
        """f3d_mesh_face_graph_dev: verts_ptr may be None without a gate; neighbours (cap entries) is written only when counts[0] <= cap."""
        self._check(self._lib.f3d_mesh_face_graph_dev(self._h, verts_ptr, vdtype, int(nv), tris_ptr, itype, int(nt), int(gate), float(cos_crease),
                                                      offsets_ptr, neighbours_ptr, int(cap), counts_ptr, stream))

    def extract_planes_dev(self, xyz_ptr, dtype, n, offsets_ptr, neighbours_ptr, normals_ptr, cos_angle, offset, dist, max_variation,
                           min_points, max_rounds, max_planes, labels_ptr, planes_ptr, corners_ptr, counts_ptr, normals_out_ptr=None,
                           stream=None):
        """f3d_extract_planes_dev: device pointers throughout (counts int64 [4] too; normals_ptr / normals_out_ptr may be None).
        Enqueues on `stream` and synchronises it every few attach rounds; a neighbour index outside [0, n) is recorded for
        take_device_error."""
        self._check(self._lib.f3d_extract_planes_dev(self._h, xyz_ptr, int(dtype), int(n), offsets_ptr, neighbours_ptr, normals_ptr,
                                                     float(cos_angle), float(offset), float(dist), float(max_variation), int(min_points),
                                                     int(max_rounds), int(max_planes), labels_ptr, planes_ptr, corners_ptr, counts_ptr,
                                                     normals_out_ptr, stream))

    def smooth_votes_dev(self, votes_ptr, vtype, n, ncols, offsets_ptr, neighbours_ptr, normals_ptr, cos_angle, colors_ptr, cdtype,
                         max_color_dist, self_weight, iterations, votes_out_ptr, stream=None):
        """f3d_smooth_votes_dev: device pointers throughout (normals_ptr / colors_ptr may be None: no gate); votes_out float64
        [n, ncols] must not overlap votes.  A bad neighbour index is recorded for take_device_error and nothing is written."""
        self._check(self._lib.f3d_smooth_votes_dev(self._h, votes_ptr, int(vtype), int(n), int(ncols), offsets_ptr, neighbours_ptr,
                                                   normals_ptr, float(cos_angle), colors_ptr, int(cdtype), float(max_color_dist),
                                                   float(self_weight), int(iterations), votes_out_ptr, stream))

    def smooth_segment_dev(self, votes_ptr, vtype, n, ncols, offsets_ptr, neighbours_ptr, normals_ptr, cos_angle, colors_ptr, cdtype,
                           max_color_dist, self_weight, iterations, nclasses, threshold, filter_classes, lastcol, classes_ptr, stream=None):
        """f3d_smooth_segment_dev: device pointers (filter_classes stays a host list); classes int64 [n]."""
        f, nf = _filter(filter_classes)
        self._check(self._lib.f3d_smooth_segment_dev(self._h, votes_ptr, int(vtype), int(n), int(ncols), offsets_ptr, neighbours_ptr,
                                                     normals_ptr, float(cos_angle), colors_ptr, int(cdtype), float(max_color_dist),
                                                     float(self_weight), int(iterations), int(nclasses), float(threshold), _ptr(f), nf,
                                                     int(bool(lastcol)), classes_ptr, stream))

    def lift_overlaps_dev(self, luts_ptr, inst_ptr, nframes, hw, npoints, max_ids, sizes_ptr, pairs_ptr, counts_ptr, cap, stream=None):
        """f3d_lift_overlaps_dev: device pointers; synchronises `stream` for its one readback -> stats int64 [6] (host).  pairs / counts
        (cap entries) are written only when stats[0] <= cap.  Bad input raises IndexError and nothing is written."""
        stats = np.zeros(6, np.int64)
        self._check(self._lib.f3d_lift_overlaps_dev(self._h, luts_ptr, inst_ptr, int(nframes), int(hw), int(npoints), int(max_ids), sizes_ptr,
                                                    pairs_ptr, counts_ptr, int(cap), _ptr(stats), stream))
        return stats

    def lift_instances_dev(self, luts_ptr, inst_ptr, nframes, hw, npoints, max_ids, ratio, min_overlap, seg_classes_ptr, min_points, ids_ptr,
                           support_ptr, seen_ptr, seg2inst_ptr, inst_points_ptr, stream=None):
        """f3d_lift_instances_dev: device pointers (seg_classes_ptr may be None; inst_points int64 [F * max_ids + 1]); synchronises
        `stream` for its one readback -> stats int64 [6] (host).  Bad input raises IndexError and nothing is written."""
        stats = np.zeros(6, np.int64)
        self._check(self._lib.f3d_lift_instances_dev(self._h, luts_ptr, inst_ptr, int(nframes), int(hw), int(npoints), int(max_ids), float(ratio),
                                                     int(min_overlap), seg_classes_ptr, int(min_points), ids_ptr, support_ptr, seen_ptr,
                                                     seg2inst_ptr, inst_points_ptr, _ptr(stats), stream))
        return stats

    def tsdf_integrate_dev(self, tsdf_ptr, weight_ptr, dims, lo, voxel, trunc, max_weight, depth_ptr, depth_type, nframes, h, w, depth_scale,
                           max_depth, views_ptr, stream=None):
        """dims = (nx, ny, nz); lo on the host; everything else device pointers (f3d.h f3d_tsdf_integrate_dev).  Enqueue only."""
        lo = _f64(lo, (3,))
        nx, ny, nz = (int(x) for x in dims)
        self._check(self._lib.f3d_tsdf_integrate_dev(self._h, tsdf_ptr, weight_ptr, nx, ny, nz, _ptr(lo), float(voxel), float(trunc), float(max_weight),
                                                     depth_ptr, int(depth_type), int(nframes), int(h), int(w), float(depth_scale), float(max_depth),
                                                     views_ptr, stream))

    def tsdf_extract_count_dev(self, tsdf_ptr, weight_ptr, dims, min_weight=1.0, stream=None):
        """-> (nv, nt) of the volume's mesh; the ranks stay in the context for tsdf_extract_fill_dev.  Synchronises `stream` once."""
        nx, ny, nz = (int(x) for x in dims)
        nv, nt = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.f3d_tsdf_extract_count_dev(self._h, tsdf_ptr, weight_ptr, nx, ny, nz, float(min_weight), C.byref(nv), C.byref(nt), stream))
        return nv.value, nt.value

    def tsdf_extract_fill_dev(self, tsdf_ptr, dims, lo, voxel, verts_ptr, tris_ptr, stream=None):
        lo = _f64(lo, (3,))
        nx, ny, nz = (int(x) for x in dims)
        self._check(self._lib.f3d_tsdf_extract_fill_dev(self._h, tsdf_ptr, nx, ny, nz, _ptr(lo), float(voxel), verts_ptr, tris_ptr, stream))

    def tsdf_integrate_color_dev(self, tsdf_ptr, weight_ptr, color_ptr, dims, lo, voxel, trunc, max_weight, depth_ptr, depth_type, rgb_ptr, nframes,
                                 h, w, hc, wc, depth_scale, max_depth, views_ptr, stream=None):
        """tsdf_integrate_dev with the colour state [nz, ny, nx, 4] (16-byte aligned) and the colour images uint8 [F, hc, wc, 3], device
        pointers both (f3d.h f3d_tsdf_integrate_color_dev).  Enqueue only."""
        lo = _f64(lo, (3,))
        nx, ny, nz = (int(x) for x in dims)
        self._check(self._lib.f3d_tsdf_integrate_color_dev(self._h, tsdf_ptr, weight_ptr, color_ptr, nx, ny, nz, _ptr(lo), float(voxel), float(trunc),
                                                           float(max_weight), depth_ptr, int(depth_type), rgb_ptr, int(nframes), int(h), int(w),
                                                           int(hc), int(wc), float(depth_scale), float(max_depth), views_ptr, stream))

    def tsdf_extract_colors_dev(self, tsdf_ptr, color_ptr, dims, rgb_ptr, colored_ptr=None, stream=None):
        """Vertex colours of the volume counted last: rgb uint8 [nv, 3], colored uint8 [nv] or None (f3d.h f3d_tsdf_extract_colors_dev).
        Enqueue only."""
        nx, ny, nz = (int(x) for x in dims)
        self._check(self._lib.f3d_tsdf_extract_colors_dev(self._h, tsdf_ptr, color_ptr, nx, ny, nz, rgb_ptr, colored_ptr, stream))

    def tsdf_raycast_dev(self, tsdf_ptr, weight_ptr, dims, lo, voxel, min_weight, K, q_wxyz, t, h, w, near, step, nsteps, vertex_ptr, normal_ptr,
                         depth_ptr, stream=None):
        """dims = (nx, ny, nz); lo, K and the pose on the host; the state and the three outputs (each may be None) device pointers
        (f3d.h f3d_tsdf_raycast_dev).  Enqueue only."""
        lo, K, q, t = _f64(lo, (3,)), _f64(K, (3, 3)), _f64(q_wxyz, (4,)), _f64(t, (3,))
        nx, ny, nz = (int(x) for x in dims)
        self._check(self._lib.f3d_tsdf_raycast_dev(self._h, tsdf_ptr, weight_ptr, nx, ny, nz, _ptr(lo), float(voxel), float(min_weight), _ptr(K),
                                                   _ptr(q), _ptr(t), int(h), int(w), float(near), float(step), int(nsteps), vertex_ptr, normal_ptr,
                                                   depth_ptr, stream))

    def icp_sums_dev(self, depth_ptr, depth_type, h, w, K, q_wxyz, t, vertex_ptr, normal_ptr, hm, wm, view_ptr, max_dist, depth_scale, max_depth,
                     sums_ptr, stream=None):
        """K and the source pose on the host, everything else device pointers (view_ptr: one f3d_view); sums float64 [29].  Enqueue only."""
        K, q, t = _f64(K, (3, 3)), _f64(q_wxyz, (4,)), _f64(t, (3,))
        self._check(self._lib.f3d_icp_sums_dev(self._h, depth_ptr, int(depth_type), int(h), int(w), _ptr(K), float(depth_scale), float(max_depth),
                                               _ptr(q), _ptr(t), vertex_ptr, normal_ptr, int(hm), int(wm), view_ptr, float(max_dist), sums_ptr, stream))

    def icp_dev(self, depth_ptr, depth_type, h, w, K, q_wxyz, t, vertex_ptr, normal_ptr, hm, wm, view_ptr, max_dist, depth_scale, max_depth,
                iterations, min_pairs, pose_ptr, stats_ptr, status_ptr=None, stream=None):
        """As icp_sums_dev; pose float64 [7], stats float64 [iterations, 3] and status int32 [1] (may be None) on the device.  Enqueue
        only: no host synchronisation between the rounds or after them."""
        K, q, t = _f64(K, (3, 3)), _f64(q_wxyz, (4,)), _f64(t, (3,))
        self._check(self._lib.f3d_icp_dev(self._h, depth_ptr, int(depth_type), int(h), int(w), _ptr(K), float(depth_scale), float(max_depth), _ptr(q),
                                          _ptr(t), vertex_ptr, normal_ptr, int(hm), int(wm), view_ptr, float(max_dist), int(iterations),
                                          int(min_pairs), pose_ptr, stats_ptr, status_ptr, stream))

    def tsdf_raycast_color_dev(self, tsdf_ptr, weight_ptr, color_ptr, dims, lo, voxel, min_weight, K, q_wxyz, t, h, w, near, step, nsteps, vertex_ptr,
                               normal_ptr, depth_ptr, rgb_ptr, intensity_ptr, stream=None):
        """tsdf_raycast_dev with the colour state [nz, ny, nx, 4] (16-byte aligned) and two more outputs, rgb float64 [h*w, 3] and intensity
        float64 [h*w]; each of the five may be None (f3d.h f3d_tsdf_raycast_color_dev).  Enqueue only."""
        lo, K, q, t = _f64(lo, (3,)), _f64(K, (3, 3)), _f64(q_wxyz, (4,)), _f64(t, (3,))
        nx, ny, nz = (int(x) for x in dims)
        self._check(self._lib.f3d_tsdf_raycast_color_dev(self._h, tsdf_ptr, weight_ptr, color_ptr, nx, ny, nz, _ptr(lo), float(voxel), float(min_weight),
                                                         _ptr(K), _ptr(q), _ptr(t), int(h), int(w), float(near), float(step), int(nsteps), vertex_ptr,
                                                         normal_ptr, depth_ptr, rgb_ptr, intensity_ptr, stream))

    def icp_color_sums_dev(self, depth_ptr, depth_type, h, w, K, q_wxyz, t, vertex_ptr, normal_ptr, hm, wm, view_ptr, max_dist, intensity_ptr, rgb_ptr,
                           hc, wc, color_weight, depth_scale, max_depth, sums_ptr, stream=None):
        """As icp_sums_dev, plus the model's intensity map float64 [hm*wm] and the source colour image uint8 [hc, wc, 3] on the device;
        sums float64 [58].  Enqueue only."""
        K, q, t = _f64(K, (3, 3)), _f64(q_wxyz, (4,)), _f64(t, (3,))
        self._check(self._lib.f3d_icp_color_sums_dev(self._h, depth_ptr, int(depth_type), int(h), int(w), _ptr(K), float(depth_scale), float(max_depth),
                                                     _ptr(q), _ptr(t), vertex_ptr, normal_ptr, int(hm), int(wm), view_ptr, float(max_dist), intensity_ptr,
                                                     rgb_ptr, int(hc), int(wc), float(color_weight), sums_ptr, stream))

    def icp_color_dev(self, depth_ptr, depth_type, h, w, K, q_wxyz, t, vertex_ptr, normal_ptr, hm, wm, view_ptr, max_dist, intensity_ptr, rgb_ptr, hc, wc,
                      color_weight, depth_scale, max_depth, iterations, min_pairs, pose_ptr, stats_ptr, status_ptr=None, stream=None):
        """As icp_color_sums_dev; pose float64 [7], stats float64 [iterations, 5] and status int32 [1] (may be None) on the device.  Enqueue
        only: no host synchronisation between the rounds or after them."""
        K, q, t = _f64(K, (3, 3)), _f64(q_wxyz, (4,)), _f64(t, (3,))
        self._check(self._lib.f3d_icp_color_dev(self._h, depth_ptr, int(depth_type), int(h), int(w), _ptr(K), float(depth_scale), float(max_depth),
                                                _ptr(q), _ptr(t), vertex_ptr, normal_ptr, int(hm), int(wm), view_ptr, float(max_dist), intensity_ptr,
                                                rgb_ptr, int(hc), int(wc), float(color_weight), int(iterations), int(min_pairs), pose_ptr, stats_ptr,
                                                status_ptr, stream))

    def take_device_error(self, stream=None):
        self._check(self._lib.f3d_take_device_error(self._h, stream))

    def project_view_dev(self, xyz_ptr, dtype, n, view, uv_ptr, inside_ptr, stream=None):
        v = _f64(view, (VIEW_DOUBLES,))
        self._check(self._lib.f3d_project_view_dev(self._h, xyz_ptr, dtype, n, _ptr(v), uv_ptr, inside_ptr, stream))

    def segment_votes_dev(self, votes_ptr, npts, ncols, nclasses, threshold, filter_classes, classes_ptr, stream=None):
        f, nf = _filter(filter_classes)
        self._check(self._lib.f3d_segment_votes_dev(self._h, votes_ptr, npts, ncols, int(nclasses), float(threshold),
                                                    _ptr(f), nf, classes_ptr, stream))

    def segment_votes_lastcol_dev(self, votes_ptr, npts, ncols, nclasses, threshold, filter_classes, classes_ptr, stream=None):
        f, nf = _filter(filter_classes)
        self._check(self._lib.f3d_segment_votes_lastcol_dev(self._h, votes_ptr, npts, ncols, int(nclasses), float(threshold),
                                                            _ptr(f), nf, classes_ptr, stream))

    def point_vote_frames_dev(self, cloud_ptr, cloud_dtype, m, queries_ptr, query_dtype, masks_ptr, nframes, hw, radius, votes_ptr, ncols,
                              stream=None):
        """Enqueues on `stream` after one readback (f3d.h); a label > nclasses on a pixel with a neighbour is recorded for
        take_device_error, non-finite queries raise ValueError here after the frames before them are enqueued."""
        self._check(self._lib.f3d_point_vote_frames_dev(self._h, cloud_ptr, int(cloud_dtype), int(m), queries_ptr, int(query_dtype), masks_ptr,
                                                        int(nframes), int(hw), float(radius), votes_ptr, int(ncols), stream))

    def render_lookups_dev(self, xyz_ptr, dtype, n, views_ptr, nviews, h, w, splat, depth_ptr, uv2pt_ptr, stream=None):
        """depth_ptr float32 [V, h, w] and uv2pt_ptr int32 [V, h*w] on the device, either may be None; enqueue only."""
        self._check(self._lib.f3d_render_lookups_dev(self._h, xyz_ptr, int(dtype), int(n), views_ptr, int(nviews), int(h), int(w), int(splat),
                                                     depth_ptr, uv2pt_ptr, stream))

    def vote_visible_dev(self, xyz_ptr, dtype, n, views_ptr, nviews, masks_ptr, h, w, splat, depth_tol, votes_ptr, ncols, views_per_pass=0,
                         stream=None):
        """Enqueue only; a label >= ncols on a visible sample is recorded for take_device_error."""
        self._check(self._lib.f3d_vote_visible_dev(self._h, xyz_ptr, int(dtype), int(n), views_ptr, int(nviews), masks_ptr, int(h), int(w),
                                                   int(splat), float(depth_tol), votes_ptr, int(ncols), int(views_per_pass), stream))

    def fuse_features_dev(self, xyz_ptr, dtype, n, views_ptr, nviews, h, w, feats_ptr, ftype, hf, wf, d, splat, depth_tol, sums_ptr, counts_ptr,
                          views_per_pass=0, stream=None):
        """Enqueue only (f3d.h f3d_fuse_features_dev): feats [V, hf, wf, d] of FEAT_F16 / FEAT_F32, sums float32 [n, d] and counts int32 [n]
        updated in place.  Scratch: reserve_render(n, nviews, h, w); none with depth_tol = inf."""
        self._check(self._lib.f3d_fuse_features_dev(self._h, xyz_ptr, int(dtype), int(n), views_ptr, int(nviews), int(h), int(w), feats_ptr,
                                                    int(ftype), int(hf), int(wf), int(d), int(splat), float(depth_tol), sums_ptr, counts_ptr,
                                                    int(views_per_pass), stream))

    def features_finalize_dev(self, sums_ptr, counts_ptr, n, d, normalize, out_ptr, stream=None):
        """Enqueue only (f3d.h f3d_features_finalize_dev); out_ptr may be sums_ptr."""
        self._check(self._lib.f3d_features_finalize_dev(self._h, sums_ptr, counts_ptr, int(n), int(d), int(bool(normalize)), out_ptr, stream))

    def render_counts_dev(self, xyz_ptr, dtype, n, views_ptr, nviews, h, w, splat, stream=None):
        """Diagnostic (synchronises): samples, covered cells and issued atomics of a render of these views, and the device-event times
        of the key fill and of the (counting) splat kernel (f3d.h f3d_debug_render_counts)."""
        counts, ms = np.zeros(3, np.uint64), np.zeros(2)
        self._check(self._lib.f3d_debug_render_counts(self._h, xyz_ptr, int(dtype), int(n), views_ptr, int(nviews), int(h), int(w), int(splat),
                                                      _ptr(counts), _ptr(ms), stream))
        return {'samples': int(counts[0]), 'cells': int(counts[1]), 'atomics': int(counts[2]), 'fill_ms': float(ms[0]), 'splat_ms': float(ms[1])}

    # mesh z-buffer (f3d.h "triangle-mesh z-buffer renders"): verts / tris as for the mesh entries (vdtype F64 / F32, itype I64 / I32)
    def render_mesh_lookups_dev(self, verts_ptr, vdtype, nv, tris_ptr, itype, nt, views_ptr, nviews, h, w, z_far, depth_ptr, uv2tri_ptr,
                                straddling_ptr, stream=None):
        """depth float32 [V, h, w], uv2tri int32 [V, h*w], straddling int64 [V] on the device, any may be None; enqueue only.  A vertex
        index outside [0, nv) writes nothing and is recorded for take_device_error."""
        self._check(self._lib.f3d_render_mesh_lookups_dev(self._h, verts_ptr, int(vdtype), int(nv), tris_ptr, int(itype), int(nt), views_ptr,
                                                          int(nviews), int(h), int(w), float(z_far), depth_ptr, uv2tri_ptr, straddling_ptr, stream))

    def vote_faces_dev(self, verts_ptr, vdtype, nv, tris_ptr, itype, nt, views_ptr, nviews, masks_ptr, h, w, z_far, votes_ptr, ncols,
                       views_per_pass=0, stream=None):
        """Enqueue only; a bad vertex index or a label >= ncols on a non-empty cell is recorded for take_device_error."""
        self._check(self._lib.f3d_vote_faces_dev(self._h, verts_ptr, int(vdtype), int(nv), tris_ptr, int(itype), int(nt), views_ptr, int(nviews),
                                                 masks_ptr, int(h), int(w), float(z_far), votes_ptr, int(ncols), int(views_per_pass), stream))

    def vote_visible_mesh_dev(self, xyz_ptr, dtype, n, verts_ptr, vdtype, nv, tris_ptr, itype, nt, views_ptr, nviews, masks_ptr, h, w, z_far,
                              depth_tol, votes_ptr, ncols, views_per_pass=0, stream=None):
        """Enqueue only; a bad vertex index or a label >= ncols on a visible sample is recorded for take_device_error."""
        self._check(self._lib.f3d_vote_visible_mesh_dev(self._h, xyz_ptr, int(dtype), int(n), verts_ptr, int(vdtype), int(nv), tris_ptr, int(itype),
                                                        int(nt), views_ptr, int(nviews), masks_ptr, int(h), int(w), float(z_far), float(depth_tol),
                                                        votes_ptr, int(ncols), int(views_per_pass), stream))

    def raster_counts_dev(self, verts_ptr, vdtype, nv, tris_ptr, itype, nt, views_ptr, nviews, h, w, z_far=np.inf, list_capacity=0,
                          depth_ptr=None, uv2tri_ptr=None, stream=None):
        """Diagnostic (synchronises): the (triangle, view) pairs each work tier of the rasteriser handled and the device-event times
        of the key fill and of the raster (f3d.h f3d_debug_raster_counts); list_capacity > 0 shrinks the deferral list for this call."""
        counts, ms = np.zeros(4, np.uint64), np.zeros(2)
        self._check(self._lib.f3d_debug_raster_counts(self._h, verts_ptr, int(vdtype), int(nv), tris_ptr, int(itype), int(nt), views_ptr,
                                                      int(nviews), int(h), int(w), float(z_far), int(list_capacity), depth_ptr, uv2tri_ptr,
                                                      _ptr(counts), _ptr(ms), stream))
        return {'small': int(counts[0]), 'medium': int(counts[1]), 'huge': int(counts[2]), 'overflow': int(counts[3]),
                'fill_ms': float(ms[0]), 'raster_ms': float(ms[1])}

    def vote_uv2pt_dev(self, uv2pt_ptr, mask_ptr, hw, votes_ptr, npts, ncols, stream=None):
        self._check(self._lib.f3d_vote_uv2pt_dev(self._h, uv2pt_ptr, mask_ptr, hw, votes_ptr, npts, ncols, stream))

    def vote_uv2pt_batch_dev(self, luts_ptr, masks_ptr, nframes, h, w, votes_ptr, npts, ncols, stream=None):
        self._check(self._lib.f3d_vote_uv2pt_batch_dev(self._h, luts_ptr, masks_ptr, int(nframes), int(h), int(w), votes_ptr, npts, ncols, stream))

    def sem_logits_to_mask_dev(self, sem_ptr, c, hw, conf, low_label, mask_ptr, stream=None):
        self._check(self._lib.f3d_sem_logits_to_mask_dev(self._h, sem_ptr, c, hw, float(conf or 0.0), int(low_label), mask_ptr, stream))

    def sem_logits_to_masks_dev(self, sem_ptr, nimg, c, hw, conf, low_label, masks_ptr, stream=None):
        """nimg images of logits [nimg, c, hw] -> nimg consecutive planes at masks_ptr (device-resident hand-off, no sync)."""
        self._check(self._lib.f3d_sem_logits_to_masks_dev(self._h, sem_ptr, int(nimg), c, hw, float(conf or 0.0), int(low_label), masks_ptr, stream))

    def points_in_obb_dev(self, xyz_ptr, dtype, n, boxes, bits_ptr, cooc_ptr, stream=None):
        b = _f64(boxes)
        self._check(self._lib.f3d_points_in_obb_dev(self._h, xyz_ptr, dtype, n, _ptr(b), len(b), bits_ptr, cooc_ptr, stream))

    def group_by_id_dev(self, ids_ptr, n, nids, order_ptr, sorted_ids_ptr, starts_ptr, stream=None):
        self._check(self._lib.f3d_group_by_id_dev(self._h, ids_ptr, n, int(nids), order_ptr, sorted_ids_ptr, starts_ptr, stream))

    def obb_extremes_dev(self, xyz_ptr, dtype, n, order_ptr, sorted_ids_ptr, nids, extremes_ptr, stream=None):
        self._check(self._lib.f3d_obb_extremes_dev(self._h, xyz_ptr, dtype, n, order_ptr, sorted_ids_ptr, int(nids), extremes_ptr, stream))

    def obb_hull_filter_dev(self, xyz_ptr, dtype, n, order_ptr, sorted_ids_ptr, starts_ptr, nids, fstart_ptr, facets_ptr, margin_ptr,
                            cand_ptr, cand_count_ptr, stream=None):
        self._check(self._lib.f3d_obb_hull_filter_dev(self._h, xyz_ptr, dtype, n, order_ptr, sorted_ids_ptr, starts_ptr, int(nids), fstart_ptr,
                                                      facets_ptr, margin_ptr, cand_ptr, cand_count_ptr, stream))

    def obb_candidates_dev(self, xyz_ptr, dtype, n, order_ptr, sorted_ids_ptr, starts_ptr, nids, min_members, cand_ptr, cand_start_ptr, stream=None):
        self._check(self._lib.f3d_obb_candidates_dev(self._h, xyz_ptr, dtype, n, order_ptr, sorted_ids_ptr, starts_ptr, int(nids), int(min_members),
                                                     cand_ptr, cand_start_ptr, stream))

    def gather_points_dev(self, xyz_ptr, dtype, idx_ptr, count, out_ptr, stream=None):
        self._check(self._lib.f3d_gather_points_dev(self._h, xyz_ptr, dtype, idx_ptr, int(count), out_ptr, stream))

    def obb_fit_dev(self, pts_ptr, start_ptr, nfit, total, boxes_ptr, status_ptr, isvert_ptr, nvert_ptr=None, stream=None):
        self._check(self._lib.f3d_obb_fit_dev(self._h, pts_ptr, start_ptr, int(nfit), int(total), boxes_ptr, status_ptr, isvert_ptr, nvert_ptr, stream))

    def unproject_depth_batch_dev(self, depth_ptr, depth_code, nframes, h, w, K, q_wxyz, t, out_ptr, depth_scale=1000.0, stream=None):
        """F depth frames [F,h,w] on the device -> world points float64 [F,h*w,3] in one launch; q_wxyz [F,4], t [F,3] host arrays."""
        K, q, t = _f64(K, (3, 3)), _f64(q_wxyz, (int(nframes), 4)), _f64(t, (int(nframes), 3))
        self._check(self._lib.f3d_unproject_depth_batch_dev(self._h, depth_ptr, int(depth_code), int(nframes), int(h), int(w), _ptr(K), float(depth_scale),
                                                            _ptr(q), _ptr(t), out_ptr, stream))

    def estimate_normals_batch_dev(self, xyz_ptr, nframes, n, cam_centres, normals_ptr, radius=0.05, max_nn=30, orient=True,
                                   counts_ptr=None, neighbours_ptr=None, stream=None):
        """F frames of n points, float64 [F,n,3] on the device -> normals [F,n,3] (counts int32 [F*n], neighbours int32 [F*n, max_nn]
        optional); cam_centres: host [F,3].  One blocking readback per call (f3d.h f3d_estimate_normals_batch_dev)."""
        c = _f64(cam_centres, (int(nframes), 3)) if orient else None
        self._check(self._lib.f3d_estimate_normals_batch_dev(self._h, xyz_ptr, int(nframes), int(n), _ptr(c), float(radius), int(max_nn),
                                                             int(bool(orient)), normals_ptr, counts_ptr, neighbours_ptr, stream))

    def relabel_dev(self, ids_ptr, n, from_id, to_id, count_ptr=None, stream=None):
        self._check(self._lib.f3d_relabel_dev(self._h, ids_ptr, n, int(from_id), int(to_id), count_ptr, stream))

    # a5 on a device-resident cloud (Fusion.fuse_device): device pointers, enqueue only (f3d.h)
    def patch_match_dev(self, uv_ptr, m, h, w, half, radius, min_cosine, seed_pts_ptr, seed_nrm_ptr, q_pts_ptr, q_nrm_ptr, q_clr_ptr,
                        free_ptr, owner_ptr, sums_ptr, counts_ptr, stream=None):
        self._check(self._lib.f3d_patch_match_dev(self._h, uv_ptr, int(m), int(h), int(w), int(half), float(radius), float(min_cosine),
                                                  seed_pts_ptr, seed_nrm_ptr, q_pts_ptr, q_nrm_ptr, q_clr_ptr, free_ptr, owner_ptr, sums_ptr,
                                                  counts_ptr, stream))

    def patch_seeds_sums_dev(self, q_pts_ptr, q_nrm_ptr, q_clr_ptr, prio_ptr, free_ptr, h, w, half, radius, min_cosine, owner_ptr, sums_ptr,
                             counts_ptr, stream=None):
        """-> the number of seed-resolution rounds (each one a 4-byte readback)."""
        rounds = C.c_int32(0)
        self._check(self._lib.f3d_patch_seeds_sums_dev(self._h, q_pts_ptr, q_nrm_ptr, q_clr_ptr, prio_ptr, free_ptr, int(h), int(w), int(half),
                                                       float(radius), float(min_cosine), owner_ptr, sums_ptr, counts_ptr, C.byref(rounds), stream))
        return rounds.value

    def fusion_hits_dev(self, inside_ptr, uv_all_ptr, n, count_ptr, pts_ptr, nrm_ptr, valid_ptr, npx, ids_ptr, uv_ptr, hit_pts_ptr,
                        hit_nrm_ptr, stats_ptr, stream=None):
        self._check(self._lib.f3d_fusion_hits_dev(self._h, inside_ptr, uv_all_ptr, int(n), count_ptr, pts_ptr, nrm_ptr, valid_ptr, int(npx),
                                                  ids_ptr, uv_ptr, hit_pts_ptr, hit_nrm_ptr, stats_ptr, stream))

    def fusion_seed_update_dev(self, ids_ptr, m, sums_ptr, counts_ptr, norm_mode, pts_ptr, nrm_ptr, clr_ptr, nmerges_ptr, occ_ptr, stream=None):
        self._check(self._lib.f3d_fusion_seed_update_dev(self._h, ids_ptr, int(m), sums_ptr, counts_ptr, int(norm_mode), pts_ptr, nrm_ptr, clr_ptr,
                                                         nmerges_ptr, occ_ptr, stream))

    def fusion_lookup_dev(self, owner_ptr, ids_ptr, npx, uv2pt_ptr, free_ptr, stream=None):
        self._check(self._lib.f3d_fusion_lookup_dev(self._h, owner_ptr, ids_ptr, int(npx), uv2pt_ptr, free_ptr, stream))

    def fusion_frame_check_dev(self, free_ptr, q_pts_ptr, q_nrm_ptr, npx, radius, min_cosine, stats_ptr, stream=None):
        self._check(self._lib.f3d_fusion_frame_check_dev(self._h, free_ptr, q_pts_ptr, q_nrm_ptr, int(npx), float(radius), float(min_cosine),
                                                         stats_ptr, stream))

    def fusion_prio_dev(self, order_ptr, npx, prio_ptr, stream=None):
        self._check(self._lib.f3d_fusion_prio_dev(self._h, order_ptr, int(npx), prio_ptr, stream))

    def fusion_new_seeds_dev(self, owner_ptr, prio_ptr, sums_ptr, counts_ptr, npx, norm_mode, count_ptr, cap, pts_ptr, nrm_ptr, clr_ptr,
                             nmerges_ptr, occ_ptr, uv2pt_ptr, free_ptr, stream=None):
        self._check(self._lib.f3d_fusion_new_seeds_dev(self._h, owner_ptr, prio_ptr, sums_ptr, counts_ptr, int(npx), int(norm_mode), count_ptr,
                                                       int(cap), pts_ptr, nrm_ptr, clr_ptr, nmerges_ptr, occ_ptr, uv2pt_ptr, free_ptr, stream))


_default = {}


def default_context(device=None):
    """Process-wide context per device (LOCAL_RANK selects the device under torchrun)."""
    if device is None:
        device = int(os.environ.get('F3D_DEVICE', os.environ.get('LOCAL_RANK', '0')))
    ctx = _default.get(device)
    if ctx is None:
        ctx = _default[device] = Context(device)
    return ctx
