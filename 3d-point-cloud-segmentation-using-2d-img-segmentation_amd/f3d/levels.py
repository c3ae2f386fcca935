"""Device-pointer bindings of coarse-to-fine registration (f3d.h f3d_depth_half_dev, f3d_maps_half_dev, f3d_icp_levels_dev).

The host bindings are ``Context.depth_half``, ``Context.maps_half`` and ``Context.icp_levels``.  Their device-pointer twins are
functions of this module that take the context first, not ``Context.*_dev`` methods: tests/test_route_cases_cpu.py checks every such
method against the table in tests/route_cases.py, and moving these three onto ``Context`` together with their table rows is a
follow-up of its own.  Until then tests/test_registration_levels_gpu.py carries their stalled-stream and strided-input cases itself.

Raw pointers in (``tensor.data_ptr()``), enqueue only: nothing here synchronises with the host.
"""
import ctypes

from f3d import IcpLevel, _f64, _fill_level, _half_check, _icp_levels_check, _ptr

__all__ = ['depth_half_dev', 'maps_half_dev', 'icp_levels_dev']


def depth_half_dev(ctx, depth_ptr, depth_type, h, w, depth_scale, max_depth, gate, out_ptr, stream=None):
    """One pyramid step of the depth frame [h, w] of `depth_type` on the device into out float64 [(h // 2) * (w // 2)], metres."""
    gate = _half_check('depth', (h, w), gate)
    ctx._check(ctx._lib.f3d_depth_half_dev(ctx._h, depth_ptr, int(depth_type), int(h), int(w), float(depth_scale), float(max_depth), gate, out_ptr,
                                           stream))


def maps_half_dev(ctx, vertex_ptr, normal_ptr, intensity_ptr, hm, wm, view_ptr, gate, vertex_out_ptr, normal_out_ptr, intensity_out_ptr=None,
                  stream=None):
    """One pyramid step of the model maps float64 [hm*wm, 3] (and the intensity map [hm*wm]; None = none, then no intensity output
    either) seen by the device view record into maps of (hm // 2) x (wm // 2) pixels."""
    gate = _half_check('the model image', (hm, wm), gate)
    if (intensity_ptr is None) != (intensity_out_ptr is None):
        raise ValueError('the intensity output goes with the intensity map: pass both or none')
    ctx._check(ctx._lib.f3d_maps_half_dev(ctx._h, vertex_ptr, normal_ptr, intensity_ptr, int(hm), int(wm), view_ptr, gate, vertex_out_ptr,
                                          normal_out_ptr, intensity_out_ptr, stream))


def icp_levels_dev(ctx, levels, q_wxyz, t, max_depth, pose_ptr, stats_ptr, status_ptr=None, rgb_ptr=None, hc=0, wc=0, color_weight=None, stream=None):
    """The rounds of icp_dev / icp_color_dev over `levels`, coarsest first, with no host round trip between rounds or levels.  A level
    is a dict of device pointers and numbers: depth, depth_type, h, w, K, depth_scale (default 1), model_vertex, model_normal, hm, wm,
    model_view, max_dist, iterations, min_pairs, and with colour model_intensity; rgb_ptr (uint8 [hc, wc, 3]) and color_weight go with
    the intensity maps, all or none.  pose float64 [7], stats float64 [sum of iterations, 3 or 5], status int32 [1] (may be None)."""
    levels = _icp_levels_check(levels, rgb_ptr, color_weight)
    for lv in levels:
        missing = [k for k in ('depth_type', 'h', 'w') if k not in lv]
        if missing:
            raise ValueError(f'a level lacks {missing}')
    q, t = _f64(q_wxyz, (4,)), _f64(t, (3,))
    recs = (IcpLevel * len(levels))()
    for rec, lv in zip(recs, levels):
        _fill_level(rec, lv['depth'], lv['depth_type'], lv['h'], lv['w'], _f64(lv['K'], (3, 3)), lv.get('depth_scale', 1.0), lv['model_vertex'],
                    lv['model_normal'], lv.get('model_intensity'), lv['hm'], lv['wm'], lv['model_view'], lv['max_dist'], lv['iterations'],
                    lv['min_pairs'])
    if rgb_ptr is not None:
        color_weight = float(color_weight)
        if not (color_weight >= 0.0 and color_weight < float('inf')):
            raise ValueError(f'color_weight must be finite and not negative, got {color_weight}')
    ctx._check(ctx._lib.f3d_icp_levels_dev(ctx._h, ctypes.byref(recs), len(levels), float(max_depth), _ptr(q), _ptr(t), rgb_ptr, int(hc), int(wc),
                                           0.0 if rgb_ptr is None else color_weight, pose_ptr, stats_ptr, status_ptr, stream))
