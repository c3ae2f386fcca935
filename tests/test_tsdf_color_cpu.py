"""CPU-side checks of the TSDF colour channel: the bindings exist, argument errors need no device, the colour-pixel rule is the
nearest rule, and the NumPy restatement (tests/tsdf_color_ref.py) keeps the two colours of the sphere-and-wall scene apart, which the
rule the contract rejects (colour on every TSDF update) does not."""
import ctypes as C

import numpy as np
import pytest

import f3d
import tsdf_ref as R
import tsdf_color_ref as CR
from Fusion3DSeg.segUtils import reconstruct, registration, voting

COLOR_SYMBOLS = ['f3d_tsdf_integrate_color', 'f3d_tsdf_integrate_color_dev', 'f3d_tsdf_extract_colors', 'f3d_tsdf_extract_colors_dev']


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------ symbols
def test_symbols_are_bound():
    lib = f3d.library()
    for name in COLOR_SYMBOLS:
        fn = getattr(lib, name)
        assert name in lib._f3d_symbols
        assert fn.restype is C.c_int and fn.argtypes and fn.argtypes[0] is C.c_void_p
    # the integrate arguments plus color, rgb, hc, wc_img; the _dev forms add the stream, extract_colors_dev also tsdf
    assert len(lib.f3d_tsdf_integrate_color.argtypes) == len(lib.f3d_tsdf_integrate.argtypes) + 4
    assert len(lib.f3d_tsdf_integrate_color_dev.argtypes) == len(lib.f3d_tsdf_integrate_color.argtypes) + 1
    assert len(lib.f3d_tsdf_extract_colors_dev.argtypes) == len(lib.f3d_tsdf_extract_colors.argtypes) + 2
    assert lib.f3d_tsdf_integrate_color.argtypes[10] is C.c_float                 # max_weight, after color
    for name in ('tsdf_integrate_color', 'tsdf_extract_colors', 'tsdf_integrate_color_dev', 'tsdf_extract_colors_dev'):
        assert callable(getattr(f3d.Context, name))


def test_header_declares_the_entries():
    import re
    from conftest import ROOT
    text = re.sub(r'/\*.*?\*/', '', (ROOT / 'include' / 'f3d.h').read_text(), flags=re.S)
    for name in COLOR_SYMBOLS:
        assert re.search(r'\bint %s\s*\(' % name, text)


def test_base_scene_is_that_of_the_depth_tests():
    import test_tsdf_gpu as G
    assert (CR.DIMS, CR.VS, CR.TRUNC, CR.H, CR.W, CR.MAX_DEPTH) == (G.DIMS, G.VS, G.TRUNC, G.H, G.W, G.MAX_DEPTH)
    assert np.array_equal(CR.LO, G.LO) and CR.EYES == G.EYES and CR.TARGETS == G.TARGETS


# ------------------------------------------------------------------------------------------------ argument errors
def test_context_checks_arrays_before_any_device_call():
    """A Context that was never opened has no library handle and no device: a call that got past the array checks would fail with
    AttributeError.  Every bad array is refused with TypeError / ValueError before that."""
    ctx = object.__new__(f3d.Context)
    shape = (6, 5, 4)
    tsdf, weight, color = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros(shape + (4,), np.float32)
    depths, rgb, views = np.ones((2, 4, 4)), np.zeros((2, 3, 5, 3), np.uint8), np.zeros((2, f3d.VIEW_DOUBLES))
    lo = np.zeros(3)

    def integrate(**kw):
        a = dict(color=color, rgb=rgb, depths=depths, views=views)
        a.update(kw)
        ctx.tsdf_integrate_color(tsdf, weight, a['color'], lo, 0.1, 0.4, 64, a['depths'], a['rgb'], a['views'])

    for bad in [dict(color=color.astype(np.float64)), dict(color=None), dict(rgb=rgb.astype(np.float32)), dict(rgb=rgb.astype(np.int8))]:
        with pytest.raises(TypeError):
            integrate(**bad)
    for bad in [dict(color=np.zeros(shape + (3,), np.float32)), dict(color=np.zeros((6, 5, 5, 4), np.float32)),
                dict(color=np.zeros((4, 5, 6, 4), np.float32).transpose(2, 1, 0, 3)), dict(color=color[..., ::1][:, :, ::-1]),
                dict(rgb=rgb[:1]), dict(rgb=np.zeros((3, 3, 5, 3), np.uint8)), dict(rgb=np.zeros((2, 3, 5, 4), np.uint8)),
                dict(rgb=np.zeros((2, 3, 5), np.uint8)), dict(rgb=np.zeros((2, 0, 5, 3), np.uint8)), dict(rgb=np.zeros((2, 3, 0, 3), np.uint8)),
                dict(depths=np.ones((4, 4))), dict(views=views[:1])]:
        with pytest.raises(ValueError):
            integrate(**bad)
    frozen = color.copy()
    frozen.setflags(write=False)
    with pytest.raises(ValueError):
        integrate(color=frozen)
    with pytest.raises(AttributeError):
        integrate()                                                     # good arrays reach the library, which this object lacks
    for bad, err in [(color.astype(np.float64), TypeError), (np.zeros(shape + (3,), np.float32), ValueError), (None, TypeError)]:
        with pytest.raises(err):
            ctx.tsdf_extract_colors(tsdf, weight, bad, lo, 0.1)
    assert not tsdf.any() and not weight.any() and not color.any()


def test_volume_argument_errors_need_no_device():
    V = reconstruct.TSDFVolume
    plain, vol = V((0.0, 0.0, 0.0), (4, 5, 6), 0.1), V((0.0, 0.0, 0.0), (4, 5, 6), 0.1, color=True)
    assert plain.color is None
    assert vol.color.shape == (6, 5, 4, 4) and vol.color.dtype == np.float32 and not vol.color.any()
    K, q, t = np.eye(3), np.array([[1.0, 0, 0, 0]]), np.zeros((1, 3))
    depths, rgb = np.zeros((1, 4, 4)), np.zeros((1, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match='color=True'):
        plain.integrate(depths, K, q, t, colors=rgb)
    with pytest.raises(ValueError, match='color=True'):
        plain.extract_mesh(colors=True)
    with pytest.raises(TypeError):
        vol.integrate(depths, K, q, t, colors=rgb.astype(np.float32))
    for bad in [np.zeros((2, 8, 8, 3), np.uint8), np.zeros((1, 8, 8, 4), np.uint8), np.zeros((1, 8, 8), np.uint8), np.zeros((1, 0, 8, 3), np.uint8)]:
        with pytest.raises(ValueError):
            vol.integrate(depths, K, q, t, colors=bad)
    with pytest.raises(ValueError):
        registration.track_frames(plain, depths, K, q, t, colors=rgb)
    with pytest.raises(ValueError):
        registration.track_frames(vol, depths, K, q, t, colors=np.zeros((2, 8, 8, 3), np.uint8))
    none = np.zeros((0, 4, 4)), K, np.zeros((0, 4)), np.zeros((0, 3))
    assert vol.integrate(*none, colors=np.zeros((0, 8, 8, 3), np.uint8)) is vol     # no frames: nothing to do, no device
    with pytest.raises(ValueError):
        plain.integrate(*none, colors=np.zeros((0, 8, 8, 3), np.uint8))
    assert not vol.color.any()


# ------------------------------------------------------------------------------------------------ the pixel rule
@pytest.mark.parametrize('w,wc', [(192, 720), (256, 960), (48, 7), (48, 48), (48, 96), (48, 180), (40, 150), (40, 5), (7, 48), (1, 4), (5, 3)])
def test_colour_pixel_is_resize_nearest(w, wc):
    """uc = u * wc // w picks the source pixel cv2's INTER_NEAREST (voting.resize_nearest) picks when the colour image is resized to
    the depth frame's size, along either axis."""
    index = np.arange(wc, dtype=np.int64)[None, :].repeat(2, axis=0)
    uc = CR.color_pixel(np.arange(w), w, wc)
    assert np.array_equal(voting.resize_nearest(index, w, 2)[0], uc) and uc.min() >= 0 and uc.max() < wc
    assert np.array_equal(voting.resize_nearest(index.T.copy(), 2, w)[:, 0], uc)


# ------------------------------------------------------------------------------------------------ the restatement
def zeros(dims):
    s = tuple(dims[::-1])
    return np.zeros(s, np.float32), np.zeros(s, np.float32), np.zeros(s + (4,), np.float32)


def near_masks(verts):
    r = 2.0 * np.sqrt(3.0) * CR.VS
    sphere = np.abs(np.linalg.norm(verts - R.SPHERE_C[None, :], axis=1) - R.SPHERE_R) <= r
    wall = np.abs(verts[:, 2] - R.WALL_Z) <= r
    return sphere, wall


@pytest.mark.parametrize('sel', [[0], [0, 1, 4], [0, 1, 2, 3, 4]])
def test_two_colours_stay_apart(sel):
    """The sphere one constant colour, the wall another.  Every vertex is coloured: a crossing edge has an inside end, an inside end
    had a negative sample, and a negative sample is in band.  Every vertex within 2 sqrt(3) voxels of the sphere carries exactly the
    sphere's colour, every vertex that close to the wall exactly the wall's, and no vertex is near neither: a voxel's in-band samples
    lie within trunc = 4 voxels of the surface their pixel sees, and the averages of one constant are exact.  The same restatement with
    the colour updated on every TSDF update fails that on the sphere: the voxels in front of its silhouette take the wall's colour
    from the frames that see the wall behind them."""
    K, q, t, depths, rgb = CR.two_colour_scene(sel)
    args = (CR.TWO_LO, CR.VS, CR.TRUNC, 64, depths, rgb, K, q, t, 1.0, CR.MAX_DEPTH)
    tsdf, weight, color = CR.integrate_color(*zeros(CR.DIMS), *args)
    want = R.integrate(*zeros(CR.DIMS)[:2], CR.TWO_LO, CR.VS, CR.TRUNC, 64, depths, K, q, t, 1.0, CR.MAX_DEPTH)
    assert np.array_equal(bits(tsdf), bits(want[0])) and np.array_equal(bits(weight), bits(want[1]))
    assert (color[..., 3] <= weight).all() and (color[..., 3] < weight).any() and (color[..., 3] > 0).any()
    verts, _ = R.extract(tsdf, weight, CR.TWO_LO, CR.VS, 1.0)
    vrgb, colored = CR.vertex_colors(tsdf, weight, color, 1.0)
    assert vrgb.shape == (len(verts), 3) and colored.shape == (len(verts),) and len(verts) > 300
    assert colored.all()
    sphere, wall = near_masks(verts)
    print(f'frames {sel}: {len(verts)} vertices, {int(sphere.sum())} near the sphere, {int(wall.sum())} near the wall, '
          f'{int((sphere & wall).sum())} near both, {int((~sphere & ~wall).sum())} near neither')
    assert sphere.sum() > 100 and wall.sum() > 100 and not (sphere & wall).any() and (sphere | wall).all()
    assert (vrgb[sphere] == CR.SPHERE_RGB[None, :]).all()
    assert (vrgb[wall] == CR.WALL_RGB[None, :]).all()
    if len(sel) > 1:                                                    # the rejected rule: it needs a second view to bleed
        _, _, bled = CR.integrate_color(*zeros(CR.DIMS), *args, every_update=True)
        brgb, _ = CR.vertex_colors(tsdf, weight, bled, 1.0)
        exact = int((brgb[sphere] == CR.SPHERE_RGB[None, :]).all(axis=1).sum())
        print(f'frames {sel}: colour on every update leaves {exact} of {int(sphere.sum())} sphere vertices exact')
        assert exact < sphere.sum()


def test_constant_colour_stays_exact_up_to_max_weight():
    """One frame integrated 7 times with max_weight 4: (C w + C) / (w + 1) == C exactly for integers of this size, wc stops at 4."""
    K, q, t, depths, _ = CR.two_colour_scene([0])
    rgb = np.empty((1, 5, 3, 3), np.uint8)
    rgb[...] = np.array([17, 255, 1], np.uint8)
    state = zeros(CR.DIMS)
    for n in range(7):
        state = CR.integrate_color(*state, CR.TWO_LO, CR.VS, CR.TRUNC, 4, depths, rgb, K, q, t, 1.0, CR.MAX_DEPTH)
        seen = state[2][..., 3] > 0
        assert seen.any() and (state[2][..., 3][seen] == min(n + 1, 4)).all()
        assert (state[2][..., :3][seen] == np.array([17, 255, 1], np.float32)).all()
        assert not state[2][~seen].any()
    assert state[1].max() == 4


def test_band_edge_is_in_band():
    """tsdf_ref.TIES, the wide volume: every product is exact, the flat depth is 1.0 and trunc 0.21875, so the layer z = 0.78125 has
    sdf == trunc, val == 1.0 exactly, and is coloured (in band iff !(val > 1.0)); the layer in front of it has val > 1: its TSDF is
    updated with the clamped 1.0 and its colour is not."""
    g, vol = R.TIES, R.TIE_VOLUMES['wide']
    depth = np.full((1, g['h'], g['w']), g['max_depth'])
    rgb = np.full((1, 4, 4, 3), 99, np.uint8)
    tsdf, weight, color = CR.integrate_color(*zeros(vol['dims']), vol['lo'], g['vs'], g['trunc'], 64, depth, rgb, g['K'], g['wxyz'][None],
                                             g['t'][None], 1.0, g['max_depth'])
    terms = R.frame_terms(g['K'], g['wxyz'], g['t'], vol['lo'], vol['dims'], g['vs'], depth[0])
    z = vol['lo'][2] + (np.arange(vol['dims'][2]) + 0.5) * g['vs']
    k = int(np.flatnonzero(z == 0.78125)[0])
    sdf = terms['sdf'].reshape(vol['dims'][::-1])
    seen = weight > 0
    assert seen[k].sum() >= 20 and seen[k - 1].sum() >= 20
    assert (sdf[k][seen[k]] == g['trunc']).all() and (tsdf[k][seen[k]] == 1.0).all()
    assert (color[k][seen[k]] == np.array([99, 99, 99, 1], np.float32)).all()
    assert (tsdf[k - 1][seen[k - 1]] == 1.0).all() and (sdf[k - 1][seen[k - 1]] > g['trunc']).all()
    assert not color[k - 1].any() and not color[:k].any()
    assert np.array_equal(color[..., 3] > 0, seen & (np.arange(vol['dims'][2]) >= k)[:, None, None])
