"""Where the label fill of the one-shot sorting call rides (csrc/f3d_fuse.hip: f3d_launch_cell_sort_with_riders): beside pass 1 of the
cell sort for a small cloud, as rider blocks of k_rs_hist2 from F3D_RIDER_SMALL_POINTS = 512 x 8192 points on.  Both sides of that size:
every point the vote leaves unlabelled must carry the fill value, so the whole label vector is held to the same call without the sort
(no riders, a fill kernel of its own) and a seeded sample to oracle/np_ref.py."""
import numpy as np
import pytest

from test_fuse_riders_gpu import NCLASSES, ODD, _call, _check, _cloud, _masks, _oracle, ctx  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu

SMALL_POINTS = 512 * 8192


@pytest.mark.parametrize('flt', [None, [3, 5, 7]], ids=['presence_book', 'filter_book'])
@pytest.mark.parametrize('n', [SMALL_POINTS - 1, SMALL_POINTS, SMALL_POINTS + 8193])
def test_fill_on_both_sides_of_the_small_cloud_size(ctx, n, flt):
    """filter_book: no presence pass, so a small cloud's pass 1 carries the fill alone and a large cloud's pass 1 has no riders at all."""
    h, w = ODD
    m = _masks(2, h, w, 0, 8)
    pts = _cloud(SMALL_POINTS + 8193)[:n]
    got = _call(ctx, pts, 2, h, w, m, 0.5, flt=flt)
    plain = _call(ctx, pts, 2, h, w, m, 0.5, flt=flt, sort=False)
    assert int((got == -7).sum()) == 0                                             # no label left as the caller's
    assert flt is not None or (got == NCLASSES).any()                              # the fill value occurs: points that no view sees
    _check(got, plain, 'sorting call against the plain call')
    sel = np.random.default_rng(20250102).integers(0, n, 50_000)
    _check(got[sel], _oracle(pts[sel], 2, h, w, m, 0.5, flt), 'sample against the oracle')
