"""Every grid-stride kernel behind f3d_grid_for through several passes: one case per kernel source, run with the process-wide debug cap
(f3d_debug_grid_cap) at 1 and at 3 blocks and compared with the reference and the rule that family's own tests use.  The inputs are
small (2500 points, 48 x 56 images): at three blocks of 256 threads the per-point and per-pixel launches take four passes, the last one
ragged, and wave-per-item kernels over a hundred.

A case is a function of a seed -> (run, want, check, rows): run(ctx) calls the public entries, want is what the reference says,
check(got, want) asserts that family's comparison, rows is the reference output whose rows must differ between two seeds.  Every case
first runs uncapped on a second input of the same shapes (another seed), so that no element a capped kernel fails to write can hold
the right value from an earlier call in a recycled buffer; then it sets the cap, runs the real input and reads the counters: a case
whose launches the cap did not lower would prove nothing."""
import numpy as np
import pytest

import f3d
from family_cases import CASES, OTHER_SEED, Q0, SEED, cloud, prepared, rows_that_differ

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    """The default context with the process-wide cap off before and after the test, whatever happens in it."""
    c = f3d.default_context()
    c.debug_grid_cap(0)
    try:
        yield c
    finally:
        c.debug_grid_cap(0)
        c.debug_grid_cap_stats()


@pytest.mark.parametrize('cap', [1, 3])
@pytest.mark.parametrize('name', sorted(CASES))
def test_results_do_not_depend_on_the_grid(ctx, name, cap):
    run, want, check, rows = prepared(name, SEED)
    other_run, _, _, other_rows = prepared(name, OTHER_SEED)
    nrows = len(rows)
    assert nrows > 0 and 2 * rows_that_differ(rows, other_rows) >= nrows             # a stale right answer would be a wrong one
    other_run(ctx)                                                                  # uncapped: fills every recycled buffer with other values
    ctx.debug_grid_cap(cap)
    ctx.debug_grid_cap_stats()
    try:
        got = run(ctx)
    except RuntimeError as e:
        if isinstance(e, f3d.F3DUnavailable) or 'hip error' in str(e).lower():      # a HIP call failed (the library's or torch's): the device
            pytest.exit(f'{name} at cap {cap}: {e!r}; nothing more is started on this device', returncode=3)     # may have faulted
        raise                                                                       # any other error status is an ordinary failure
    finally:
        ctx.debug_grid_cap(0)
    calls, lowered = ctx.debug_grid_cap_stats()
    print(f'{name} cap {cap}: {calls} grids sized under the cap, {lowered} lowered')
    assert calls >= lowered >= 1
    check(got, want)


def test_zz_the_cap_is_off_again(ctx):
    """Runs last in the module (pytest keeps the file's order): the cap reads back as off -- a grid sized now is neither counted nor
    lowered -- and a negative cap is refused."""
    assert ctx.debug_grid_cap_stats() == (0, 0)
    pts = cloud(np.random.default_rng(0))
    ctx.rotate(pts, Q0)
    assert ctx.debug_grid_cap_stats() == (0, 0)
    with pytest.raises(ValueError):
        ctx.debug_grid_cap(-1)
    ctx.debug_grid_cap(3)
    ctx.rotate(pts, Q0)
    ctx.debug_grid_cap(0)
    assert ctx.debug_grid_cap_stats() == (1, 1) and ctx.debug_grid_cap_stats() == (0, 0)
