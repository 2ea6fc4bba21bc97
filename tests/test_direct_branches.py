"""Direct pose (viso_direct_pose -> direct_level_kernel) against the fp64
oracle on the window, edge and tile paths that the sequence data of
tests/test_track.py does not reach.

The inputs and the census that shows which kernel branch each of them takes
are tests/direct_cases.py; tests/test_direct_cases.py proves on the CPU that
every branch is populated.  Here:

* faithful mode, every case and every size of the tile sweep: relative
  Frobenius < 1e-12 against oracle_lib.direct_pose (the stage's bar in
  tests/test_track.py: the arithmetic is bit-identical, libm's sin / cos may
  differ by an ulp).  A failure prints the case's census: the classes it
  populates localise the fault.
* the tile sweep pins T = min(64, ceil(n / 256)): one round of waves
  (T <= 12), the looping waves with the last-arriver tree (12 < T <= 16), the
  block-barrier tree (T > 16), the 9-wave prefetch wrapping once (T > 9) and
  twice (T > 18), a partial last tile, fewer than 256 tiles, and the full map
  of 16,384 points; 16,385 points are refused by the host (VISO_ERR_ARG).
* tolerance mode (precision = FAST; the split tiling of tile_range, the fp32
  point routine, the LDLT solve): relative Frobenius < 1e-4 against the same
  oracle poses, the mode's stated contract, on the cases and sweep sizes whose
  oracle cond(H) stays within direct_cases.COND_CEILING (the conditioning of
  the data that contract was shown on; tests/test_direct_cases.py lists what
  is excluded and why).  This leg found the tolerance-mode point routine
  taking floor() where sample_px truncates: a gradient sample at a coordinate
  in (-1, 0) (class edge_lt, a projection in [4, 5)) read taps -1, 0 instead
  of 0, 1, which moved odd_t64 by 5.6e-4 and big_step by 1.5e-3; with the
  routine following the truncation rule every admitted input is below 1e-9.
"""
import numpy as np
import pytest

from tests import direct_cases as dc

_fast_ctx: dict = {}


def _rel_frob(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _context(K, fast):
    import viso_amd
    if not fast:
        return viso_amd.default_context(K=K)
    c = _fast_ctx.get(K)
    if c is None:
        c = viso_amd.Context(viso_amd.default_params(fx=K[0], fy=K[1], cx=K[2], cy=K[3],
                                                     precision=viso_amd.PRECISION_FAST))
        _fast_ctx[K] = c
    return c


def _check(key, fast, bar):
    c = dc.get(key)
    exp = dc.oracle_pose(key)
    got = _context(c["K"], fast).direct_pose(c["last"], c["cur"], c["w"], c["h"], c["points"], c["pose_last"],
                                            c["pose_init"])
    rel = _rel_frob(got, exp)
    print(f"direct pose {key} {'fast' if fast else 'faithful'}: rel Frobenius {rel:.3e} (bar {bar:g})")
    assert np.isfinite(got).all() and rel < bar, f"{key}: rel {rel:.3e} >= {bar:g}\n" + dc.format_census(dc.census(key))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dc.CASES))
def test_gpu_direct_branches_faithful(name):
    _check(name, False, 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("n", dc.SWEEP_N)
def test_gpu_direct_tile_sweep_faithful(n):
    _check(n, False, 1e-12)


@pytest.mark.gpu
def test_gpu_direct_pose_refuses_more_than_the_map_capacity():
    import viso_amd
    c = dc.sweep_case(3)
    pts = np.ones((16385, 3))
    with pytest.raises(viso_amd._lib.VisoError) as e:
        _context(c["K"], False).direct_pose(c["last"], c["cur"], c["w"], c["h"], pts, c["pose_last"],
                                            c["pose_init"])
    assert e.value.rc == -1  # VISO_ERR_ARG: a host check, nothing is launched


@pytest.mark.gpu
@pytest.mark.parametrize("name", dc.FAST_CASES)
def test_gpu_direct_branches_tolerance_mode(name):
    assert max(dc.census(name)["cond"]) <= dc.COND_CEILING
    _check(name, True, 1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("n", dc.FAST_SWEEP_N)
def test_gpu_direct_tile_sweep_tolerance_mode(n):
    assert max(dc.census(n)["cond"]) <= dc.COND_CEILING
    _check(n, True, 1e-4)
