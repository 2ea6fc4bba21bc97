"""The prologue of direct_level_kernel (viso_amd/csrc/direct.hip): the load and
canonical tree of the previous level's tile partials, and the 6 x 6 solve
(viso_amd/csrc/direct_solve.hpp), whose LU places each step's quotients on
lanes.

* CPU, sizes: n in SIZES gives one point per tile (map_tile(n) == 1), so the
  tile count equals n and crosses every wave edge of the 256-thread partial
  loader (63 / 64 / 65, 127 / 128 / 129, 191 / 192 / 193).  Each case is usable
  in the oracle alone (the conditions of test_direct_cases.test_case_is_usable,
  and good points at every level).
* CPU, pivots: a numpy PartialPivLU (first maximal |pivot|, as
  tests/pose_refine_ref.inverse6) on the oracle's per-level H of PIVOT_KEYS:
  over these 20 solves every LU step 0..4 occurs both with and without a row
  swap.  The row-swap branch sits between the lane-placed divisions of one
  step and the next step's, so these are the inputs that can break it.
* GPU, against the oracle: relative Frobenius < 1e-12 (the stage's bar),
  faithful, on the nine sizes and the five pivot keys.
* GPU, against the parent commit's library, bit for bit:
  tests/golden/direct_prologue_parent.npz holds the 12 pose doubles as uint64
  bit patterns per key and precision, recorded with the library of the commit
  before the lane-placed quotients (tests/golden/make_direct_prologue.py).
  Both libraries use the same device sincos, so no ulp allowance applies.
"""
import os

import numpy as np
import pytest

from tests import direct_cases as dc

SIZES = (63, 64, 65, 127, 128, 129, 191, 192, 193)
PIVOT_KEYS = ("gentle", "big_step_far", "near_pts", 3, 12)
PARENT_KEYS = SIZES + PIVOT_KEYS + (255, 256, 257, 2465, "small_l3", "odd_t64")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "direct_prologue_parent.npz")


def fast_admitted(key) -> bool:
    """The keys the tolerance-mode contract covers (direct_cases)."""
    return key in dc.FAST_CASES or key in dc.FAST_SWEEP_N


def golden_name(key, fast: bool) -> str:
    return f"{'fast' if fast else 'faithful'}_{key}"


def partial_piv_lu_transpositions(H):
    """Row transpositions of Eigen's PartialPivLU on a 6 x 6 H: tr[k] is the
    row swapped with row k at step k (the first maximal |pivot| wins)."""
    lu = np.array(H, np.float64).reshape(6, 6).copy()
    tr = []
    for k in range(6):
        col = np.abs(lu[k:, k])
        p = k + int(np.argmax(col))  # argmax returns the first maximum
        tr.append(p)
        if col.max() != 0.0:
            if p != k:
                lu[[k, p]] = lu[[p, k]]
            lu[k + 1:, k] = lu[k + 1:, k] / lu[k, k]
        lu[k + 1:, k + 1:] = lu[k + 1:, k + 1:] - np.outer(lu[k + 1:, k], lu[k, k + 1:])
    return tuple(tr)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_are_one_point_per_tile_and_usable(n):
    assert dc.map_tile(n) == 1
    cen = dc.census(n)
    assert cen["n"] == n and cen["tile"] == 1
    assert all(cen["update_finite"]), (n, cen["update_finite"])
    assert all(g > 0 for g in cen["good"]), (n, cen["good"])
    assert cen["moved"], n
    assert not np.array_equal(dc.oracle_pose(n), dc.get(n)["pose_init"])


def test_pivot_keys_take_every_lu_step_both_ways():
    trs = []
    for key in PIVOT_KEYS:
        _, stats, _ = dc.walk_levels(dc.get(key))
        for lv in range(dc.LEVELS):
            H = stats[lv][2:38]
            assert np.isfinite(H).all(), (key, lv)
            trs.append(partial_piv_lu_transpositions(H))
    assert len(trs) == 20
    print("transposition vectors:", sorted(set(trs)))
    for k in range(5):
        assert any(tr[k] != k for tr in trs), f"LU step {k} never swaps rows"
        assert any(tr[k] == k for tr in trs), f"LU step {k} always swaps rows"


def _rel_frob(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


_fast_ctx: dict = {}


def _direct_pose(key, fast):
    import viso_amd
    c = dc.get(key)
    if not fast:
        ctx = viso_amd.default_context(K=c["K"])
    else:
        ctx = _fast_ctx.get(c["K"])
        if ctx is None:
            K = c["K"]
            ctx = viso_amd.Context(viso_amd.default_params(fx=K[0], fy=K[1], cx=K[2], cy=K[3],
                                                           precision=viso_amd.PRECISION_FAST))
            _fast_ctx[K] = ctx
    return ctx.direct_pose(c["last"], c["cur"], c["w"], c["h"], c["points"], c["pose_last"], c["pose_init"])


@pytest.mark.gpu
@pytest.mark.parametrize("key", SIZES + PIVOT_KEYS)
def test_gpu_direct_prologue_against_oracle(key):
    exp = dc.oracle_pose(key)
    got = _direct_pose(key, False)
    rel = _rel_frob(got, exp)
    print(f"direct pose {key} faithful: rel Frobenius {rel:.3e} (bar 1e-12)")
    assert np.isfinite(got).all() and rel < 1e-12, f"{key}: rel {rel:.3e}\n" + dc.format_census(dc.census(key))


def _parent_params():
    out = []
    for key in PARENT_KEYS:
        out.append((key, False))
        if fast_admitted(key):
            out.append((key, True))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("key,fast", _parent_params())
def test_gpu_direct_prologue_bits_of_the_parent(key, fast):
    with np.load(GOLDEN) as g:
        exp = g[golden_name(key, fast)]
    assert exp.dtype == np.uint64 and exp.shape == (12,)
    got = np.ascontiguousarray(_direct_pose(key, fast), np.float64).reshape(12).view(np.uint64)
    diff = np.flatnonzero(got != exp)
    print(f"direct pose {key} {'fast' if fast else 'faithful'}: {len(diff)} of 12 doubles differ from the parent's bits")
    assert len(diff) == 0, (key, fast, [(int(i), hex(int(got[i])), hex(int(exp[i]))) for i in diff])
