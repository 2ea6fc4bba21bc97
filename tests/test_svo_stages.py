"""GPU parity of the stereo VO matching and motion stages (viso_amd/csrc/svo.hip)
with the spec (oracle/oracle_svo.cpp) on the crafted cases of tests/svo_cases.py:
SAD ties, candidate lists of 64..400, 8-band windows, window clamps, empty
sets and index 32767 for `best_match` / `svo_circle_kernel`; every tree shape
of `svo_refine_kernel` from 6 to 8000 matches, the spec's failure exits and
the capacity refusals for the motion stage.  Integers and fp64 in a fixed
order: everything is compared exactly.  What each case reaches is proven on
the CPU by tests/test_svo_cases.py; a failure here prints that census line."""
from __future__ import annotations

import numpy as np
import pytest

from tests import oracle_lib as ol
from tests import svo_cases as sc
from tests.test_svo_cases import (MATCH_CASES, MOTION_CASES, census_line, match_params, motion_census_line,
                                  spec_motion)

pytestmark = pytest.mark.gpu

IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


@pytest.fixture(scope="module")
def contexts():
    """One VisualOdometryStereo per distinct parameter set, made on first use."""
    from viso_amd import svo
    made = {}

    def get(w, h, kw):
        key = (w, h) + tuple(sorted(kw.items()))
        if key not in made:
            made[key] = svo.VisualOdometryStereo(svo.default_params(w, h, *sc.K, **kw))
        return made[key]

    yield get
    for vo in made.values():
        vo.close()


@pytest.mark.parametrize("case", MATCH_CASES, ids=repr)
def test_gpu_match_case(contexts, case):
    vo = contexts(case.w, case.h, case.kw)
    exp = ol.svo_match(case.f4, case.h, match_params(case))
    got = vo.match(case.f4)
    assert np.array_equal(got, exp), census_line(case)


@pytest.mark.parametrize("case", [c for c in MOTION_CASES if not c.refused], ids=repr)
def test_gpu_estimate_case(contexts, case):
    vo = contexts(*sc.MOTION_CONTEXTS[case.ctx])
    m_exp, inl_exp, n_exp, _ = spec_motion(case)
    m_got, inl_got, n_got = vo.estimate(case.uv8, case.frame)
    line = motion_census_line(case)
    assert n_got == n_exp, line
    assert np.array_equal(inl_got, inl_exp), (int(inl_got.sum()), int(inl_exp.sum()), line)
    assert np.array_equal(m_got, m_exp), line  # fp64, same expression order: bit-exact
    if n_exp < 0:
        assert np.array_equal(m_got, IDENTITY) and not inl_got.any(), line


@pytest.mark.parametrize("case", [c for c in MOTION_CASES if c.refused], ids=repr)
def test_gpu_estimate_refuses_over_capacity(contexts, case):
    """One match more than buckets x bucket_max: refused, and the context
    still answers the largest accepted size afterwards."""
    from viso_amd._lib import ERRORS, VisoError
    vo = contexts(*sc.MOTION_CONTEXTS[case.ctx])
    assert len(case.uv8) == sc.MOTION_MCAP[case.ctx] + 1
    with pytest.raises(VisoError) as e:
        vo.estimate(case.uv8, case.frame)
    assert ERRORS[e.value.rc] == case.refused
    full = next(c for c in MOTION_CASES if c.ctx == case.ctx and len(c.uv8) == sc.MOTION_MCAP[case.ctx])
    m_exp, inl_exp, n_exp, _ = spec_motion(full)
    m_got, inl_got, n_got = vo.estimate(full.uv8, full.frame)
    assert n_got == n_exp and np.array_equal(inl_got, inl_exp) and np.array_equal(m_got, m_exp)


def test_gpu_match_refuses_more_than_max_features(contexts):
    """A set longer than max_features is an argument error, not a write past the buffers."""
    from viso_amd._lib import ERRORS, VisoError
    case = next(c for c in MATCH_CASES if c.name == "dense_400")
    vo = contexts(case.w, case.h, case.kw)
    S = case.f4[sc.R2]
    reps = case.kw["max_features"] // len(S) + 1
    big = sc.Feats(np.tile(S.u, reps), np.sort(np.tile(S.v, reps), kind="stable"), np.tile(S.cls, reps),
                   np.tile(S.desc, (reps, 1)))
    assert len(big) > case.kw["max_features"]
    with pytest.raises(VisoError) as e:
        vo.match([case.f4[0], case.f4[1], case.f4[2], big])
    assert ERRORS[e.value.rc] == "VISO_ERR_ARG"
