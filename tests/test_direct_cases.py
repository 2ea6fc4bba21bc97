"""The inputs of tests/test_direct_branches.py reach every branch of the
direct-pose kernel (CPU; the census of tests/direct_cases.py, oracle only).

These are conditions on the inputs, not tolerances: every sampling class of
direct_cases' branch map holds at least 8 good points at some level of some
case; each edge class holds 8 at every level 0-3 of one case; each
prediction-miss class holds 8 at a level <= 2 (where the window was predicted
by a solved level); every case is usable (the oracle's update is finite at
all four levels and the pose moves off the seed); and the lists admitted to
the tolerance-mode leg are exactly those inside the conditioning rule.

Census of the committed cases: good points per class at levels 0 / 1 / 2 / 3
(classes that stay empty in a case are left out; max cond(H) over the levels).

  gentle    320x240 (3,2) n=2465 T=10          cond 20
    good 2263/2127/1856/1435   shared 1337/813/281/19   straddle 897/1221/1393/1014
    per_sample 29/93/182/402   edge_lt 0/2/11/103   edge_r 4/11/18/31   edge_b 10/21/36/74
  small_l3  320x152 (16,0) n=4097 T=17         cond 26
    good 3509/3249/2767/1906   shared 1793/766/149/0   straddle 1647/2260/2203/0
    per_sample 69/223/415/0   edge_lt 6/53/94/0   edge_r 8/17/39/0   edge_b 15/35/89/0
    win_off 0/0/0/1906 (level 3 is 40x19)
  odd_t64   333x251 (20,-12) n=16384 T=64      cond 19
    good 15265/14297/12495/9543   shared 9433/5887/2113/159   straddle 5543/7773/9016/6776
    per_sample 289/637/1366/2608   edge_lt 30/63/236/656   edge_r 48/100/159/303
    edge_b 67/122/247/400
  big_step  640x480 (64,0) scale 128 near 0.5 n=3321 T=13   cond 18
    good 2848/2791/2722/2586   shared 1890/0/0/420   straddle 418/0/0/1838
    per_sample 540/2791/2722/328   edge_lt 2/2/5/85   edge_r 3/3/21/32   edge_b 2/5/11/49
    partial_miss 212/2788/2684/0   full_miss 0/3/38/0   prediction error up to 17.3 px
  big_step_far  the same pair, near 0           cond 800
    good 2897/2843/2749/2586   shared 1934/0/0/420   straddle 391/0/0/1838
    per_sample 572/2843/2749/328   edge_lt 2/2/0/85   edge_r 4/8/16/32   edge_b 2/3/8/49
    partial_miss 226/2783/2639/0   full_miss 0/19/110/0   prediction error up to 18.2 px
  near_pts  320x240 (56,0) seed 3 scale 128 near 0.05 n=3321 T=13   cond 190
    good 2440/2328/2159/1924   shared 1058/397/0/16   straddle 272/92/1/1341
    per_sample 1110/1839/2158/567   edge_lt 7/10/17/156   edge_r 9/10/27/60   edge_b 1/8/39/108
    partial_miss 385/1501/2108/0   full_miss 2/0/44/0   prediction error up to 22.3 px
  wide      1242x375 (5,-3) seed 1 scale 16 n=2465 T=10     cond 17
    good 2360/2292/2131/1899   shared 1777/1386/798/180   straddle 565/872/1253/1468
    per_sample 18/34/80/251   edge_lt 10/13/17/72   edge_r 1/2/9/11   edge_b 0/0/5/45
  tile sweep 320x240 (3,2) near 0.5: n (T) = 3, 12, 13, 255, 256 (1), 257 (2), 2300 (9),
    2465 (10), 3070 (12), 3321 (13), 4090 (16), 4100 (17), 4600 (18), 4860 (19), 16100 (63),
    16300, 16384 (64); cond 18.5 - 19.8 from n = 255 up.

Every class holds >= 8 somewhere; edge_lt, edge_r and edge_b hold >= 8 at every
level of odd_t64 (edge_b also of gentle); partial_miss and full_miss hold >= 8
at level 2 of big_step, big_step_far and near_pts.

cond(H) ceiling (the oracle on the inputs of test_gpu_direct_pose, steps 1 and
2, all four levels): 50.926 (level 3 of step 1), kept as
direct_cases.COND_CEILING = 50.93.  Outside the rule, so not run in tolerance
mode: big_step_far (cond 800), near_pts (190), and the tile sweep's n = 3
(1.2e4), n = 12 (63.7) and n = 13 (54.2).
"""
import numpy as np
import pytest

from tests import direct_cases as dc
from tests import seqdata

MIN = 8
EDGES = ("edge_lt", "edge_r", "edge_b")
MISSES = ("partial_miss", "full_miss")


@pytest.mark.parametrize("cls", [c for c in dc.CLASSES])
def test_every_class_is_populated(cls):
    best = max(max(dc.census(name)[cls]) for name in dc.CASES)
    assert best >= MIN, (cls, best)


@pytest.mark.parametrize("cls", EDGES)
def test_edge_classes_at_every_level_of_one_case(cls):
    per_case = {name: min(dc.census(name)[cls]) for name in dc.CASES}
    assert max(per_case.values()) >= MIN, (cls, per_case)


@pytest.mark.parametrize("cls", MISSES)
def test_miss_classes_below_level_3(cls):
    best = max(max(dc.census(name)[cls][:3]) for name in dc.CASES)
    assert best >= MIN, (cls, best)


@pytest.mark.parametrize("key", list(dc.CASES) + list(dc.SWEEP_N))
def test_case_is_usable(key):
    cen = dc.census(key)
    assert all(cen["update_finite"]), (key, cen["update_finite"])
    assert cen["moved"], key
    assert not np.array_equal(dc.oracle_pose(key), dc.get(key)["pose_init"])


def test_sweep_pins_the_tile_sizes():
    tiles = [dc.map_tile(n) for n in dc.SWEEP_N]
    assert set(tiles) >= {1, 2, 9, 10, 12, 13, 16, 17, 18, 19, 63, 64}
    for n, t in zip(dc.SWEEP_N, tiles):
        if t >= 9 and n != 16384:
            assert 256 * (t - 1) < n <= 256 * t and n % t != 0, (n, t)  # a partial last tile
    assert {3, 12, 13, 255, 256, 257, 16384} <= set(dc.SWEEP_N)


def test_wide_case_straddles_512_and_1024():
    c = dc.case("wide")
    start, _, _ = dc.walk_levels(c)
    m = dc.classify_level(c, 0, start[0], start[1])
    uc, _ = dc._project(start[0], c["K"], np.asarray(c["points"]), 1.0)
    for b in (512.0, 1024.0):
        hit = m["straddle"] & (uc - 6.0 < b) & (uc + 6.0 >= b)
        assert hit.sum() >= MIN, (b, int(hit.sum()))


def test_tolerance_lists_follow_the_conditioning_rule():
    d = seqdata.initialised()
    f0, pose = d["init_frame"], d["kf_poses"][1]
    ceiling = 0.0
    for step in (1, 2):  # test_track.py::test_gpu_direct_pose
        c = dict(last=seqdata.pyramid(f0), cur=seqdata.pyramid(f0 + step), w=seqdata.W, h=seqdata.H, K=d["K"],
                 points=d["points"], pose_last=pose, pose_init=pose)
        ceiling = max(ceiling, max(dc.census_of(c)["cond"]))
    # the committed constant is the measured ceiling, rounded up in the 4th digit
    assert ceiling <= dc.COND_CEILING <= ceiling * 1.001, ceiling
    admitted = tuple(k for k in dc.CASES if max(dc.census(k)["cond"]) <= dc.COND_CEILING)
    assert admitted == dc.FAST_CASES, {k: max(dc.census(k)["cond"]) for k in dc.CASES}
    admitted_n = tuple(n for n in dc.SWEEP_N if max(dc.census(n)["cond"]) <= dc.COND_CEILING)
    assert admitted_n == dc.FAST_SWEEP_N, {n: max(dc.census(n)["cond"]) for n in dc.SWEEP_N}
