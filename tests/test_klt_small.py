"""KLT (OpticalFlowMultiLevel, src/viso.cpp:259-391) away from the bench
geometry: images whose upper pyramid levels are smaller than the kernel's
24 x 24 LDS window (so the window is off at some or all levels) or than the
8 x 8 patch (so level 3's bounds test fails for every point), keypoints on and
next to the borders, and track counts that do not fill a workgroup of four.
Positions and success flags agree with the oracle bit for bit."""
import numpy as np
import pytest

from tests import images, oracle_lib

# (h, w): level 3 is 2 x 2, 4 x 2, 12 x 7 and 19 x 5; the window (both sides
# >= 24) is off at every level, at every level, at levels 2-3 and at levels 1-3
SIZES = [(16, 16), (17, 33), (61, 97), (46, 155)]


def _case(h, w):
    """(ref pyramid, cur pyramid, kp1, kp2): cur is ref moved by (1, 2)
    pixels; the first five keypoints are the ones the short track counts use."""
    base = images.smooth(h + 4, w + 4, seed=h + w, scale=5)
    ref = np.ascontiguousarray(base[2:2 + h, 2:2 + w])
    cur = np.ascontiguousarray(base[0:h, 1:1 + w])  # content moves +1 x, +2 y
    cx, cy = w / 2, h / 2
    kp1 = [[cx, cy],                                  # interior
           [0, 0],                                    # a corner of the image
           [4.5, cy],                                 # just inside the bounds test (b > 4)
           [cx + 1, cy - 1],                          # (gets the far guess below)
           [w + 40, h + 40],                          # level-3 patch wholly outside the image
           [w - 1, 0], [0, h - 1], [w - 1, h - 1],    # the other corners
           [3.5, cy], [w - 3.5, cy], [w - 4.5, cy],   # 3.5 / 4.5 from each border
           [cx, 3.5], [cx, 4.5], [cx, h - 3.5], [cx, h - 4.5],
           [cx - 2, cy + 1]]
    kp1 = np.array(kp1, np.float32)
    kp2 = kp1.copy()
    # an initial guess far from the truth (inside the bounds test at level 0 of the two larger sizes,
    # where the 24 x 24 window is placed around the guess and the iterations start there)
    kp2[3] += [w * 0.3, -h * 0.2]
    return oracle_lib.pyramid(ref), oracle_lib.pyramid(cur), kp1, kp2


@pytest.mark.parametrize("h,w", SIZES)
def test_oracle_klt_small_has_successes_and_failures(h, w):
    p0, p1, kp1, kp2 = _case(h, w)
    out, succ = oracle_lib.klt(p0, p1, w, h, kp1, kp2)
    assert succ.any() and not succ.all()
    assert succ[0] == 1 and np.allclose(out[0] - kp1[0], [1, 2], atol=0.5)  # the interior point is tracked
    assert succ[1] == 0 and succ[4] == 0  # the corner and the point outside are not
    # n = 0 is a no-op
    out0, succ0 = oracle_lib.klt(p0, p1, w, h, kp1[:0], kp2[:0])
    assert out0.shape == (0, 2) and succ0.shape == (0,)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SIZES)
def test_gpu_klt_small_bitexact(h, w):
    from viso_amd import default_context
    ctx = default_context()
    p0, p1, kp1, kp2 = _case(h, w)
    for n in [len(kp1), 0, 1, 3, 4, 5]:
        exp_kp, exp_s = oracle_lib.klt(p0, p1, w, h, kp1[:n], kp2[:n])
        got_kp, got_s = ctx.klt(p0, p1, w, h, kp1[:n], kp2[:n])
        assert got_kp.shape == exp_kp.shape == (n, 2)
        assert np.array_equal(got_s, exp_s), n
        assert np.array_equal(got_kp.view(np.uint32), exp_kp.view(np.uint32)), n
        if n == len(kp1):
            assert exp_s.any() and not exp_s.all()
