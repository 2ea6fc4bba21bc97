"""FAST on the frame path (Viso::OnNewFrame's detection frames, src/viso.cpp:
100-108): the tiles fused into the one-frame chunk's level-1 launch, the
tiles run by the detection frame itself in a longer chunk, the count capped at
max_features, kp2 = kp1, and a re-detection into the scratch block of a denser
frame — at small odd sizes, against the oracle's FAST list and its Viso.
tests/test_fast_patterns.py pins the references on the CPU."""
import numpy as np
import pytest

from tests import fast_patterns as fp
from tests import images, oracle_lib

pytestmark = pytest.mark.gpu

K = (517.3, 516.5, 325.1, 249.7)
SIZES = [(43, 253, 270), (19, 129, 54)]  # h, w, corners of images.mixed(seed 4) at threshold 20
THRESH = 20


def _kp(img, thresh=THRESH):
    xs, ys, _ = oracle_lib.fast(img, thresh)
    return np.stack([xs, ys], 1).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _viso(h, w, **kw):
    import viso_amd
    return viso_amd.Viso(*K, width=w, height=h, fast_thresh=THRESH, **kw)


def _device_chunk(v, frames):
    import torch
    d = torch.from_numpy(np.stack(frames)).cuda()
    torch.cuda.synchronize()
    v.process_device(d.data_ptr(), None, len(frames), frames[0].size)
    v.synchronize()
    del d


@pytest.mark.parametrize("h,w,n", SIZES)
def test_gpu_detection_frame_fused_tiles(h, w, n):
    img = images.mixed(h, w, seed=4)
    exp = _kp(img)
    assert len(exp) == n
    v = _viso(h, w)
    try:
        v.OnNewFrame(img)
        k1, k2, s = v.tracks()
    finally:
        v.close()
    assert k1.shape == (n, 2)
    assert np.array_equal(_bits(k1), _bits(exp))
    assert np.array_equal(_bits(k2), _bits(k1))
    assert s.shape == (n,) and not s.any()


@pytest.mark.parametrize("cap", [37, 64])
@pytest.mark.parametrize("h,w,n", SIZES[:1])
def test_gpu_detection_frame_max_features(h, w, n, cap):
    """The oracle's Viso does not cap: the first max_features corners in
    row-major order, and that count."""
    img = images.mixed(h, w, seed=4)
    exp = _kp(img)
    assert len(exp) == n > cap
    v = _viso(h, w, max_features=cap)
    try:
        v.OnNewFrame(img)
        k1, k2, s = v.tracks()
    finally:
        v.close()
    assert k1.shape == (cap, 2)
    assert np.array_equal(_bits(k1), _bits(exp[:cap]))
    assert np.array_equal(_bits(k2), _bits(k1))
    assert not s.any()


@pytest.mark.parametrize("h,w,n", SIZES)
def test_gpu_detection_frame_unfused_tiles(h, w, n):
    """A chunk of two frames of one image: the detection frame runs its own
    tiles, the second frame tracks its corners."""
    img = images.mixed(h, w, seed=4)
    ov = oracle_lib.Viso(K, w, h, fast_thresh=THRESH)
    ov.on_new_frame(img)
    assert len(ov.tracks()[0]) == n
    ov.on_new_frame(img)
    e1, e2, es = ov.tracks()
    assert 0 < len(e1) <= n
    v = _viso(h, w)
    try:
        _device_chunk(v, [img, img])
        k1, k2, s = v.tracks()
    finally:
        v.close()
    assert k1.shape == e1.shape
    assert np.array_equal(_bits(k1), _bits(e1))
    assert np.array_equal(_bits(k2), _bits(e2))
    assert np.array_equal(s, es)


@pytest.mark.parametrize("chunked", [False, True])
def test_gpu_redetection_into_used_scratch(chunked):
    """reinitialize_after = 0 makes every frame a detection frame: a sparse
    frame after a dense one, through the fused launch (one frame at a time) and
    through the frames' own tiles (one chunk)."""
    h, w = 43, 253
    dense = fp.full_slots(h, w, 1)
    sparse = fp.seams(h, w)[0]
    nd, ns = len(_kp(dense)), len(_kp(sparse))
    assert fp.slot_counts(*oracle_lib.fast(dense, THRESH)[:2], h, w).max() == 62  # (all 62 odd candidate columns of a tile)
    assert 0 < ns < nd // 20
    ov = oracle_lib.Viso(K, w, h, fast_thresh=THRESH, reinitialize_after=0)
    v = _viso(h, w, reinitialize_after=0)
    try:
        if chunked:
            ov.on_new_frame(dense)
            ov.on_new_frame(sparse)
            _device_chunk(v, [dense, sparse])
            k1, k2, s = v.tracks()
        else:
            ov.on_new_frame(dense)
            v.OnNewFrame(dense)
            k1, k2, s = v.tracks()
            assert np.array_equal(_bits(k1), _bits(_kp(dense))) and np.array_equal(_bits(k2), _bits(k1))
            ov.on_new_frame(sparse)
            v.OnNewFrame(sparse)
            k1, k2, s = v.tracks()
    finally:
        v.close()
    e1, e2, es = ov.tracks()
    assert np.array_equal(_bits(e1), _bits(_kp(sparse)))
    assert k1.shape == (ns, 2)
    assert np.array_equal(_bits(k1), _bits(e1))
    assert np.array_equal(_bits(k2), _bits(e2))
    assert np.array_equal(s, es) and not s.any()
