"""The direct pose's level partials with four levels of the tile tree taken in
the loads (viso_amd/csrc/direct.hip: partial_index, load_partials_tree16;
common.hpp: reduce_tree16_pairs).

Layout of a level's scratch, [4 waves][16][56][2]: sum k of tile b lies at
double ((b >> 6) * 16 + (b & 15)) * 112 + ((k >> 1) * 4 + ((b >> 4) & 3)) * 2
+ (k & 1).  Wave w of the next launch's prologue owns tiles 64 w .. 64 w + 63;
its lane l < 56 is (g = l & 3, s = l >> 2) and owns sums 2 s and 2 s + 1 of
tiles 64 w + 16 g .. + 15: load instruction j (of sixteen 16-byte loads) brings
both sums of tile 64 w + 16 g + j, and the 56 lanes of one instruction read one
contiguous 896-byte run (lane l at byte 16 l).  A load is issued only for a
tile below n_tiles; the register of an absent tile holds +0.0.  The 16 tiles
of a sum are added in registers in the canonical pairing, then xor 1 on g is a
reduce-scatter step (even g keeps sum 2 s, odd g sum 2 s + 1), xor 2 on g a
butterfly, and the four waves combine as (w0 + w1) + (w2 + w3).

CPU part: a numpy model of the index map, the lane map and that tree.

* every (sum, tile) of 28 x 256 is read exactly once, by the lane and load
  that the tree takes it from, and no load reads a tile at or beyond n_tiles
  (the model's scratch holds NaN there);
* every load instruction's active lanes cover one contiguous run;
* the modelled tree equals, bit for bit, the canonical tree over the 256 tile
  slots (tiles at or beyond n_tiles are +0.0), and the oracle's tree_sum over
  the n_tiles tile sums (oracle/oracle_common.hpp, restated in numpy below:
  neither tests/oracle_lib nor oracle/numpy_ref.py exports it).  tree_sum pads
  to the next power of two, the device to 256 slots: from 129 tiles on the two
  are the same tree; below, the device's adds further +0.0 levels, which
  change nothing but the sign of a -0.0 result, so there the bar is
  bits(model) == bits(tree_sum + 0.0).

GPU part: Context.direct_pose against the oracle (relative Frobenius < 1e-12,
the stage's bar) and against the parent commit's bits
(tests/golden/direct_partial_tree_parent.npz, recorded with the library of the
commit before this layout by tests/golden/make_direct_partial_tree.py) on

* one point per tile at every edge of a lane's 16 tiles and of a wave's 64:
  n in {1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65};
* n = 258 (129 tiles of two points) and the sweep's 255 / 256 / 257;
* the cost == 0 continuation (k-major continuation scratch and the level
  scratch in one launch);
* a 3-frame then a 2-frame process_device call (merged L(3) and standalone F
  read the layout): the frame path's bar, 1e-10, and the parent's bits.
"""
import os

import numpy as np
import pytest

from tests import direct_cases as dc
from tests import test_direct_partials_layout as tl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "direct_partial_tree_parent.npz")

SUMS, TILES, WAVES, LANES = 28, 256, 4, 56
N_TILES = (1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 129, 247, 255, 256)

EDGE_MAKE = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 258)
EDGE_SWEEP = (255, 256, 257)
KEYS = tuple(f"n{n}" for n in EDGE_MAKE + EDGE_SWEEP) + ("repeat",)


# ------------------------------------------------------------------ the model

def partial_index(k, b):
    """direct.hip partial_index<true>: the double of sum k of tile b."""
    return (((b >> 6) * 16 + (b & 15)) * LANES + ((k >> 1) * 4 + ((b >> 4) & 3))) * 2 + (k & 1)


def load_address(w, lane, j):
    """First double of the 16-byte load j of lane `lane` in wave w."""
    return ((w * 16 + j) * LANES + lane) * 2


def lane_owns(w, lane, j):
    """(sum of .x, sum of .y, tile) that load j of the lane brings."""
    g, s = lane & 3, lane >> 2
    return 2 * s, 2 * s + 1, 64 * w + 16 * g + j


def scatter(values, n_tiles):
    """The producer side: values[k, b] of tiles < n_tiles stored through
    partial_index into a scratch that holds NaN everywhere else."""
    scratch = np.full(SUMS * TILES, np.nan)
    for b in range(n_tiles):
        for k in range(SUMS):
            scratch[partial_index(k, b)] = values[k, b]
    return scratch


def model_tree(scratch, n_tiles):
    """The prologue's reduction of one level as the kernel forms it: 28 sums."""
    red = np.zeros((WAVES, SUMS))
    with np.errstate(all="ignore"):
        for w in range(WAVES):
            a = np.zeros((64, 2))  # per lane: sums 2 s and 2 s + 1 over its 16 tiles
            for lane in range(LANES):
                m = n_tiles - (64 * w + 16 * (lane & 3))
                x = np.zeros((16, 2))  # an absent tile's register pair: +0.0
                for j in range(16):
                    if j < m:
                        p = load_address(w, lane, j)
                        x[j] = scratch[p:p + 2]
                st = 1
                while st < 16:
                    for j in range(0, 16, 2 * st):
                        x[j] = x[j] + x[j + st]
                    st *= 2
                a[lane] = x[0]
            c = np.zeros(64)
            for lane in range(64):  # xor 1 on g: even g keeps sum 2 s, odd g sum 2 s + 1
                e = lane & 1
                c[lane] = a[lane, e] + a[lane ^ 1, e]
            d = np.array([c[lane] + c[lane ^ 2] for lane in range(64)])  # xor 2 on g
            for lane in range(LANES):
                if not lane & 2:
                    red[w, 2 * (lane >> 2) + (lane & 1)] = d[lane]
        return (red[0] + red[1]) + (red[2] + red[3])


def tree_sum(v):
    """oracle_common.hpp tree_sum over axis 0: the leaves padded with +0.0 to
    the next power of two, neighbours first."""
    n = v.shape[0]
    p = 1
    while p < n:
        p <<= 1
    t = np.concatenate([v, np.zeros((p - n,) + v.shape[1:])])
    with np.errstate(all="ignore"):
        while t.shape[0] > 1:
            t = t[0::2] + t[1::2]
    return t[0]


def random_values(seed):
    """[28][256] fp64: mixed signs over 40 binades, -0.0, +0.0 and denormals
    sprinkled in; sum 5 is -0.0 in every tile and sum 6 denormal in every tile."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((SUMS, TILES)) * np.exp2(rng.integers(-20, 20, (SUMS, TILES)))
    r = rng.random((SUMS, TILES))
    v[r < 0.06] = -0.0
    v[(r >= 0.06) & (r < 0.09)] = 0.0
    den = (r >= 0.09) & (r < 0.15)
    v[den] = (rng.integers(1, 1 << 30, (SUMS, TILES)) * 5e-324 * rng.choice([-1.0, 1.0], (SUMS, TILES)))[den]
    v[5] = -0.0
    v[6] = rng.integers(1, 1 << 20, TILES) * 5e-324 * rng.choice([-1.0, 1.0], TILES)
    return v


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------ CPU tests

def test_every_sum_of_every_tile_is_read_once_where_the_tree_takes_it():
    seen = np.zeros(SUMS * TILES, np.int64)
    for w in range(WAVES):
        for lane in range(LANES):
            for j in range(16):
                p = load_address(w, lane, j)
                kx, ky, b = lane_owns(w, lane, j)
                assert p == partial_index(kx, b) and p + 1 == partial_index(ky, b), (w, lane, j)
                seen[p:p + 2] += 1
    assert (seen == 1).all()
    idx = np.array([[partial_index(k, b) for b in range(TILES)] for k in range(SUMS)])
    assert np.array_equal(np.sort(idx.ravel()), np.arange(SUMS * TILES))


def test_each_load_instruction_reads_one_contiguous_run():
    for w in range(WAVES):
        for j in range(16):
            byte = np.array([8 * load_address(w, lane, j) for lane in range(LANES)])
            assert np.array_equal(byte - byte[0], 16 * np.arange(LANES)), (w, j)  # 896 bytes, lane l at 16 l
            assert byte[0] % 128 == 0  # a run starts on a cache line


def test_tile_counts_of_the_gpu_cases():
    got = [(tl.n_tiles(n), dc.map_tile(n)) for n in EDGE_MAKE + EDGE_SWEEP]
    assert got == [(n, 1) for n in EDGE_MAKE[:-1]] + [(129, 2), (255, 1), (256, 1), (129, 2)]


@pytest.mark.parametrize("n_tiles", N_TILES)
def test_modelled_tree_is_the_canonical_tree_bit_for_bit(n_tiles):
    for seed in (0, 1):
        v = random_values(seed + 10 * n_tiles)
        got = model_tree(scatter(v, n_tiles), n_tiles)
        assert not np.isnan(got).any()  # nothing at or beyond n_tiles was read
        slots = np.zeros((TILES, SUMS))
        slots[:n_tiles] = v[:, :n_tiles].T
        want256 = tree_sum(slots)
        assert np.array_equal(bits(got), bits(want256)), n_tiles
        oracle = tree_sum(np.ascontiguousarray(v[:, :n_tiles].T))
        want = oracle if n_tiles > 128 else oracle + 0.0
        assert np.array_equal(bits(got), bits(want)), n_tiles
        assert np.array_equal(got, oracle)
        # the all -0.0 sum: -0.0 only where no slot is a pad
        assert bits(got[5:6])[0] == (0x8000000000000000 if n_tiles == TILES else 0)


# ------------------------------------------------------------------ GPU tests

def make_cases():
    out = {}
    w, h, shift, seed, scale, near = dc.SWEEP_ARGS
    for n in EDGE_MAKE:
        out[f"n{n}"] = dc.make(w, h, shift, n, seed, scale, near)
    for n in EDGE_SWEEP:
        out[f"n{n}"] = dc.get(n)
    out["repeat"] = dc.make(w, h, (0, 0), tl.REPEAT_N, seed, scale, near)
    return out


@pytest.fixture(scope="module")
def cases():
    return make_cases()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_gpu_direct_pose_against_oracle_and_parent_bits(key, cases, golden):
    c = cases[key]
    exp = tl.oracle_pose(c, "partial_tree_" + key)
    got = np.ascontiguousarray(tl.direct_pose(c), np.float64).reshape(12)
    par = golden[key]
    rel = tl._rel(got, exp)
    diff = np.flatnonzero(got.view(np.uint64) != par)
    print(f"direct pose {key}: rel Frobenius vs oracle {rel:.3e} (bar 1e-12); {len(diff)} of 12 doubles differ "
          f"from the parent's bits")
    assert np.isfinite(got).all() and rel < 1e-12, (key, rel)
    assert len(diff) == 0, (key, [(int(i), hex(int(got.view(np.uint64)[i])), hex(int(par[i]))) for i in diff])


@pytest.mark.gpu
def test_gpu_three_then_two_frame_calls_against_oracle_and_parent_bits(golden):
    from tests import oracle_lib, seqdata
    got, lefts, rights = tl.two_frame_poses()
    seq = seqdata.sequence(0)
    ov = oracle_lib.Viso(seq.K, seqdata.W, seqdata.H, enable_tracking=1)
    ov.set_stereo(seq.p.baseline, 128, 1)
    for k in range(tl.FRAMES):
        ov.on_new_stereo(lefts[k], rights[k])
    exp = ov.poses()
    par = golden["two_frame"]
    assert got.shape == exp.shape and len(exp) == tl.FRAMES - 1
    rel = tl._rel(got, exp)
    ndiff = int((got.view(np.uint64).ravel() != par.ravel()).sum())
    print(f"3 + 2 frame calls: rel Frobenius vs oracle {rel:.3e} (bar 1e-10); {ndiff} of {got.size} doubles differ "
          f"from the parent's bits")
    assert rel < 1e-10
    assert ndiff == 0
