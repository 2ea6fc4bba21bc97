"""Crafted FAST images whose corner lists can be derived by hand, aimed at the
fixed geometry of the device detector (viso_amd/csrc/image.hip): tiles of 126
output columns x 8 output rows with a one-pixel NMS halo, a per-wave candidate
list of 192 entries scored in 64s, and slots of 64 keypoints per (row, tile).

* ``seams``      — single-pixel dots on a flat background: the four extreme
  candidates, dots just outside the candidate range, and pairs of dots that
  force an NMS decision across every tile seam (x = 126 k) and band seam
  (y = 8 k).  Returns the image and the survivor list derived by hand.
* ``full_slots`` — dots on every 2nd column: 63 survivors per (row, tile), the
  most strict NMS can keep in 126 columns.
* ``full_rows``  — a texture in which every pixel of every other row passes the
  corner test: 128 candidates per tile row, the most a wave's list can get.

tests/test_fast_patterns.py pins, on the oracle alone, that each pattern
reaches the edge it is built for; the GPU cases rely on those pins.
"""
from __future__ import annotations

import numpy as np

from tests import oracle_lib

TILE_COLS = 126   # kFtCols
BAND_ROWS = 8     # kFtRows
SLOT_CAP = 64     # kFtCap
SEAM_BG = 200
SEAM_THRESH = 50


# ---------------------------------------------------------------- seams
# A dot of value v on the flat background B is a 16-of-16 "brighter" corner
# with cornerScore (B - v) - 1 (tests/test_image.py::test_fast_known_answers).
# The circle has radius 3 and NMS looks one pixel around, so dots that are 4
# or more apart (Chebyshev) neither change each other's score nor suppress
# each other; a background pixel sees at most a handful of dark circle pixels,
# never 9 contiguous.  Each group below is therefore decided on its own.
class _Board:
    def __init__(self, h: int, w: int):
        self.h, self.w = h, w
        self.img = np.full((h, w), SEAM_BG, np.uint8)
        self.dots = np.zeros((0, 2), np.int64)
        self.keep: list[tuple[int, int, int]] = []
        self.groups: list[tuple[str, tuple]] = []
        self._k = 0

    def value(self) -> int:
        """Distinct-ish dot values, all with SEAM_BG - v > SEAM_THRESH."""
        self._k += 1
        return (37 * self._k) % 120

    def candidate(self, x: int, y: int) -> bool:
        return 3 <= x <= self.w - 4 and 3 <= y <= self.h - 4

    def free(self, pts, gap: int) -> bool:
        p = np.asarray(pts, np.int64)
        if np.any(p < 0) or np.any(p[:, 0] >= self.w) or np.any(p[:, 1] >= self.h):
            return False
        if len(self.dots) == 0:
            return True
        d = np.abs(self.dots[None, :, :] - p[:, None, :]).max(axis=2)
        return bool(d.min() >= gap)

    def put(self, kind: str, pts, vals, key=()):
        """Place a group; the survivors: every candidate dot that is strictly
        deeper than each other dot of its group within one pixel."""
        for (x, y), v in zip(pts, vals):
            self.img[y, x] = v
        for i, ((x, y), v) in enumerate(zip(pts, vals)):
            if not self.candidate(x, y):
                continue
            rivals = [vals[j] for j, (a, b) in enumerate(pts)
                      if j != i and self.candidate(a, b) and max(abs(a - x), abs(b - y)) <= 1]
            if all(v < r for r in rivals):
                self.keep.append((x, y, SEAM_BG - v - 1))
        self.dots = np.concatenate([self.dots, np.asarray(pts, np.int64)])
        self.groups.append((kind, key))

    def _try(self, gap: int, kind: str, anchors, offsets, depth: str, key=(), need_candidates: bool = True) -> bool:
        for ax, ay in anchors:
            pts = [(ax + dx, ay + dy) for dx, dy in offsets]
            if need_candidates and not all(self.candidate(x, y) for x, y in pts):
                continue
            if not self.free(pts, gap):
                continue
            a = self.value()
            vals = {"single": [a], "first": [a, a + 20], "second": [a + 20, a], "equal": [a, a]}[depth]
            self.put(kind, pts, vals, key)
            return True
        return False

    def place(self, *specs) -> None:
        """Place the groups of `specs` (argument tuples of _try), each at its
        first anchor with room: 8 pixels from every other group if all of them
        fit that way, else 4 (still non-interacting), and then those that fit."""
        specs = [(s[0], list(s[1])) + tuple(s[2:]) for s in specs]
        saved = self.img.copy(), self.dots, list(self.keep), list(self.groups), self._k
        if all([self._try(8, *s) for s in specs]):
            return
        self.img, self.dots, self.keep, self.groups, self._k = saved
        for s in specs:
            self._try(4, *s)


def seams(h: int, w: int):
    """(image, survivors, groups): survivors = the hand-derived (x, y, score)
    list in row-major order at threshold SEAM_THRESH; groups = the (kind, key)
    of every group that found room."""
    b = _Board(h, w)
    xl, xr, yt, yb = 3, w - 4, 3, h - 4
    one, pair_h, pair_v, pair_d = [(0, 0)], [(0, 0), (1, 0)], [(0, 0), (0, 1)], [(0, 0), (1, 1)]
    # the four extreme candidates
    for x, y in [(xl, yt), (xr, yt), (xl, yb), (xr, yb)]:
        b.place(("extreme", [(x, y)], one, "single", (x, y)))
    tile_seams = [X for X in range(TILE_COLS, w, TILE_COLS) if X - 1 >= 3 and X <= w - 4]
    band_seams = [Y for Y in range(BAND_ROWS, h, BAND_ROWS) if Y - 1 >= 3 and Y <= h - 4]
    # one diagonal pair across a tile seam and a band seam at once
    b.place(("both", [(X - 1, Y - 1) for Y in band_seams for X in tile_seams], pair_d, "second"))
    both_x = int(b.dots[-1][0]) if b.groups[-1][0] == "both" else -1  # (its second dot is (X, Y))
    rows = list(range(yt, yb + 1))
    cols = list(range(xl, xr + 1))
    for X in tile_seams:
        # horizontally adjacent: the left one deeper (the right tile must see
        # it in its halo), equal depth (both tiles must see the other), and a
        # diagonal with the right one deeper (the left tile's halo); the pair
        # on both seams is the diagonal of its tile seam
        col = [(X - 1, y) for y in rows]
        specs = [("tile-deeper", col, pair_h, "first", (X,)), ("tile-equal", col, pair_h, "equal", (X,))]
        if X != both_x:
            specs.append(("tile-diagonal", col, pair_d, "second", (X,)))
        b.place(*specs)
    for Y in band_seams:
        row = [(x, Y - 1) for x in cols]
        b.place(("band-deeper", row, pair_v, "first", (Y,)), ("band-equal", row, pair_v, "equal", (Y,)),
                ("band-diagonal", row, pair_d, "second", (Y,)))
    # a corner in the last candidate row / column where the extreme ones had no room
    if not any(y == yb for _, y, _ in b.keep):
        b.place(("edge", [(x, yb) for x in cols], one, "single", ("row",)))
    if not any(x == xr for x, _, _ in b.keep):
        b.place(("edge", [(xr, y) for y in rows], one, "single", ("col",)))
    # one column and one row outside the candidate range: never reported
    b.place(("outside", [(2, y) for y in rows], one, "single", ("left",), False))
    b.place(("outside", [(w - 3, y) for y in rows], one, "single", ("right",), False))
    b.place(("outside", [(x, 2) for x in cols], one, "single", ("top",), False))
    b.place(("outside", [(x, h - 3) for x in cols], one, "single", ("bottom",), False))
    keep = sorted(b.keep, key=lambda k: (k[1], k[0]))
    return b.img, keep, b.groups


# the geometry sweep: widths at height 19, heights at width 131
WIDTHS = [8, 9, 125, 126, 127, 128, 129, 130, 131, 251, 252, 253, 255, 257, 379, 4031, 4032, 4033, 4035, 4096]
HEIGHTS = [8, 9, 10, 11, 12, 15, 16, 17, 18, 19, 20, 23, 25, 33]
SWEEP = [(19, w) for w in WIDTHS] + [(h, 131) for h in HEIGHTS if h != 19]  # (19 x 131 is in both)
# what the smallest sizes have room for, derived by hand: the extreme
# candidates that are 4 apart, a pair across band seam 8 (the deeper, upper dot
# stays) and a single dot in the last candidate row
SMALLEST = {
    (19, 8): [(3, 3, 162), (3, 7, 88), (3, 15, 125)],
    (19, 9): [(3, 3, 162), (3, 7, 88), (3, 15, 125)],
    (8, 131): [(3, 3, 162), (127, 3, 125), (11, 4, 88)],
    (9, 131): [(3, 3, 162), (127, 3, 125), (11, 5, 88)],
    (10, 131): [(3, 3, 162), (127, 3, 125), (11, 6, 88)],
}


def as_arrays(keep):
    k = np.asarray(keep, np.int32).reshape(-1, 3)
    return k[:, 0].copy(), k[:, 1].copy(), k[:, 2].copy()


# ---------------------------------------------------------------- density
FULL_SLOT_THRESH = 50
FULL_ROW_THRESH = 10
DENSE_SHAPE = (43, 381)


def full_slots(h: int, w: int, x0: int, seed: int = 0) -> np.ndarray:
    """Background 230, dots of value [0, 150) on every 4th row from row 4 and
    every 2nd column from x0.  Dots two columns or four rows apart are not on
    each other's circle and not NMS neighbours, so every dot inside the
    candidate range is kept with score 229 - v: 63 per (row, tile) of 126
    columns."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 230, np.uint8)
    ys = np.arange(4, h, 4)
    xs = np.arange(x0, w, 2)
    img[np.ix_(ys, xs)] = rng.integers(0, 150, (len(ys), len(xs)))
    return img


def full_rows(h: int, w: int, seed: int = 0, phase: int = 0) -> np.ndarray:
    """The 2x4 block [[200, 20, 20, 200], [140, 140, 140, 80]] tiled from row
    -phase, with a jitter of +-2 so that the scores differ."""
    rng = np.random.default_rng(seed)
    blk = np.array([[200, 20, 20, 200], [140, 140, 140, 80]], np.int64)
    img = np.tile(blk, (h // 2 + 2, w // 4 + 1))[phase:phase + h, :w]
    return (img + rng.integers(-2, 3, (h, w))).astype(np.uint8)


def score_map(img: np.ndarray, thresh: int) -> np.ndarray:
    """The oracle's score map before NMS (0 = no corner)."""
    h, w = img.shape
    im8 = np.ascontiguousarray(img, np.uint8)
    out = np.zeros(h * w, np.uint8)
    oracle_lib.load().oracle_fast_score_map(im8.ctypes.data, w, h, int(thresh), out.ctypes.data)
    return out.reshape(h, w)


def slot_counts(xs, ys, h: int, w: int) -> np.ndarray:
    """Corners per (row, tile): (h, ntx)."""
    ntx = (w + TILE_COLS - 1) // TILE_COLS
    c = np.zeros((h, ntx), np.int64)
    np.add.at(c, (np.asarray(ys), np.asarray(xs) // TILE_COLS), 1)
    return c


def window_counts(smap: np.ndarray) -> np.ndarray:
    """Non-zero scores per (row, tile) in the tile's 128-column score window
    (output columns 126 t .. 126 t + 125 and one halo column each side)."""
    h, w = smap.shape
    ntx = (w + TILE_COLS - 1) // TILE_COLS
    nz = smap > 0
    c = np.zeros((h, ntx), np.int64)
    for t in range(ntx):
        c[:, t] = nz[:, max(TILE_COLS * t - 1, 0):min(TILE_COLS * t + TILE_COLS + 1, w)].sum(axis=1)
    return c
