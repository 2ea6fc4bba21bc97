"""The row exchanges of the direct pose's 6 x 6 PartialPivLU
(viso_amd/csrc/direct_solve.hpp, solve_wave0_rep): every (LU step k, pivot row
p) pair in front of the product's solve.

* CPU: a seeded generator of SPD matrices H = J^T J (40 rows, columns mixed by
  I + 0.8 N(0, 1), column scales a random permutation of 10^(0, 0.5, ..., 2.5),
  condition number < 1e10); a numpy PartialPivLU in Eigen's order (the first
  maximal |pivot| wins, as tests/pose_refine_ref.inverse6); the first draws
  that add a new (k, p) pair are kept, and the kept set covers all 20 pairs
  (k = 0..4, p = k..5).  One all-zero H takes the `best == 0` path.
  All arithmetic of the generator is plain Python floats in a fixed order, so
  the matrices are the same bits on every machine;
  tests/golden/direct_lu_swaps.txt holds them (hex floats, 28 sums per line)
  for tools/ubench/solve_bench.hip, and a CPU test holds the file to the
  generator.
* GPU: on every kept matrix with a random b, the six `update` doubles of the
  stage entry viso_direct_solve (one wave running the product's faithful
  solve_wave0) equal the numpy restatement bit for bit: LU, then column-wise
  forward and backward substitution, then row-wise H^-1 b with ascending
  columns, as solve_after_lu states it.  The zero matrix gives a NaN update
  and the unchanged state.
"""
import os

import numpy as np
import pytest

SEED = 19
MAX_DRAWS = 64
ALL_PAIRS = frozenset((k, p) for k in range(5) for p in range(k, 6))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "direct_lu_swaps.txt")
STATE = (0.01, -0.02, 0.005, 0.9997, 0.3, -0.1, 1.2)
N_GOOD = 1000


def _div(a, b):
    """IEEE division (a zero divisor gives inf / nan instead of raising)."""
    return float(np.float64(a) / np.float64(b))


def partial_piv_lu(H):
    """Eigen's PartialPivLU of a 6 x 6 H (row-major list of 36): (lu, tr), unit
    L below the diagonal, U on and above, tr[k] the row exchanged with row k."""
    lu = [float(v) for v in H]
    tr = [0] * 6
    for k in range(6):
        p, best = k, abs(lu[7 * k])
        for i in range(k + 1, 6):
            s = abs(lu[6 * i + k])
            if s > best:
                best, p = s, i
        tr[k] = p
        if best != 0.0:
            if p != k:
                for j in range(6):
                    lu[6 * k + j], lu[6 * p + j] = lu[6 * p + j], lu[6 * k + j]
            for i in range(k + 1, 6):
                lu[6 * i + k] = _div(lu[6 * i + k], lu[7 * k])
        for i in range(k + 1, 6):
            for j in range(k + 1, 6):
                lu[6 * i + j] = lu[6 * i + j] - lu[6 * i + k] * lu[6 * k + j]
    return lu, tr


def solve_update(H, b):
    """update = H^-1 b as solve_after_lu computes it: column c of the inverse by
    forward (unit L) and backward (U) substitution on column c of P * I, then
    row r's dot product with b over ascending columns."""
    lu, tr = partial_piv_lu(H)
    with np.errstate(all="ignore"):
        inv = [[0.0] * 6 for _ in range(6)]
        for c in range(6):
            pos = c
            for k in range(6):
                if pos == k:
                    pos = tr[k]
                elif pos == tr[k]:
                    pos = k
            x = [np.float64(1.0 if r == pos else 0.0) for r in range(6)]
            for j in range(6):
                for i in range(j + 1, 6):
                    x[i] = x[i] - np.float64(lu[6 * i + j]) * x[j]
            for j in range(5, -1, -1):
                x[j] = x[j] / np.float64(lu[7 * j])
                for i in range(j):
                    x[i] = x[i] - np.float64(lu[6 * i + j]) * x[j]
            for r in range(6):
                inv[r][c] = x[r]
        out = []
        for r in range(6):
            s = inv[r][0] * np.float64(b[0])
            for c in range(1, 6):
                s = s + inv[r][c] * np.float64(b[c])
            out.append(float(s))
    return np.array(out, np.float64), tuple(tr)


def draw_spd(rng):
    """One H = J^T J (row-major list of 36, exactly symmetric) and a b (6)."""
    G = rng.standard_normal((40, 6)).tolist()
    M = (np.eye(6) + 0.8 * rng.standard_normal((6, 6))).tolist()
    scales = [10.0 ** (0.5 * int(e)) for e in rng.permutation(6)]
    b = rng.standard_normal(6).tolist()
    J = [[0.0] * 6 for _ in range(40)]
    for r in range(40):
        for c in range(6):
            s = 0.0
            for m in range(6):
                s = s + G[r][m] * M[m][c]
            J[r][c] = s * scales[c]
    H = [0.0] * 36
    for i in range(6):
        for j in range(i, 6):
            s = 0.0
            for r in range(40):
                s = s + J[r][i] * J[r][j]
            H[6 * i + j] = H[6 * j + i] = s
    return H, [v * scales[i] for i, v in enumerate(b)]


_kept = None


def kept_inputs():
    """[(H, b, pairs added)]: the first draws that add a new (step, pivot row)
    pair, computed once."""
    global _kept
    if _kept is None:
        rng = np.random.default_rng(SEED)
        seen, kept, draws = set(), [], 0
        while seen != ALL_PAIRS and draws < MAX_DRAWS:
            H, b = draw_spd(rng)
            draws += 1
            if not np.linalg.cond(np.array(H).reshape(6, 6)) < 1e10:
                continue
            _, tr = partial_piv_lu(H)
            new = {(k, tr[k]) for k in range(5)} - seen
            if new:
                seen |= new
                kept.append((H, b, sorted(new)))
        _kept = (kept, draws, seen)
    return _kept


def sums_of(H, b, cost=1234.5):
    """The 28 canonical sums: H's upper triangle row-major, b, the cost sum."""
    return [H[6 * r + c] for r in range(6) for c in range(r, 6)] + list(b) + [cost]


def golden_lines():
    kept, _, _ = kept_inputs()
    rows = [sums_of(H, b) for H, b, _ in kept] + [sums_of([0.0] * 36, kept[0][1])]
    return [" ".join(float(v).hex() for v in row) for row in rows]


def test_kept_matrices_cover_every_step_and_pivot_row():
    kept, draws, seen = kept_inputs()
    print(f"{len(kept)} matrices out of {draws} draws; pairs per matrix: {[k[2] for k in kept]}")
    assert seen == ALL_PAIRS, sorted(ALL_PAIRS - seen)
    for H, _, _ in kept:
        A = np.array(H).reshape(6, 6)
        assert np.array_equal(A, A.T) and np.linalg.cond(A) < 1e10
        assert np.linalg.eigvalsh(A).min() > 0


def test_restated_solve_is_a_solve():
    """The restatement solves H x = b (to the conditioning), so a bit match
    with it is a match with the right thing."""
    for H, b, _ in kept_inputs()[0]:
        x, _ = solve_update(H, b)
        A = np.array(H).reshape(6, 6)
        ref = np.linalg.solve(A, np.array(b))
        rel = np.linalg.norm(x - ref) / np.linalg.norm(ref)
        assert rel < 1e-16 * 64 * np.linalg.cond(A), rel


def test_golden_file_is_the_generators():
    with open(GOLDEN) as fh:
        lines = [l.strip() for l in fh if l.strip() and not l.startswith("#")]
    assert lines == golden_lines()


_ctx = None


def _solve(H, b):
    global _ctx
    import viso_amd
    if _ctx is None:
        _ctx = viso_amd.default_context()
    return _ctx.direct_solve(sums_of(H, b), N_GOOD, STATE)


def _cases():
    return list(range(len(kept_inputs()[0])))


@pytest.mark.gpu
@pytest.mark.parametrize("idx", _cases())
def test_gpu_update_bits_on_every_pivot_row(idx):
    H, b, pairs = kept_inputs()[0][idx]
    exp, tr = solve_update(H, b)
    stats, state = _solve(H, b)
    got = stats[44:50]
    diff = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    print(f"matrix {idx}: transpositions {tr}, new pairs {pairs}, {len(diff)} of 6 update doubles differ")
    assert np.isfinite(exp).all()
    assert np.array_equal(stats[2:38], np.array(H)) and np.array_equal(stats[38:44], np.array(b))
    assert stats[0] == N_GOOD and stats[1] == 1234.5 / N_GOOD
    assert len(diff) == 0, (idx, tr, [(int(i), float(got[i]).hex(), float(exp[i]).hex()) for i in diff])
    assert np.isfinite(state).all() and not np.array_equal(state, np.array(STATE))


@pytest.mark.gpu
def test_gpu_zero_matrix_gives_nan_update_and_keeps_the_state():
    b = kept_inputs()[0][0][1]
    exp, tr = solve_update([0.0] * 36, b)
    assert tr == (0, 1, 2, 3, 4, 5) and np.isnan(exp).all()
    stats, state = _solve([0.0] * 36, b)
    assert np.isnan(stats[44:50]).all(), stats[44:50]
    assert np.array_equal(state, np.array(STATE))


if __name__ == "__main__":  # rewrite the fixture: python -m tests.test_direct_lu_swaps
    with open(GOLDEN, "w") as fh:
        fh.write("# tests/test_direct_lu_swaps.py: 28 sums per line (H upper triangle, b, cost), hex floats\n")
        fh.write("\n".join(golden_lines()) + "\n")
    print(GOLDEN, len(golden_lines()), "rows")
