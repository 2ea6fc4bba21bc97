// viso_amd — ordered ranks over a workgroup: the building block of every
// stable stream compaction of the map-maintenance kernels (DESIGN.md §Ordered
// compaction).
//
// A workgroup of W waves holds one flag per lane.  A wave ranks its flagged
// lanes by ballot / popcount, lane 0 stores the wave's count in an LDS table of
// W entries, and behind a barrier every lane sums the counts of the waves
// before its own (its offset) and of all waves (the total).  A kernel that
// walks an array in rounds of 64 W rows keeps a running base across rounds:
// row i of the round goes to base + rank, then base += total.  Integer
// arithmetic only, so the order and the counts depend on nothing but the flags.
#pragma once

#include <hip/hip_runtime.h>

namespace viso {

// the flagged lanes of a wave below `lane`
__device__ inline int popc_below(unsigned long long ballot, int lane) {
    return __popcll(ballot & ((1ULL << lane) - 1ULL));
}

// rank: the flagged lanes of the workgroup before this one, in thread order
// (defined for unflagged lanes too); total: the workgroup's flagged lanes
struct BlockRank {
    int rank, total;
};

// Ranks of F flags per lane at once, in two barriers.  EVERY lane of the
// workgroup (W waves, blockDim.x = 64 W) must call it, from uniform control
// flow: it barriers twice, once between the table's writes and its reads and
// once behind the reads, so the table may be written again right after the
// call (the next round's, or another call's).  Whatever a caller reads before
// the call is read before the first barrier, whatever it writes after the call
// is written behind the second: an in-place compaction that loads a round's
// rows before the call and stores them after it is ordered by that alone.
template <int W, int F>
__device__ inline void block_rank(const bool (&flag)[F], int (&table)[F * W], BlockRank (&out)[F]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long b[F];
#pragma unroll
    for (int q = 0; q < F; ++q) {
        b[q] = __ballot(flag[q]);
        if (lane == 0) table[q * W + wave] = __popcll(b[q]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < F; ++q) {
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int t = table[q * W + k];
            before += k < wave ? t : 0;
            total += t;
        }
        out[q].rank = before + popc_below(b[q], lane);
        out[q].total = total;
    }
    __syncthreads();
}

// one flag
template <int W>
__device__ inline BlockRank block_rank(bool flag, int (&table)[W]) {
    const bool f[1] = {flag};
    BlockRank r[1];
    block_rank<W, 1>(f, table, r);
    return r[0];
}

}  // namespace viso
