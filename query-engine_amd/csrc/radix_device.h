// Device-side pieces of the 8-bit radix passes that the kernels of more than one unit use
// (k_sort.hip, k_partition.hip): the tile shape and the stable in-tile ranking.
#pragma once
#include "../../include/qeh.h"
#include "device_common.h"

namespace qeh {

constexpr int kRadixBits = 8;
constexpr int kRadix = 1 << kRadixBits;

// One pass's tile (k_rs_scatter, k_part_scatter*): 1024 threads, kRsIpt rows each.
constexpr int kRsIpt = 8;
constexpr int kRsThreads = 1024;
constexpr int kRsSTile = kRsThreads * kRsIpt;  // 8192

// the most partitions the small move kernels (k_part_scatter_small, k_part_gather_small) take
constexpr int kPsDig = 16;

__device__ __forceinline__ int64_t ordered_key(const ColRef &c, int64_t row) {
    const int64_t x = load_i64(c, row);
    if (c.dtype == QEH_DT_FLOAT32 || c.dtype == QEH_DT_FLOAT64) return f64_order_key(as_f64(x));
    return x;
}

// lanes of this wave whose digit equals mine (wave64 has no match_any: 8 ballots)
__device__ __forceinline__ uint64_t digit_peers(uint32_t dg, bool live) {
    uint64_t peers = __ballot(live);
#pragma unroll
    for (int b = 0; b < kRadixBits; ++b) {
        const uint64_t m = __ballot((dg >> b) & 1);
        peers &= ((dg >> b) & 1) ? m : ~m;
    }
    return peers;
}

// Stable rank of this lane's row among the rows of digit dg ranked so far by this wave (wc = the
// wave's counters): one returning LDS atomic when the device serves a wave's lanes in lane order
// (AT, the default after the lds_atomic_rank_ok self-check), else ballot peers; dead lanes get 0.
template <bool AT>
__device__ __forceinline__ uint32_t tile_rank(uint32_t *wc, uint32_t dg, bool live) {
    if constexpr (AT) {
        return live ? atomicAdd(&wc[dg], 1u) : 0u;
    } else {
        const uint32_t d = live ? dg : 0u;
        const uint64_t peers = digit_peers(d, live);
        const uint32_t before = wc[d];
        if (live && mbcnt(peers) == 0) wc[d] = before + (uint32_t)popc64(peers);
        return live ? before + mbcnt(peers) : 0u;
    }
}

// a barrier that waits for LDS only: global loads issued before it stay in flight
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

}  // namespace qeh
