// evsort.hip — infw_events_sort: the deny-event records of a buffer into packet order on the device (gfx950).
//
// The classify kernels append their records with one atomic per wave, so a buffer holds them in no order
// (include/infw.h, Sidebands); the reference's reader sees one queue's records in arrival order (kernel.c:392-399,
// events.go:77-96).  This is the step between classify and capture: a stable LSD radix sort of events[0 .. m),
// m = min(*count, cap) read on the device, by key = min(pkt_index, index_bound).  The 24-B records are not what the
// passes move:
//
//   extract   one pass over the records writes (key, slot) pairs — 8 B {key low, slot}, plus a 4-B column of key high
//             words when the bound does not fit 32 bits — and a straight copy of the records into scratch (the sort ends
//             in `events` itself, so the gather needs a source the scatter does not overwrite).  It also counts the
//             first digit: it is evsort_count with its input read from the records.
//   passes    8 bits per pass over the pairs only, ceil(bits(index_bound) / 8) of them, chosen on the host.  A pass is
//             three forward-only launches, as in xdpchain.hip — no workgroup ever waits on another (no look-back
//             flags, no tickets):
//     evsort_count     one workgroup per tile of kTile pairs -> the tile's 256 digit counts, hist[digit][tile]
//     evsort_scan      workgroup d: exclusive scan of row d over the live tiles, in place, and the row's total
//     evsort_scatter   per tile again: a 256-wide scan of the row totals gives each digit's base, the scanned row the
//                      tile's offset inside it; the tile is ordered by digit in LDS and written out in runs
//   gather    the last pass's scatter writes records, not pairs: events[dst] = copy[slot], each record whole.  So the
//             result lands in `events` whether the pass count is even or odd, and a record is read and written twice
//             in all (the copy, the gather).
//
// Inside a tile of 2048 = 4 waves x 8 rounds x 64 lanes, wave w owns elements [512 w, 512 w + 512) in order.  A lane's
// rank among the lanes of its round with the same digit comes from eight ballots (one per digit bit, and-ed into a
// peer mask) and a popcount of the peers below it; the wave keeps a running count per digit in its own LDS row, read
// by all peers and bumped by the first.  The four rows are then prefixed across waves and the 256 totals scanned, so
// element (wave, round, lane) knows its place in the tile's digit order — equal digits keep their order, which is
// what makes every pass, and so the whole sort, stable.  The tile is staged at those places in LDS (16 KiB of pairs,
// 8 KiB of high words) and lane i writes staged element i to digit base + i: neighbours of a run go to neighbouring
// addresses.  Plain vector loads and stores and LDS only.
//
// Launches are sized by cap; a tile at or past m returns at once, and the scan reads only the rows' live part, so the
// cost follows the records present.  Every global index is bounded before its use: a tile touches [base, base +
// n_tile) with n_tile <= m - base, destinations and gathered slots are checked against m (they are below it by
// construction: the offsets are a permutation of [0, m)), and m <= cap is what the scratch was sized for.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "../../include/infw.h"
#include "infw_launch.h"

namespace {

constexpr uint32_t kTile = INFW_EVSORT_TILE, kBlock = 256, kWaves = kBlock / 64, kRounds = kTile / kBlock;
constexpr uint32_t kScanPer = 4;  // row entries per lane and round of evsort_scan
static_assert(kTile % kBlock == 0 && kBlock == 256, "one thread per digit, whole rounds");
static_assert(sizeof(infw_event_rec) == 24, "three 8-B words per record");

struct Pairs {
    uint2 *kv;     // {key low, slot}
    uint32_t *hi;  // key high (wide keys only)
};

__device__ __forceinline__ void wave_lds_handoff() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool Wide>
__device__ __forceinline__ uint32_t digit_of(uint32_t lo, uint32_t hi, uint32_t shift) {
    return ((Wide && shift >= 32) ? hi >> (shift - 32) : lo >> shift) & 255u;
}

// The lanes of the wave that are valid and hold digit d (meaningful in valid lanes).  Every lane calls it.
__device__ __forceinline__ uint64_t digit_peers(uint32_t d, bool valid) {
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        peers &= bit ? bal : ~bal;
    }
    return peers;
}

// Exclusive scan of one value per thread over the 256 threads; *total = the sum.  s_w: kWaves words, free on return.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *s_w, uint32_t *total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t q = 0; q < kWaves; q++) {
        const uint32_t x = s_w[q];
        base += q < w ? x : 0u;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

__device__ __forceinline__ uint64_t live_records(const uint64_t *count, uint64_t cap) {
    const uint64_t c = *count;
    return c < cap ? c : cap;
}

// The tile's digit counts at `shift`.  Extract: the pairs are made here from the records (key clamped to `bound`,
// 0 = no clamp) and written to p with a copy of the records; otherwise they are read from p.
template <bool Wide, bool Extract>
__global__ __launch_bounds__(kBlock) void evsort_count(const uint64_t *__restrict__ events, uint64_t cap,
                                                       const uint64_t *__restrict__ count, uint64_t bound,
                                                       uint64_t *__restrict__ copy, Pairs p, uint32_t shift,
                                                       uint32_t *__restrict__ hist, uint32_t tiles) {
    __shared__ uint32_t s_hist[256];
    const uint64_t m = live_records(count, cap), base = (uint64_t)blockIdx.x * kTile;
    if (base >= m) return;
    const uint32_t n_tile = m - base < kTile ? (uint32_t)(m - base) : kTile;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    s_hist[tid] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t i = r * kBlock + tid;
        const bool valid = i < n_tile;
        uint32_t lo = 0, hi = 0;
        if (valid) {
            const uint64_t at = base + i;
            if (Extract) {
                const uint64_t w0 = events[3 * at], w1 = events[3 * at + 1], w2 = events[3 * at + 2];
                const uint64_t key = bound && w2 > bound ? bound : w2;
                lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
                p.kv[at] = make_uint2(lo, (uint32_t)at);
                if (Wide) p.hi[at] = hi;
                copy[3 * at] = w0, copy[3 * at + 1] = w1, copy[3 * at + 2] = w2;
            } else {
                lo = p.kv[at].x;
                if (Wide) hi = p.hi[at];
            }
        }
        const uint32_t d = digit_of<Wide>(lo, hi, shift);
        const uint64_t peers = digit_peers(d, valid);
        if (valid && (peers & ((1ull << lane) - 1)) == 0) atomicAdd(&s_hist[d], (uint32_t)__popcll(peers));
    }
    __syncthreads();
    hist[(size_t)tid * tiles + blockIdx.x] = s_hist[tid];
}

// Row blockIdx.x of hist (one digit, a count per tile) -> its exclusive scan over the live tiles, and its total.
__global__ __launch_bounds__(kBlock) void evsort_scan(uint32_t *__restrict__ hist, uint32_t tiles, uint64_t cap,
                                                      const uint64_t *__restrict__ count,
                                                      uint32_t *__restrict__ row_total) {
    __shared__ uint32_t s_w[kWaves];
    const uint64_t m = live_records(count, cap);
    const uint32_t live = (uint32_t)((m + kTile - 1) / kTile);  // <= tiles: m <= cap
    uint32_t *const row = hist + (size_t)blockIdx.x * tiles;
    uint32_t carry = 0;
    for (uint32_t b = 0; b < live; b += kBlock * kScanPer) {
        const uint32_t i0 = b + threadIdx.x * kScanPer;
        uint32_t v[kScanPer], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < kScanPer; j++) {
            v[j] = i0 + j < live ? row[i0 + j] : 0u;
            sum += v[j];
        }
        uint32_t tot;
        uint32_t run = carry + block_excl_scan(sum, s_w, &tot);
#pragma unroll
        for (uint32_t j = 0; j < kScanPer; j++) {
            if (i0 + j < live) row[i0 + j] = run;
            run += v[j];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) row_total[blockIdx.x] = carry;
}

// The tile's pairs, stably by digit, to their places in `out`; Last: the records they stand for, from `copy` to
// `events`, instead.
template <bool Wide, bool Last>
__global__ __launch_bounds__(kBlock) void evsort_scatter(Pairs in, Pairs out, uint64_t cap,
                                                         const uint64_t *__restrict__ count, uint32_t shift,
                                                         const uint32_t *__restrict__ hist, uint32_t tiles,
                                                         const uint32_t *__restrict__ row_total,
                                                         const uint64_t *__restrict__ copy,
                                                         uint64_t *__restrict__ events) {
    __shared__ uint32_t s_rank[kWaves][256];  // per wave and digit: running count, then the digit's place in the tile
    __shared__ uint32_t s_dst[256];           // per digit: global offset of its run minus the run's place in the tile
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint2 s_kv[kTile];
    __shared__ uint32_t s_hi[Wide ? kTile : 1];
    const uint64_t m = live_records(count, cap), base = (uint64_t)blockIdx.x * kTile;
    if (base >= m) return;
    const uint32_t n_tile = m - base < kTile ? (uint32_t)(m - base) : kTile;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
#pragma unroll
    for (uint32_t q = 0; q < kWaves; q++) s_rank[q][tid] = 0;
    __syncthreads();
    uint2 kv[kRounds];
    uint32_t hi[kRounds], rank[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t i = w * (kTile / kWaves) + r * 64 + lane;
        const bool valid = i < n_tile;
        kv[r] = make_uint2(0, 0), hi[r] = 0;
        if (valid) {
            kv[r] = in.kv[base + i];
            if (Wide) hi[r] = in.hi[base + i];
        }
        const uint32_t d = digit_of<Wide>(kv[r].x, hi[r], shift);
        const uint64_t peers = digit_peers(d, valid);
        const uint32_t below = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
        const uint32_t old = valid ? s_rank[w][d] : 0u;
        wave_lds_handoff();
        if (valid && below == 0) s_rank[w][d] = old + (uint32_t)__popcll(peers);
        wave_lds_handoff();
        rank[r] = old + below;
    }
    __syncthreads();
    {   // thread = digit: the waves' counts -> prefixes over the waves; the totals -> places in the tile and in `out`
        uint32_t c[kWaves], tile_count = 0, ignore;
#pragma unroll
        for (uint32_t q = 0; q < kWaves; q++) {
            c[q] = s_rank[q][tid];
            tile_count += c[q];
        }
        const uint32_t place = block_excl_scan(tile_count, s_w, &ignore);
        const uint32_t digit_base = block_excl_scan(row_total[tid], s_w, &ignore);
        uint32_t run = place;
#pragma unroll
        for (uint32_t q = 0; q < kWaves; q++) {
            s_rank[q][tid] = run;
            run += c[q];
        }
        s_dst[tid] = digit_base + hist[(size_t)tid * tiles + blockIdx.x] - place;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t i = w * (kTile / kWaves) + r * 64 + lane;
        if (i < n_tile) {
            const uint32_t at = s_rank[w][digit_of<Wide>(kv[r].x, hi[r], shift)] + rank[r];  // < n_tile
            s_kv[at] = kv[r];
            if (Wide) s_hi[at] = hi[r];
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < n_tile; i += kBlock) {
        const uint2 e = s_kv[i];
        const uint32_t h = Wide ? s_hi[i] : 0u;
        const uint64_t dst = (uint32_t)(s_dst[digit_of<Wide>(e.x, h, shift)] + i);
        if (dst >= m) continue;  // never: the offsets are a permutation of [0, m)
        if (Last) {
            if (e.y >= m) continue;  // never: a slot is an index the extract pass wrote
            const uint64_t *const src = copy + 3 * (uint64_t)e.y;
            const uint64_t w0 = src[0], w1 = src[1], w2 = src[2];
            events[3 * dst] = w0, events[3 * dst + 1] = w1, events[3 * dst + 2] = w2;
        } else {
            out.kv[dst] = e;
            if (Wide) out.hi[dst] = h;
        }
    }
}

template <bool Wide>
void launch_passes(uint64_t *events, uint64_t cap, const uint64_t *count, uint64_t bound, uint32_t passes,
                   uint64_t *copy, Pairs a, Pairs b, uint32_t *hist, uint32_t *row_total, uint32_t tiles,
                   hipStream_t stream) {
    const dim3 grid(tiles), block(kBlock);
    for (uint32_t p = 0; p < passes; p++) {
        const Pairs in = p & 1 ? b : a, out = p & 1 ? a : b;
        const uint32_t shift = 8 * p;
        if (p == 0)
            hipLaunchKernelGGL((evsort_count<Wide, true>), grid, block, 0, stream, (const uint64_t *)events, cap, count,
                               bound, copy, in, shift, hist, tiles);
        else
            hipLaunchKernelGGL((evsort_count<Wide, false>), grid, block, 0, stream, (const uint64_t *)events, cap,
                               count, bound, copy, in, shift, hist, tiles);
        hipLaunchKernelGGL(evsort_scan, dim3(256), block, 0, stream, hist, tiles, cap, count, row_total);
        if (p + 1 == passes)
            hipLaunchKernelGGL((evsort_scatter<Wide, true>), grid, block, 0, stream, in, out, cap, count, shift,
                               (const uint32_t *)hist, tiles, (const uint32_t *)row_total, (const uint64_t *)copy,
                               events);
        else
            hipLaunchKernelGGL((evsort_scatter<Wide, false>), grid, block, 0, stream, in, out, cap, count, shift,
                               (const uint32_t *)hist, tiles, (const uint32_t *)row_total, (const uint64_t *)copy,
                               events);
    }
}

}  // namespace

extern "C" int infw_launch_events_sort(infw_event_rec *events, uint64_t cap, const uint64_t *count, uint64_t bound,
                                       hipMemPool_t pool, hipStream_t stream) {
    if (cap == 0) return 0;
    // keys are min(pkt_index, bound), so `bound` itself is the largest: its bits decide the passes and the pair's width
    const uint32_t bits = bound ? 64u - (uint32_t)__builtin_clzll(bound) : 64u, passes = (bits + 7) / 8;
    const bool wide = bound == 0 || bound > 0xFFFFFFFFull;
    const uint32_t tiles = (uint32_t)((cap + kTile - 1) / kTile);  // cap < 2^32 (the caller's check)
    // one stream-ordered allocation from the context's pool, carved at 16-B boundaries: per slot the record's copy (24)
    // and two pairs (8 + 8; 12 + 12 with wide keys), per tile 256 counts, and the 256 row totals
    size_t bytes = 0;
    auto carve = [&](size_t sz) {
        const size_t at = bytes;
        bytes += (sz + 15) & ~(size_t)15;
        return at;
    };
    const size_t o_copy = carve(cap * 24), o_a = carve(cap * 8), o_b = carve(cap * 8), o_ah = carve(wide ? cap * 4 : 0),
                 o_bh = carve(wide ? cap * 4 : 0), o_hist = carve((size_t)tiles * 256 * 4), o_tot = carve(256 * 4);
    uint8_t *sc = nullptr;
    if (!pool || hipMallocFromPoolAsync(reinterpret_cast<void **>(&sc), bytes, pool, stream) != hipSuccess) {
        (void)hipGetLastError();
        return -ENOMEM;
    }
    const Pairs a{reinterpret_cast<uint2 *>(sc + o_a), reinterpret_cast<uint32_t *>(sc + o_ah)},
        b{reinterpret_cast<uint2 *>(sc + o_b), reinterpret_cast<uint32_t *>(sc + o_bh)};
    (wide ? launch_passes<true> : launch_passes<false>)(
        reinterpret_cast<uint64_t *>(events), cap, count, bound, passes, reinterpret_cast<uint64_t *>(sc + o_copy), a, b,
        reinterpret_cast<uint32_t *>(sc + o_hist), reinterpret_cast<uint32_t *>(sc + o_tot), tiles, stream);
    const int rc = hipGetLastError() == hipSuccess ? 0 : -EIO;
    (void)hipFreeAsync(sc, stream);
    return rc;
}
