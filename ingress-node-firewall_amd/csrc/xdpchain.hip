// xdpchain.hip — a multi-buffer AF_XDP ring (XDP_USE_SG) -> one frame per descriptor chain (infw_classify_xdp_mb).
//
// The ring is compacted to an infw_frame_batch in scratch, the registered frames kernel classifies it once per frame
// (infw_launch_classify, INFW_INPUT_FRAMES: selector, shapes and sidebands unchanged), and the answers are scattered
// back to every descriptor of each chain.  Whether a descriptor heads a frame depends on its predecessor, a frame's
// length is a sum over a run of descriptors that may cross waves, workgroups and tiles, and every descriptor needs its
// frame's index: a segmented scan over the ring, done as three forward-only kernels so that no workgroup ever waits on
// another (no look-back flags, no tickets):
//
//   xdp_chain_reduce   one workgroup per tile of kTile descriptors, one descriptor per lane -> the tile's summary
//                      {heads in the tile, sum of len from its last head to its end (the whole tile if it has none)}
//   xdp_chain_carry    one workgroup: exclusive scan of the summaries with (h1,l1) o (h2,l2) = (h1+h2, h2 ? l2 : l1+l2),
//                      in place, kCarry summaries per round -> per tile {frames before it, length a chain open
//                      at its start already has}, and the ring's frame count
//   xdp_chain_emit     per tile again, with its carry: frame_of[i]; a head writes its frame's umem offset and linear
//                      length, the chain's closing descriptor the frame length; slots past the frame count are zeroed
//                      (linear length 0: the frames kernel reads nothing for them and counts nothing)
//   xdp_chain_scatter  result_words[i] = frame results[frame_of[i]], verdicts alike
//
// Within a wave the head mask is one ballot; a lane's distance to its chain's head follows from the mask by clz, and
// the segmented sum is a DPP scan (row_shr 1/2/4/8, row_bcast 15/31) whose every step is guarded by that distance.
// The waves of a tile are combined through LDS.  The classify never uses a continuation's addr.
//
// Deny events (infw_classify_xdp_mb_ex): the frames kernel's event instantiation appends its records with the scratch
// frame index; xdp_chain_emit also writes head_of[frame] and snapshots *events_count, and xdp_event_remap rewrites
// pkt_index to the head's ring index for the records this call appended, and for no other.
//
//   xdp_event_samples_kernel   infw_events_capture_xdp: the perf sample of each record, its first `captured` bytes
//                      gathered across the chain's buffers — the one place a continuation's addr is dereferenced
//
// Many rings in one call (infw_classify_xdp_rings): the same passes over 64-descriptor chunks of all the rings, with a
// ring table and a chunk -> ring map in scratch — the xdp_rings_* kernels below.  Their deny events
// (infw_classify_xdp_rings_ex) carry the flat index of the frame's head; xdp_rings_event_samples finds each record's
// ring in the table's flat-index column (staged in LDS, two wave-wide compares) and walks the chain inside that ring.
// The output side of a poll (infw_classify_xdp_rings_split): each ring partitioned by verdict into its forward and fill
// lists after the frames kernel — the xdp_rings_split_* kernels, a second run of xdp_chain_carry between them.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "../../include/infw.h"
#include "infw_launch.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = INFW_XDP_CHAIN_TILE;    // descriptors per workgroup = threads: one descriptor per lane
constexpr int kWaves = kTile / 64;
constexpr int kCarry = INFW_XDP_CHAIN_CARRY;  // summaries per round of the carry kernel = its threads
static_assert(kTile % 64 == 0 && kCarry % 64 == 0 && kTile <= 1024 && kCarry <= 1024, "whole waves, one workgroup");

template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint32_t dpp0(uint32_t v) {  // lanes without a source (or masked off) read 0
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, kRowMask, 0xF, false);
}
constexpr int kRowShr = 0x110, kWaveShr1 = 0x138, kRowBcast15 = 0x142, kRowBcast31 = 0x143;

struct LaneScan {
    uint32_t len;     // the descriptor's len (0 past the ring)
    uint32_t opt;     // its options
    uint64_t addr;
    bool head;        // first descriptor of a frame
    uint32_t heads;   // heads of the wave at or below this lane
    uint32_t wheads;  // heads of the whole wave
    uint32_t sum;     // len summed from the lane's head — or from the wave's lane 0 when heads == 0 — to the lane
};

// One descriptor per lane, every lane of the wave active.  Descriptor i heads a frame iff i == 0 or descriptor i - 1
// has PKT_CONTD clear: the predecessor's options come from the lane below (DPP wave_shr), the wave's lane 0 reads them.
__device__ __forceinline__ LaneScan scan_wave(const infw_xdp_desc *__restrict__ descs, uint64_t i, uint64_t n) {
    const uint32_t lane = threadIdx.x & 63u;
    LaneScan s{};
    if (i < n) {
        const u32x4 d = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(descs) + i);
        s.addr = (uint64_t)d[1] << 32 | d[0];
        s.len = d[2];
        s.opt = d[3];
    }
    uint32_t prev = dpp0<kWaveShr1, 0xF>(s.opt);
    if (lane == 0 && i > 0 && i < n) prev = __builtin_nontemporal_load(&descs[i - 1].options);
    s.head = i < n && (i == 0 || !(prev & INFW_XDP_PKT_CONTD));
    const uint64_t m = __ballot(s.head);
    const uint64_t below = m & (~0ull >> (63u - lane));
    s.heads = (uint32_t)__popcll(below);
    s.wheads = (uint32_t)__popcll(m);
    // lanes below this one that belong to the same run (all of them when the wave has no head at or below it)
    const uint32_t dist = below ? lane - (63u - (uint32_t)__clzll(below)) : lane;
    uint32_t x = s.len, t;
    // within a row of 16: after the step of d, x covers [max(head, row start, lane - 2d + 1), lane]
    t = dpp0<kRowShr + 1, 0xF>(x);
    if (dist >= 1) x += t;
    t = dpp0<kRowShr + 2, 0xF>(x);
    if (dist >= 2) x += t;
    t = dpp0<kRowShr + 4, 0xF>(x);
    if (dist >= 4) x += t;
    t = dpp0<kRowShr + 8, 0xF>(x);
    if (dist >= 8) x += t;
    // rows 1 and 3 take the row below's last lane when the run started before their row, then lanes 32..63 take
    // lane 31 (by then complete from lane 0) when it started before lane 32
    t = dpp0<kRowBcast15, 0xA>(x);
    if ((lane & 16u) && dist > (lane & 15u)) x += t;
    t = dpp0<kRowBcast31, 0xC>(x);
    if ((lane & 32u) && dist > (lane & 31u)) x += t;
    s.sum = x;
    return s;
}

// (h1, l1) o (h2, l2) = (h1 + h2, h2 ? l2 : l1 + l2): runs of descriptors appended left to right
__device__ __forceinline__ uint2 chain_op(uint2 a, uint2 b) { return make_uint2(a.x + b.x, b.x ? b.y : a.y + b.y); }

__global__ __launch_bounds__(kTile) void xdp_chain_reduce(const infw_xdp_desc *__restrict__ descs, uint64_t n,
                                                           uint2 *__restrict__ tiles) {
    __shared__ uint2 s_w[kWaves];
    const LaneScan s = scan_wave(descs, (uint64_t)blockIdx.x * kTile + threadIdx.x, n);
    if ((threadIdx.x & 63u) == 63u) s_w[threadIdx.x >> 6] = make_uint2(s.wheads, s.sum);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint2 t = s_w[0];
        for (int w = 1; w < kWaves; w++) t = chain_op(t, s_w[w]);
        tiles[blockIdx.x] = t;
    }
}

// Exclusive scan of the tile summaries, in place (a thread reads its own summary before it writes its carry), and the
// ring's frame count.  One workgroup; kCarry summaries per round, the rounds chained by the running total.
__global__ __launch_bounds__(kCarry) void xdp_chain_carry(uint2 *__restrict__ tiles, uint32_t n_tiles,
                                                           uint32_t *__restrict__ n_frames) {
    __shared__ uint2 s_w[kCarry / 64];
    __shared__ uint2 s_total;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint2 run = make_uint2(0u, 0u);
    // the rounds are one serial chain, so a round's summaries are loaded a round ahead: their latency overlaps the
    // scan and the barriers of the round before (nobody has written them yet: a thread writes only its own slot)
    uint2 next = threadIdx.x < n_tiles ? tiles[threadIdx.x] : make_uint2(0u, 0u);
    for (uint32_t base = 0; base < n_tiles; base += kCarry) {  // block-uniform trip count (the barriers below)
        const uint32_t t = base + threadIdx.x;
        uint2 v = next;
        next = t + kCarry < n_tiles ? tiles[t + kCarry] : make_uint2(0u, 0u);
        for (uint32_t d = 1; d < 64; d <<= 1) {  // inclusive scan within the wave
            const uint2 p = make_uint2(__shfl_up(v.x, d), __shfl_up(v.y, d));
            if (lane >= d) v = chain_op(p, v);
        }
        if (lane == 63u) s_w[wv] = v;
        __syncthreads();
        uint2 pre = run;  // everything before this wave
        for (uint32_t w = 0; w < wv; w++) pre = chain_op(pre, s_w[w]);
        const uint2 incl = chain_op(pre, v);
        uint2 excl = make_uint2(__shfl_up(incl.x, 1u), __shfl_up(incl.y, 1u));
        if (lane == 0) excl = pre;
        if (t < n_tiles) tiles[t] = excl;
        if (threadIdx.x == kCarry - 1) s_total = incl;
        __syncthreads();
        run = s_total;
    }
    if (threadIdx.x == 0) *n_frames = run.x;
}

struct ChainFrames {  // the scratch infw_frame_batch and the map back
    uint64_t *offsets;
    uint32_t *linear_len, *pkt_len, *ifindex, *frame_of;
    uint32_t *head_of;           // events only (else null): a frame's head descriptor
    const uint64_t *ev_count;    // events only: the caller's event count, copied to *ev_before ahead of the classify
    uint64_t *ev_before;
};

__global__ __launch_bounds__(kTile) void xdp_chain_emit(const infw_xdp_desc *__restrict__ descs, uint64_t n,
                                                         const uint2 *__restrict__ tiles,
                                                         const uint32_t *__restrict__ n_frames, uint32_t ifindex,
                                                         ChainFrames out) {
    __shared__ uint2 s_w[kWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    const LaneScan s = scan_wave(descs, i, n);
    if ((threadIdx.x & 63u) == 63u) s_w[threadIdx.x >> 6] = make_uint2(s.wheads, s.sum);
    __syncthreads();
    uint2 pre = tiles[blockIdx.x];  // {frames before the tile, length of the chain open at its start}
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) pre = chain_op(pre, s_w[w]);
    if (i >= n) return;
    if (i == 0 && out.ev_before) *out.ev_before = *out.ev_count;
    // descriptor 0 is a head, so pre.x + s.heads >= 1
    const uint32_t frame = pre.x + s.heads - 1u;
    out.frame_of[i] = frame;
    out.ifindex[i] = ifindex;
    if (i >= *n_frames) {  // a slot no frame owns (frame < n_frames <= i: no head or closer writes it)
        out.offsets[i] = 0;
        out.linear_len[i] = 0;
        out.pkt_len[i] = 0;
    }
    if (s.head) {
        out.offsets[frame] = (s.addr & ((1ull << 48) - 1)) + (s.addr >> 48);
        out.linear_len[frame] = s.len;
        if (out.head_of) out.head_of[frame] = (uint32_t)i;
    }
    if (!(s.opt & INFW_XDP_PKT_CONTD) || i == n - 1) out.pkt_len[frame] = s.sum + (s.heads ? 0u : pre.y);
}

__global__ __launch_bounds__(256) void xdp_chain_scatter(const uint32_t *__restrict__ frame_of, uint64_t n,
                                                          const uint32_t *__restrict__ fres,
                                                          const uint8_t *__restrict__ fver,
                                                          uint32_t *__restrict__ results, uint8_t *__restrict__ verdicts) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t f = __builtin_nontemporal_load(&frame_of[i]);
        if (results) __builtin_nontemporal_store(fres[f], &results[i]);
        if (verdicts) __builtin_nontemporal_store(fver[f], &verdicts[i]);
    }
}

// The records the frames kernel appended during this call — slots [*before, min(*count, cap)) — carry the scratch
// frame index: rewrite it to the ring index of the frame's head.  Records that were in the buffer before are not read.
__global__ __launch_bounds__(256) void xdp_event_remap(infw_event_rec *__restrict__ ev, uint64_t cap,
                                                        const uint64_t *__restrict__ before,
                                                        const uint64_t *__restrict__ count,
                                                        const uint32_t *__restrict__ head_of, uint64_t n) {
    const uint64_t c = *count, end = c < cap ? c : cap;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = *before + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < end; k += stride) {
        const uint64_t f = ev[k].pkt_index;
        if (f < n) ev[k].pkt_index = head_of[f];  // always true for a record of this call (f < frames <= n)
    }
}

// ---- infw_events_capture_xdp: perf samples gathered across a chain's buffers ------------------------------------
//
// One wave per event record, kSampleWaves records per workgroup, grid-stride over min(*count, cap).  The wave builds
// the record's 272-B slot in its own LDS image and stores it as 34 8-byte words:
//   walk   64 descriptors per round from the head h = pkt_index: lane l loads descriptor h + 64 r + l (one 16-B load,
//          only below n); the chain ends at the first lane with PKT_CONTD clear or index n - 1 (ballot + ctz).  The
//          lens up to there, each clamped to the 256 bytes a sample can hold (the sums cannot wrap, and nothing behind
//          a clamped descriptor is wanted), go through an unsegmented inclusive DPP scan; with the bytes covered by
//          earlier rounds that is each descriptor's start S in the frame.  A lane is live when [S, S + len) meets
//          [0, captured).  Rounds go on while the chain is open and fewer than `captured` bytes are covered.
//   copy   wave-uniform loop over the live mask: source pointer, S and byte count of fragment j by readlane, then all
//          64 lanes copy it coalesced (lane t takes bytes t, t + 64, ...) to image[12 + S + t]; at most 256 bytes per
//          record however the frame is cut.  Only [buffer_j, buffer_j + min(len_j, captured - S_j)) is read.
//   out    the image is zeroed before the walk (so the pad, and the frame bytes of a record whose chain is not in
//          this ring or is shorter than `captured`, are zeros), size and header go in last; lanes 0..33 read their
//          word back (ds_read_b64) and store it.  The hand-offs through LDS are within one wave: wave-scope fences,
//          no workgroup barrier (the waves of a workgroup run different numbers of records and rounds).
constexpr int kSampleWaves = 4;
constexpr uint32_t kSampleWords = INFW_EVENT_SAMPLE_BYTES / 8;
static_assert(INFW_EVENT_SAMPLE_BYTES % 8 == 0 && kSampleWords <= 64 && INFW_MAX_EVENT_DATA + 12 <= INFW_EVENT_SAMPLE_BYTES,
              "one wave per slot");

__device__ __forceinline__ void wave_lds_handoff() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x) {  // unsegmented: the ladder of scan_wave, unguarded
    x += dpp0<kRowShr + 1, 0xF>(x);
    x += dpp0<kRowShr + 2, 0xF>(x);
    x += dpp0<kRowShr + 4, 0xF>(x);
    x += dpp0<kRowShr + 8, 0xF>(x);
    x += dpp0<kRowBcast15, 0xA>(x);
    x += dpp0<kRowBcast31, 0xC>(x);
    return x;
}

// One record, by one wave: the slot of record `e`, whose chain starts at descriptor h of the ring (umem, descs, n) —
// or, with in_ring false, belongs to no ring of the call — built in the wave's image and stored to `slot`.
__device__ __forceinline__ void sample_record(uint64_t *__restrict__ img8, const infw_event_rec &e,
                                              const uint8_t *__restrict__ umem,
                                              const infw_xdp_desc *__restrict__ descs, uint64_t n, uint64_t h,
                                              bool in_ring, uint8_t *__restrict__ slot) {
    const uint32_t lane = threadIdx.x & 63u;
    uint8_t *const img = reinterpret_cast<uint8_t *>(img8);
    const uint32_t captured = e.captured < INFW_MAX_EVENT_DATA ? e.captured : INFW_MAX_EVENT_DATA;
    if (lane < kSampleWords) img8[lane] = 0;
    wave_lds_handoff();
    uint32_t covered = 0;  // frame bytes the descriptors of earlier rounds hold (clamped: >= captured ends the walk)
    bool open = in_ring;   // a record of another batch: size and header only
    for (uint64_t at = h; open && covered < captured; at += 64) {
        const uint64_t i = at + lane;
        uint64_t addr = 0;
        uint32_t len = 0, opt = 0;
        if (i < n) {
            const u32x4 d = *(reinterpret_cast<const u32x4 *>(descs) + i);
            addr = (uint64_t)d[1] << 32 | d[0];
            len = d[2];
            opt = d[3];
        }
        // lanes at or past n close the chain too, so nothing behind the ring's end is summed (i == n - 1 is first)
        const uint64_t ends = __ballot(i + 1 >= n || !(opt & INFW_XDP_PKT_CONTD));
        const uint32_t last = ends ? (uint32_t)__builtin_ctzll(ends) : 63u;
        open = ends == 0;
        const uint32_t l = lane <= last ? (len < INFW_MAX_EVENT_DATA ? len : INFW_MAX_EVENT_DATA) : 0u;
        const uint32_t incl = wave_scan_incl(l);
        const uint32_t S = covered + incl - l;
        uint64_t live = __ballot(l != 0 && S < captured);
        const uint64_t src = (addr & ((1ull << 48) - 1)) + (addr >> 48);
        while (live) {  // wave-uniform
            const int j = __builtin_ctzll(live);
            live &= live - 1;
            const uint64_t sj = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(src >> 32), j) << 32 |
                                (uint32_t)__builtin_amdgcn_readlane((int)src, j);
            const uint32_t Sj = (uint32_t)__builtin_amdgcn_readlane((int)S, j);
            const uint32_t lj = (uint32_t)__builtin_amdgcn_readlane((int)l, j);
            const uint32_t room = captured - Sj, cnt = lj < room ? lj : room;  // Sj < captured <= 256
            const uint8_t *__restrict__ f = umem + sj;
            for (uint32_t b = lane; b < cnt; b += 64) img[12u + Sj + b] = f[b];
        }
        covered += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (lane == 0) {
        uint32_t hw[2];
        __builtin_memcpy(hw, &e.hdr, 8);
        uint32_t *const img4 = reinterpret_cast<uint32_t *>(img);
        img4[0] = ((8u + e.captured + 4u + 7u) & ~7u) - 4u;  // perf's raw size, as event_samples_kernel writes it
        img4[1] = hw[0];
        img4[2] = hw[1];
    }
    wave_lds_handoff();
    if (lane < kSampleWords) reinterpret_cast<uint64_t *>(slot)[lane] = img8[lane];
    wave_lds_handoff();  // the next record rewrites the image
}

__global__ __launch_bounds__(64 * kSampleWaves) void xdp_event_samples_kernel(
    const uint8_t *__restrict__ umem, const infw_xdp_desc *__restrict__ descs, uint64_t n,
    const infw_event_rec *__restrict__ ev, uint64_t cap, const uint64_t *__restrict__ count,
    uint8_t *__restrict__ out) {
    __shared__ uint64_t s_img[kSampleWaves][kSampleWords];
    const uint64_t c = *count, n_rec = c < cap ? c : cap;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // the record is wave-uniform
    const uint64_t waves = (uint64_t)gridDim.x * kSampleWaves;
    for (uint64_t r = (uint64_t)blockIdx.x * kSampleWaves + wv; r < n_rec; r += waves) {
        const infw_event_rec e = ev[r];
        sample_record(s_img[wv], e, umem, descs, n, e.pkt_index, e.pkt_index < n, out + r * INFW_EVENT_SAMPLE_BYTES);
    }
}

// ---- infw_classify_xdp_rings: every ring of a poll through one chain pass ------------------------------------------
//
// The unit of work is a chunk: 64 consecutive descriptors of one ring, one wave.  Ring r owns ceil(n_r / 64) consecutive
// chunks, a workgroup of kRingWaves waves takes kRingWaves consecutive chunks (of one ring or of several), and its
// summary is the tile summary of the single-ring pass, so xdp_chain_carry runs over it as it is.  Every ring's first
// chunk has a head at lane 0 and chain_op drops the left length at a head: a chain open at a ring's last descriptor
// ends there, and frame indices run on across rings.  Frames, frame_of and the frame results live in flat descriptor
// space (the ring's first flat index + i), which is dense, so the frames kernel runs once over the sum of the n_r.
//
//   xdp_rings_upload   the ring table {umem, descs, results, verdicts, n, ifindex, first chunk, first flat index},
//                      64 entries per launch by value in the kernel arguments: stream-ordered, nothing of the caller's
//                      is read after the call returns, and no host-side wait
//   xdp_rings_map      chunk -> ring, one u32 per chunk (binary search of the first-chunk column, once per call;
//                      the passes below read their ring with one wave-uniform load)
//   xdp_rings_reduce / xdp_rings_emit / xdp_rings_scatter   the three passes of the single-ring form per chunk; the
//                      emit writes umem_r - umem_0 + offset (modulo 2^64) for the frames kernel's umem_0 + offset
constexpr int kRingWaves = 4;  // chunks per workgroup of the reduce / emit / scatter kernels
constexpr int kRingGroup = INFW_XDP_RINGS_GROUP;
static_assert(sizeof(infw_xdp_ring_ent) == 48, "three 16-B words per entry");

struct RingGroup {
    infw_xdp_ring_ent e[kRingGroup];
};

__global__ __launch_bounds__(kRingGroup) void xdp_rings_upload(const RingGroup g, uint32_t cnt,
                                                                infw_xdp_ring_ent *__restrict__ table) {
    if (threadIdx.x < cnt) table[threadIdx.x] = g.e[threadIdx.x];
}

// The rings of the table are non-empty, so the first-chunk column is strictly increasing: the chunk's ring is the last
// one that starts at or before it.
__global__ __launch_bounds__(256) void xdp_rings_map(const infw_xdp_ring_ent *__restrict__ table, uint32_t n_rings,
                                                      uint32_t n_chunks, uint32_t *__restrict__ chunk_ring) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n_chunks) return;
    uint32_t lo = 0, hi = n_rings;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (table[mid].chunk0 <= c) lo = mid;
        else hi = mid;
    }
    chunk_ring[c] = lo;
}

// The wave's chunk: its ring's entry (wave-uniform) and the lane's ring-relative index.  Past the last chunk the ring
// is empty (n == 0: scan_wave loads nothing and reports no head), so every lane of the workgroup stays in the scan.
__device__ __forceinline__ infw_xdp_ring_ent ring_of_chunk(const infw_xdp_ring_ent *__restrict__ table,
                                                           const uint32_t *__restrict__ chunk_ring, uint32_t c,
                                                           uint32_t n_chunks, uint64_t &i) {
    infw_xdp_ring_ent e{};
    i = threadIdx.x & 63u;
    if (c < n_chunks) {
        e = table[__builtin_amdgcn_readfirstlane((int)chunk_ring[c])];
        i += (uint64_t)(c - e.chunk0) * 64u;
    }
    return e;
}

__global__ __launch_bounds__(64 * kRingWaves) void xdp_rings_reduce(const infw_xdp_ring_ent *__restrict__ table,
                                                                     const uint32_t *__restrict__ chunk_ring,
                                                                     uint32_t n_chunks, uint2 *__restrict__ tiles) {
    __shared__ uint2 s_w[kRingWaves];
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t i;
    const infw_xdp_ring_ent e = ring_of_chunk(table, chunk_ring, blockIdx.x * kRingWaves + wv, n_chunks, i);
    const LaneScan s = scan_wave(e.descs, i, e.n);
    if ((threadIdx.x & 63u) == 63u) s_w[wv] = make_uint2(s.wheads, s.sum);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint2 t = s_w[0];
        for (int w = 1; w < kRingWaves; w++) t = chain_op(t, s_w[w]);
        tiles[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(64 * kRingWaves) void xdp_rings_emit(const infw_xdp_ring_ent *__restrict__ table,
                                                                   const uint32_t *__restrict__ chunk_ring,
                                                                   uint32_t n_chunks, const uint2 *__restrict__ tiles,
                                                                   const uint32_t *__restrict__ n_frames,
                                                                   const uint8_t *umem0, ChainFrames out) {
    __shared__ uint2 s_w[kRingWaves];
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t i;
    const infw_xdp_ring_ent e = ring_of_chunk(table, chunk_ring, blockIdx.x * kRingWaves + wv, n_chunks, i);
    const LaneScan s = scan_wave(e.descs, i, e.n);
    if ((threadIdx.x & 63u) == 63u) s_w[wv] = make_uint2(s.wheads, s.sum);
    __syncthreads();
    uint2 pre = tiles[blockIdx.x];  // {frames before the workgroup's chunks, length of the chain open at their start}
    for (uint32_t w = 0; w < wv; w++) pre = chain_op(pre, s_w[w]);
    if (i >= e.n) return;
    // chunk 0 starts a ring and every ring starts with a head, so pre.x + s.heads >= 1; in a ring's first chunk
    // s.heads >= 1 on every lane, so the length carried in from the ring before (pre.y) is never added
    const uint32_t frame = pre.x + s.heads - 1u;
    const uint64_t g = e.flat0 + i;
    if (g == 0 && out.ev_before) *out.ev_before = *out.ev_count;
    out.frame_of[g] = frame;
    if (g >= *n_frames) {  // a slot no frame owns (frame < n_frames <= g: no head or closer writes it)
        out.offsets[g] = 0;
        out.linear_len[g] = 0;
        out.pkt_len[g] = 0;
        out.ifindex[g] = e.ifindex;
    }
    if (s.head) {
        out.offsets[frame] = (uint64_t)(e.umem - umem0) + (s.addr & ((1ull << 48) - 1)) + (s.addr >> 48);
        out.linear_len[frame] = s.len;
        out.ifindex[frame] = e.ifindex;
        if (out.head_of) out.head_of[frame] = (uint32_t)g;
    }
    if (!(s.opt & INFW_XDP_PKT_CONTD) || i == e.n - 1u) out.pkt_len[frame] = s.sum + (s.heads ? 0u : pre.y);
}

__global__ __launch_bounds__(64 * kRingWaves) void xdp_rings_scatter(const infw_xdp_ring_ent *__restrict__ table,
                                                                      const uint32_t *__restrict__ chunk_ring,
                                                                      uint32_t n_chunks,
                                                                      const uint32_t *__restrict__ frame_of,
                                                                      const uint32_t *__restrict__ fres,
                                                                      const uint8_t *__restrict__ fver) {
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t waves = gridDim.x * kRingWaves;
    for (uint32_t c = blockIdx.x * kRingWaves + wv; c < n_chunks; c += waves) {
        uint64_t i;
        const infw_xdp_ring_ent e = ring_of_chunk(table, chunk_ring, c, n_chunks, i);
        if (i >= e.n) continue;
        const uint32_t f = __builtin_nontemporal_load(&frame_of[e.flat0 + i]);
        if (e.results) __builtin_nontemporal_store(fres[f], &e.results[i]);
        if (e.verdicts) __builtin_nontemporal_store(fver[f], &e.verdicts[i]);
    }
}

// ---- infw_classify_xdp_rings_split: every ring partitioned by its frames' verdicts --------------------------------
//
// After the frames kernel: ring r's descriptors whose frame passed go to pass_r in ring order (16 B each, verbatim),
// the umem address of every other one to fill_r, and the pass count to n_pass[r] — a segmented, stable partition over
// the same chunks, with the same forward-only shape as the chain pass (no workgroup waits on another):
//
//   xdp_rings_split_upload  the output table {pass, fill, caller's ring index} beside the ring table, 64 entries per
//                      launch by value; its first launch also zeroes n_pass (an empty ring has no entry and reads 0)
//   xdp_rings_split_count   per chunk the two gathers fver[frame_of[flat0 + i]] once: one ballot of verdict == PASS is
//                      the chunk's pass mask (lanes past n clear), kept in scratch (8 B per chunk); the workgroup's
//                      summary is {ring starts among its chunks, passes since the last of them} — chain_op's monoid,
//                      exact because a ring starts on a chunk boundary
//   xdp_chain_carry    as it is, over those summaries -> per workgroup the passes its open ring already has
//   xdp_rings_split_write   per chunk: base = the carry folded with the earlier waves of the workgroup through LDS (0 in
//                      a ring's first chunk), rank = popcount(mask & lanes below); a pass lane stores its descriptor
//                      to pass[base + rank], any other lane addr & (2^48 - 1) to fill[i - base - rank]; the wave of a
//                      ring's last chunk writes n_pass
struct SplitGroup {
    infw_xdp_split_ent e[kRingGroup];
};
static_assert(sizeof(infw_xdp_split_ent) == 32, "two 16-B words per entry");

__global__ __launch_bounds__(kRingGroup) void xdp_rings_split_upload(const SplitGroup g, uint32_t cnt,
                                                                      infw_xdp_split_ent *__restrict__ table,
                                                                      uint32_t *__restrict__ n_pass, uint32_t n_zero) {
    if (threadIdx.x < cnt) table[threadIdx.x] = g.e[threadIdx.x];
    for (uint32_t r = threadIdx.x; r < n_zero; r += kRingGroup) n_pass[r] = 0;
}

__global__ __launch_bounds__(64 * kRingWaves) void xdp_rings_split_count(const infw_xdp_ring_ent *__restrict__ table,
                                                                          const uint32_t *__restrict__ chunk_ring,
                                                                          uint32_t n_chunks,
                                                                          const uint32_t *__restrict__ frame_of,
                                                                          const uint8_t *__restrict__ fver,
                                                                          uint64_t *__restrict__ masks,
                                                                          uint2 *__restrict__ sums) {
    __shared__ uint2 s_w[kRingWaves];
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t c = blockIdx.x * kRingWaves + wv;
    uint64_t i;
    const infw_xdp_ring_ent e = ring_of_chunk(table, chunk_ring, c, n_chunks, i);  // past the last chunk: n == 0
    bool pass = false;
    if (i < e.n) {
        const uint32_t f = __builtin_nontemporal_load(&frame_of[e.flat0 + i]);
        pass = __builtin_nontemporal_load(&fver[f]) == INFW_XDP_PASS;
    }
    const uint64_t m = __ballot(pass);
    if ((threadIdx.x & 63u) == 0) {
        if (c < n_chunks) masks[c] = m;
        s_w[wv] = make_uint2(c < n_chunks && c == e.chunk0 ? 1u : 0u, (uint32_t)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint2 t = s_w[0];
        for (int w = 1; w < kRingWaves; w++) t = chain_op(t, s_w[w]);
        sums[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(64 * kRingWaves) void xdp_rings_split_write(const infw_xdp_ring_ent *__restrict__ table,
                                                                          const infw_xdp_split_ent *__restrict__ outs,
                                                                          const uint32_t *__restrict__ chunk_ring,
                                                                          uint32_t n_chunks,
                                                                          const uint64_t *__restrict__ masks,
                                                                          const uint2 *__restrict__ sums,
                                                                          uint32_t *__restrict__ n_pass) {
    __shared__ uint2 s_w[kRingWaves];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t c = blockIdx.x * kRingWaves + wv;
    const bool live = c < n_chunks;  // wave-uniform
    infw_xdp_ring_ent e{};
    infw_xdp_split_ent o{};
    uint64_t m = 0;
    if (live) {
        const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk_ring[c]);
        e = table[r];
        o = outs[r];
        m = masks[c];
    }
    const bool start = live && c == e.chunk0;
    if (lane == 0) s_w[wv] = make_uint2(start ? 1u : 0u, (uint32_t)__popcll(m));
    __syncthreads();
    if (!live) return;
    uint2 pre = sums[blockIdx.x];  // {ring starts before the workgroup's chunks, passes of the ring open at their start}
    for (uint32_t w = 0; w < wv; w++) pre = chain_op(pre, s_w[w]);
    const uint32_t base = start ? 0u : pre.y;  // passed descriptors of this ring before this chunk
    const uint32_t first = (c - e.chunk0) * 64u;  // < n: the ring owns exactly ceil(n / 64) chunks
    const uint32_t i = first + lane;
    if (i < e.n) {
        const u32x4 d = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(e.descs) + i);
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (m >> lane & 1ull) {
            if (o.pass) __builtin_nontemporal_store(d, reinterpret_cast<u32x4 *>(o.pass) + (base + rank));
        } else if (o.fill) {
            const uint64_t addr = ((uint64_t)d[1] << 32 | d[0]) & ((1ull << 48) - 1);
            __builtin_nontemporal_store(addr, &o.fill[i - base - rank]);
        }
    }
    if (lane == 0 && e.n - first <= 64u) n_pass[o.ring] = base + (uint32_t)__popcll(m);
}

// ---- infw_classify_xdp_rings_ex / infw_events_capture_xdp_rings: perf samples over the rings of one call ----------
//
// A record's pkt_index is the flat index of its frame's head (the ring's first flat index + i), so the sample kernel
// has one thing to do before the walk of xdp_event_samples_kernel: find the record's ring.  The table's first-flat-index
// column is strictly increasing (its rings are non-empty) and at most INFW_XDP_RINGS_MAX long:
//   stage   every workgroup copies the column into LDS once (4 KiB, entries past the table = 2^32 - 1, above every
//           flat index), one barrier, before the record loop
//   locate  per record, by its wave: lane l compares entry 16 l with pkt_index, the ballot is a run of ones from
//           lane 0 (entry 0 is 0) whose popcount names the block of 16; lanes 0..15 compare the block's entries, the
//           second ballot's popcount names the ring — two LDS reads, no dependent chain of global loads
//   walk    the ring's 48-B entry is loaded wave-uniformly; the chain starts at h = pkt_index - flat0 of the ring's own
//           descs and is bounded by the ring's own n, so it ends at the ring's last descriptor whatever follows it in
//           memory; the fragments are read from the ring's own umem (sample_record)
// Persistent grid-stride grid, one wave per record, no workgroup barrier inside the loop.  `first` (the fused form:
// the count's snapshot xdp_rings_emit took) names the first record to sample; null is 0.
constexpr uint32_t kRingsMax = INFW_XDP_RINGS_MAX;
static_assert(kRingsMax == 64 * 16, "two levels of the wave-wide search: 64 blocks of 16 entries");

__global__ __launch_bounds__(64 * kSampleWaves) void xdp_rings_event_samples(
    const infw_xdp_ring_ent *__restrict__ table, uint32_t n_ents, uint64_t total,
    const infw_event_rec *__restrict__ ev, uint64_t cap, const uint64_t *__restrict__ first,
    const uint64_t *__restrict__ count, uint8_t *__restrict__ out) {
    __shared__ uint32_t s_flat0[kRingsMax];
    __shared__ uint64_t s_img[kSampleWaves][kSampleWords];
    for (uint32_t t = threadIdx.x; t < kRingsMax; t += 64 * kSampleWaves) s_flat0[t] = t < n_ents ? table[t].flat0 : ~0u;
    __syncthreads();
    const uint64_t c = *count, n_rec = c < cap ? c : cap;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // the record is wave-uniform
    const uint64_t waves = (uint64_t)gridDim.x * kSampleWaves;
    for (uint64_t r = (first ? *first : 0) + (uint64_t)blockIdx.x * kSampleWaves + wv; r < n_rec; r += waves) {
        const infw_event_rec e = ev[r];
        const bool in_ring = e.pkt_index < total;  // total < 2^31; else a record of another batch: size and header only
        infw_xdp_ring_ent g{};
        if (in_ring) {  // wave-uniform
            const uint32_t p = (uint32_t)e.pkt_index;
            const uint32_t blk = (uint32_t)__popcll(__ballot(s_flat0[16u * lane] <= p)) - 1u;  // lane 0 always votes
            const uint32_t at = (uint32_t)__popcll(__ballot(lane < 16u && s_flat0[16u * blk + (lane & 15u)] <= p)) - 1u;
            g = table[__builtin_amdgcn_readfirstlane((int)(16u * blk + at))];  // < n_ents: the padding is above p
        }
        sample_record(s_img[wv], e, g.umem, g.descs, g.n, e.pkt_index - g.flat0, in_ring,
                      out + r * INFW_EVENT_SAMPLE_BYTES);
    }
}

}  // namespace

extern "C" int infw_launch_classify_xdp_mb(const infw_launch_args *a) {
    const uint64_t n = a->n;
    if (n == 0) return 0;
    const uint32_t n_tiles = (uint32_t)((n + kTile - 1) / kTile);  // n < 2^31 (the caller's check)
    const bool events = a->ev_count != nullptr;
    // one stream-ordered allocation from the context's pool, carved at 16-B boundaries: 29 B per descriptor (frame
    // batch 20, frame_of 4, frame results 4 + 1), 8 B per tile and the frame count; with the event stream 4 B more
    // per descriptor (head_of) and the count's snapshot
    size_t bytes = 0;
    auto carve = [&](size_t sz) {
        const size_t at = bytes;
        bytes += (sz + 15) & ~(size_t)15;
        return at;
    };
    const size_t o_off = carve(n * 8), o_lin = carve(n * 4), o_plen = carve(n * 4), o_ifx = carve(n * 4),
                 o_fof = carve(n * 4), o_res = carve(n * 4), o_ver = carve(n), o_tiles = carve((size_t)n_tiles * 8),
                 o_nf = carve(4), o_hof = carve(events ? n * 4 : 0), o_evb = carve(events ? 8 : 0);
    uint8_t *sc = nullptr;
    if (!a->pool || hipMallocFromPoolAsync(reinterpret_cast<void **>(&sc), bytes, a->pool, a->stream) != hipSuccess) {
        (void)hipGetLastError();
        return -ENOMEM;
    }
    uint32_t *head_of = events ? reinterpret_cast<uint32_t *>(sc + o_hof) : nullptr;
    uint64_t *ev_before = events ? reinterpret_cast<uint64_t *>(sc + o_evb) : nullptr;
    const ChainFrames cf{reinterpret_cast<uint64_t *>(sc + o_off), reinterpret_cast<uint32_t *>(sc + o_lin),
                         reinterpret_cast<uint32_t *>(sc + o_plen), reinterpret_cast<uint32_t *>(sc + o_ifx),
                         reinterpret_cast<uint32_t *>(sc + o_fof), head_of, a->ev_count, ev_before};
    uint32_t *fres = reinterpret_cast<uint32_t *>(sc + o_res);
    uint8_t *fver = sc + o_ver;
    uint2 *tiles = reinterpret_cast<uint2 *>(sc + o_tiles);
    uint32_t *n_frames = reinterpret_cast<uint32_t *>(sc + o_nf);

    hipLaunchKernelGGL(xdp_chain_reduce, dim3(n_tiles), dim3(kTile), 0, a->stream, a->xdp, n, tiles);
    hipLaunchKernelGGL(xdp_chain_carry, dim3(1), dim3(kCarry), 0, a->stream, tiles, n_tiles, n_frames);
    hipLaunchKernelGGL(xdp_chain_emit, dim3(n_tiles), dim3(kTile), 0, a->stream, a->xdp, n, (const uint2 *)tiles,
                       (const uint32_t *)n_frames, a->xdp_ifindex, cf);
    int rc = hipGetLastError() == hipSuccess ? 0 : -EIO;
    if (rc == 0) {
        // a->ev / ev_cap / ev_count go with the copy: the frames kernel's event instantiation appends the records
        const infw_frame_batch fb{a->umem, cf.offsets, 0, cf.linear_len, cf.pkt_len, cf.ifindex};
        infw_launch_args f = *a;
        f.input = INFW_INPUT_FRAMES;
        f.frames = &fb;
        f.umem = nullptr;
        f.xdp = nullptr;
        f.results = a->results ? fres : nullptr;
        f.verdicts = a->verdicts ? fver : nullptr;
        rc = infw_launch_classify(&f);
    }
    if (rc == 0 && events && a->ev_cap) {  // at most one new record per frame, and none past the capacity
        const uint64_t most = n < a->ev_cap ? n : a->ev_cap, blocks = (most + 255) / 256, cap = (uint64_t)a->cus * 8;
        hipLaunchKernelGGL(xdp_event_remap, dim3((uint32_t)(blocks < cap ? blocks : cap)), dim3(256), 0, a->stream,
                           a->ev, a->ev_cap, (const uint64_t *)ev_before, (const uint64_t *)a->ev_count,
                           (const uint32_t *)head_of, n);
        if (hipGetLastError() != hipSuccess) rc = -EIO;
    }
    if (rc == 0 && (a->results || a->verdicts)) {
        const uint64_t blocks = (n + 255) / 256, cap = (uint64_t)a->cus * 8;
        hipLaunchKernelGGL(xdp_chain_scatter, dim3((uint32_t)(blocks < cap ? blocks : cap)), dim3(256), 0, a->stream,
                           (const uint32_t *)cf.frame_of, n, (const uint32_t *)fres, (const uint8_t *)fver, a->results,
                           a->verdicts);
        if (hipGetLastError() != hipSuccess) rc = -EIO;
    }
    (void)hipFreeAsync(sc, a->stream);
    return rc;
}

// The ring table into scratch, stream-ordered: INFW_XDP_RINGS_GROUP entries per launch, by value.
static void upload_ring_table(const infw_xdp_ring_ent *ents, uint32_t n_ents, infw_xdp_ring_ent *table,
                              hipStream_t stream) {
    RingGroup grp{};
    for (uint32_t base = 0; base < n_ents; base += kRingGroup) {
        const uint32_t cnt = n_ents - base < (uint32_t)kRingGroup ? n_ents - base : (uint32_t)kRingGroup;
        for (uint32_t k = 0; k < cnt; k++) grp.e[k] = ents[base + k];
        hipLaunchKernelGGL(xdp_rings_upload, dim3(1), dim3(kRingGroup), 0, stream, grp, cnt, table + base);
    }
}

// One wave per record, kSampleWaves per workgroup, at most `most` records to sample, the grid capped per CU.
static void launch_rings_samples(const infw_xdp_ring_ent *table, uint32_t n_ents, uint64_t total,
                                 const infw_event_rec *ev, uint64_t cap, const uint64_t *first, const uint64_t *count,
                                 infw_event_sample *samples, uint64_t most, uint32_t cus, hipStream_t stream) {
    const uint64_t blocks = (most + kSampleWaves - 1) / kSampleWaves, lim = 8ull * cus;
    hipLaunchKernelGGL(xdp_rings_event_samples, dim3((uint32_t)(blocks < lim ? blocks : lim)), dim3(64 * kSampleWaves),
                       0, stream, table, n_ents, total, ev, cap, first, count, reinterpret_cast<uint8_t *>(samples));
}

// ents: the call's non-empty rings with their first chunk and first flat index filled in (abi.cpp), read before the
// call returns; a->n is the sum of their n (< 2^31), n_chunks the sum of their chunks.
extern "C" int infw_launch_classify_xdp_rings(const infw_launch_args *a, const infw_xdp_ring_ent *ents, uint32_t n_ents,
                                              uint32_t n_chunks, infw_event_sample *samples,
                                              const infw_xdp_split_args *split) {
    const uint64_t n = a->n;
    if (n == 0 || n_ents == 0) {
        if (!split || split->n_rings == 0) return 0;
        hipLaunchKernelGGL(xdp_rings_split_upload, dim3(1), dim3(kRingGroup), 0, a->stream, SplitGroup{}, 0u,
                           (infw_xdp_split_ent *)nullptr, split->n_pass, split->n_rings);  // only empty rings: the zeros
        return hipGetLastError() == hipSuccess ? 0 : -EIO;
    }
    const uint32_t n_tiles = (n_chunks + kRingWaves - 1) / kRingWaves;
    const bool events = a->ev_count != nullptr;
    bool any_res = false, any_ver = false;
    for (uint32_t r = 0; r < n_ents; r++) any_res |= ents[r].results != nullptr, any_ver |= ents[r].verdicts != nullptr;
    // one stream-ordered allocation, carved at 16-B boundaries: 29 B per descriptor as for one ring, 4 B per chunk
    // (its ring), 8 B per workgroup of kRingWaves chunks (its summary), 48 B per ring (the table) and the frame count;
    // with the event stream 4 B more per descriptor (head_of) and the count's snapshot.  With the split, behind all of
    // those (without it the carve is the plain call's): 8 B per chunk (its pass mask), 32 B per ring (the output table)
    // and the second carry's total.  The split's per-workgroup summaries reuse `tiles`: xdp_rings_emit, the chain
    // pass's last reader of it, has run before the frames kernel, and the split passes run after.
    size_t bytes = 0;
    auto carve = [&](size_t sz) {
        const size_t at = bytes;
        bytes += (sz + 15) & ~(size_t)15;
        return at;
    };
    const size_t o_off = carve(n * 8), o_lin = carve(n * 4), o_plen = carve(n * 4), o_ifx = carve(n * 4),
                 o_fof = carve(n * 4), o_res = carve(n * 4), o_ver = carve(n), o_tiles = carve((size_t)n_tiles * 8),
                 o_nf = carve(4), o_map = carve((size_t)n_chunks * 4),
                 o_tab = carve((size_t)n_ents * sizeof(infw_xdp_ring_ent)), o_hof = carve(events ? n * 4 : 0),
                 o_evb = carve(events ? 8 : 0), o_mask = carve(split ? (size_t)n_chunks * 8 : 0),
                 o_out = carve(split ? (size_t)n_ents * sizeof(infw_xdp_split_ent) : 0), o_nst = carve(split ? 4 : 0);
    uint8_t *sc = nullptr;
    if (!a->pool || hipMallocFromPoolAsync(reinterpret_cast<void **>(&sc), bytes, a->pool, a->stream) != hipSuccess) {
        (void)hipGetLastError();
        return -ENOMEM;
    }
    uint32_t *head_of = events ? reinterpret_cast<uint32_t *>(sc + o_hof) : nullptr;
    uint64_t *ev_before = events ? reinterpret_cast<uint64_t *>(sc + o_evb) : nullptr;
    const ChainFrames cf{reinterpret_cast<uint64_t *>(sc + o_off), reinterpret_cast<uint32_t *>(sc + o_lin),
                         reinterpret_cast<uint32_t *>(sc + o_plen), reinterpret_cast<uint32_t *>(sc + o_ifx),
                         reinterpret_cast<uint32_t *>(sc + o_fof), head_of, a->ev_count, ev_before};
    uint32_t *fres = reinterpret_cast<uint32_t *>(sc + o_res);
    uint8_t *fver = sc + o_ver;
    uint2 *tiles = reinterpret_cast<uint2 *>(sc + o_tiles);
    uint32_t *n_frames = reinterpret_cast<uint32_t *>(sc + o_nf);
    uint32_t *chunk_ring = reinterpret_cast<uint32_t *>(sc + o_map);
    infw_xdp_ring_ent *table = reinterpret_cast<infw_xdp_ring_ent *>(sc + o_tab);
    const uint8_t *umem0 = ents[0].umem;

    upload_ring_table(ents, n_ents, table, a->stream);
    infw_xdp_split_ent *outs = reinterpret_cast<infw_xdp_split_ent *>(sc + o_out);
    if (split) {
        SplitGroup grp{};
        for (uint32_t base = 0; base < n_ents; base += kRingGroup) {
            const uint32_t cnt = n_ents - base < (uint32_t)kRingGroup ? n_ents - base : (uint32_t)kRingGroup;
            for (uint32_t k = 0; k < cnt; k++) grp.e[k] = split->ents[base + k];
            hipLaunchKernelGGL(xdp_rings_split_upload, dim3(1), dim3(kRingGroup), 0, a->stream, grp, cnt, outs + base,
                               split->n_pass, base ? 0u : split->n_rings);
        }
    }
    hipLaunchKernelGGL(xdp_rings_map, dim3((n_chunks + 255) / 256), dim3(256), 0, a->stream,
                       (const infw_xdp_ring_ent *)table, n_ents, n_chunks, chunk_ring);
    hipLaunchKernelGGL(xdp_rings_reduce, dim3(n_tiles), dim3(64 * kRingWaves), 0, a->stream,
                       (const infw_xdp_ring_ent *)table, (const uint32_t *)chunk_ring, n_chunks, tiles);
    hipLaunchKernelGGL(xdp_chain_carry, dim3(1), dim3(kCarry), 0, a->stream, tiles, n_tiles, n_frames);
    hipLaunchKernelGGL(xdp_rings_emit, dim3(n_tiles), dim3(64 * kRingWaves), 0, a->stream,
                       (const infw_xdp_ring_ent *)table, (const uint32_t *)chunk_ring, n_chunks, (const uint2 *)tiles,
                       (const uint32_t *)n_frames, umem0, cf);
    int rc = hipGetLastError() == hipSuccess ? 0 : -EIO;
    if (rc == 0) {
        // a->ev / ev_cap / ev_count go with the copy: the frames kernel's event instantiation appends the records,
        // ifId from the frame's own ifindex
        const infw_frame_batch fb{umem0, cf.offsets, 0, cf.linear_len, cf.pkt_len, cf.ifindex};
        infw_launch_args f = *a;
        f.input = INFW_INPUT_FRAMES;
        f.frames = &fb;
        f.umem = nullptr;
        f.xdp = nullptr;
        f.results = any_res ? fres : nullptr;
        f.verdicts = any_ver || split ? fver : nullptr;  // the split reads the frame verdicts whoever else does
        rc = infw_launch_classify(&f);
    }
    if (rc == 0 && events && a->ev_cap) {  // at most one new record per frame, and none past the capacity
        const uint64_t most = n < a->ev_cap ? n : a->ev_cap, blocks = (most + 255) / 256, cap = (uint64_t)a->cus * 8;
        hipLaunchKernelGGL(xdp_event_remap, dim3((uint32_t)(blocks < cap ? blocks : cap)), dim3(256), 0, a->stream,
                           a->ev, a->ev_cap, (const uint64_t *)ev_before, (const uint64_t *)a->ev_count,
                           (const uint32_t *)head_of, n);
        // the fused capture: the records this call appended, from the table already in scratch
        if (samples)
            launch_rings_samples(table, n_ents, n, a->ev, a->ev_cap, ev_before, a->ev_count, samples, most, a->cus,
                                 a->stream);
        if (hipGetLastError() != hipSuccess) rc = -EIO;
    }
    if (rc == 0 && (any_res || any_ver)) {
        const uint32_t cap = a->cus * 8;
        hipLaunchKernelGGL(xdp_rings_scatter, dim3(n_tiles < cap ? n_tiles : cap), dim3(64 * kRingWaves), 0, a->stream,
                           (const infw_xdp_ring_ent *)table, (const uint32_t *)chunk_ring, n_chunks,
                           (const uint32_t *)cf.frame_of, (const uint32_t *)fres, (const uint8_t *)fver);
        if (hipGetLastError() != hipSuccess) rc = -EIO;
    }
    if (rc == 0 && split) {
        uint64_t *masks = reinterpret_cast<uint64_t *>(sc + o_mask);
        hipLaunchKernelGGL(xdp_rings_split_count, dim3(n_tiles), dim3(64 * kRingWaves), 0, a->stream,
                           (const infw_xdp_ring_ent *)table, (const uint32_t *)chunk_ring, n_chunks,
                           (const uint32_t *)cf.frame_of, (const uint8_t *)fver, masks, tiles);
        hipLaunchKernelGGL(xdp_chain_carry, dim3(1), dim3(kCarry), 0, a->stream, tiles, n_tiles,
                           reinterpret_cast<uint32_t *>(sc + o_nst));
        hipLaunchKernelGGL(xdp_rings_split_write, dim3(n_tiles), dim3(64 * kRingWaves), 0, a->stream,
                           (const infw_xdp_ring_ent *)table, (const infw_xdp_split_ent *)outs,
                           (const uint32_t *)chunk_ring, n_chunks, (const uint64_t *)masks, (const uint2 *)tiles,
                           split->n_pass);
        if (hipGetLastError() != hipSuccess) rc = -EIO;
    }
    (void)hipFreeAsync(sc, a->stream);
    return rc;
}

// The stand-alone capture: the table alone goes to scratch (48 B per non-empty ring), then the sample kernel over
// every record below min(*count, cap).  With no non-empty ring every record is one of another batch.
extern "C" int infw_launch_event_samples_xdp_rings(const infw_xdp_ring_ent *ents, uint32_t n_ents, uint64_t total,
                                                   const infw_event_rec *ev, uint64_t cap, const uint64_t *count,
                                                   infw_event_sample *samples, uint32_t cus, hipMemPool_t pool,
                                                   hipStream_t stream) {
    if (cap == 0) return 0;
    infw_xdp_ring_ent *table = nullptr;
    if (n_ents) {
        if (!pool || hipMallocFromPoolAsync(reinterpret_cast<void **>(&table), (size_t)n_ents * sizeof(*table), pool,
                                            stream) != hipSuccess) {
            (void)hipGetLastError();
            return -ENOMEM;
        }
        upload_ring_table(ents, n_ents, table, stream);
    }
    launch_rings_samples(table, n_ents, total, ev, cap, nullptr, count, samples, cap, cus, stream);
    const int rc = hipGetLastError() == hipSuccess ? 0 : -EIO;
    if (table) (void)hipFreeAsync(table, stream);
    return rc;
}

// One wave per record: kSampleWaves records per workgroup, the grid capped by the CU count (grid-stride beyond it).
extern "C" int infw_launch_event_samples_xdp(const uint8_t *umem, const infw_xdp_desc *descs, uint64_t n,
                                             const infw_event_rec *ev, uint64_t cap, const uint64_t *count,
                                             infw_event_sample *samples, uint32_t cus, hipStream_t stream) {
    if (cap == 0) return 0;
    const uint64_t blocks = (cap + kSampleWaves - 1) / kSampleWaves, lim = 8ull * cus;
    hipLaunchKernelGGL(xdp_event_samples_kernel, dim3((uint32_t)(blocks < lim ? blocks : lim)), dim3(64 * kSampleWaves),
                       0, stream, umem, descs, n, ev, cap, count, reinterpret_cast<uint8_t *>(samples));
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
