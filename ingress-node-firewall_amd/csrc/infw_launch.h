// infw_launch.h — the launch interface between the C ABI (abi.cpp) and the kernels (classify.hip).
//
// One call describes one classify launch: the epoch's table view, the batch in one of its three forms, the outputs,
// the launch shape (infw_set_launch) and the sidebands.  The kernel instantiation it runs is chosen by one
// deterministic selector from the epoch's kind (lean, per-list part counts, /16 words, half-first reads, two-phase)
// and the shape; every instantiation the selector can return is listed in one registry (classify.hip), which the
// tests enumerate (infw_kernel_variant_name) and run one by one against the oracle.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/infw.h"
#include "infw_tables.h"

struct infw_launch_args {
    const infw_dev_tables *T;      // the epoch's view, split / stat_flush_tiles already decided by the caller
    int input;                     // INFW_INPUT_SOA / _COMPACT / _FRAMES / _XDP (include/infw.h)
    const infw_batch_soa *soa;
    const infw_batch_soa_c *compact;
    const infw_frame_batch *frames;
    const uint8_t *umem;             // INFW_INPUT_XDP (infw_classify_xdp): AF_XDP descriptors, frames at
    const infw_xdp_desc *xdp;        // umem + addr, one ifindex for the ring
    uint32_t xdp_ifindex;
    uint64_t n;
    uint32_t *results;
    uint8_t *verdicts;
    uint64_t *stats;
    uint32_t cus;
    int block, group, blocks_per_cu;  // a shape infw_launch_shape_ok accepts
    hipStream_t stream;
    hipMemPool_t pool;             // the context's pool for the two-phase scratch (null: the fused kernel runs)
    uint64_t *split_counts;        // non-null: [0] += 1 per two-phase launch, [1] += 1 per two-phase launch that ran
                                   // the fused kernel for want of scratch (host-side atomics; infw_launch_counts)
    infw_event_rec *ev;
    uint64_t ev_cap;
    uint64_t *ev_count;            // non-null: the deny-event sideband
    uint64_t *dbg_fp;              // non-null: the debug-lookup sideband
    uint32_t *dbg_keys;
    uint32_t *dbg_count;
    uint32_t dbg_slots;
};

// One ring of infw_classify_xdp_rings as the chain pass reads it from its table in scratch: the caller's pointers, and
// where the ring starts in chunk space (64 descriptors per chunk, no chunk shared by two rings) and in flat
// descriptor space.  48 B; up to INFW_XDP_RINGS_GROUP of them travel in one upload kernel's arguments.
struct infw_xdp_ring_ent {
    const uint8_t *umem;
    const infw_xdp_desc *descs;
    uint32_t *results;
    uint8_t *verdicts;
    uint32_t n, ifindex, chunk0, flat0;
};
#define INFW_XDP_RINGS_GROUP 64
// infw_classify_xdp_rings_split: the output side of one ring, parallel to its infw_xdp_ring_ent — the caller's forward
// and fill lists and the caller's ring index (the table holds the non-empty rings only; n_pass is indexed by the
// caller's).  24 B padded to 32: two 16-B words per entry, and 64 of them fit one upload kernel's arguments.
struct infw_xdp_split_ent {
    infw_xdp_desc *pass;
    uint64_t *fill;
    uint32_t ring, pad[3];
};
struct infw_xdp_split_args {
    const infw_xdp_split_ent *ents;  // one per entry of the ring table, same order
    uint32_t *n_pass;                // device, n_rings words: zeroed, then one word per non-empty ring
    uint32_t n_rings;                // the caller's ring count, empty rings included
};

extern "C" {
// Launch (asynchronous).  0, or -EIO on a launch error.
int infw_launch_classify(const infw_launch_args *a);
// The instantiation(s) the launch would run, by registry name ("<phase 1>+decide.512" for the two-phase form),
// without launching anything (host code: no device needed).  0, -ERANGE when cap is too small.
int infw_launch_variant(const infw_launch_args *a, char *name, size_t cap);
int infw_launch_variant_count(void);
const char *infw_launch_variant_name(int i);
// The launch shapes infw_set_launch accepts.
int infw_launch_shape_ok(int block, int group, int blocks_per_cu);
// infw_classify_xdp_mb (xdpchain.hip): a->umem / xdp / xdp_ifindex / n as for INFW_INPUT_XDP; the ring is compacted to
// one frame per descriptor chain in scratch from a->pool, classified by infw_launch_classify as INFW_INPUT_FRAMES
// (a->input is ignored) and the answers scattered to a->results / a->verdicts per descriptor.  Asynchronous.
// 0, -EIO on a launch error, -ENOMEM when there is no pool or the scratch cannot be allocated.
// With a->ev_count the frames kernel's event instantiation appends the deny records, and the records this call
// appended get pkt_index = the ring index of the frame's head descriptor (infw_classify_xdp_mb_ex).
int infw_launch_classify_xdp_mb(const infw_launch_args *a);
// infw_classify_xdp_rings (xdpchain.hip): the same for `n_ents` non-empty rings at once — one allocation, one set of
// launches, one free; no chain runs from one ring into the next.  ents[r].chunk0 / flat0 are the running sums of
// ceil(n / 64) and n; a->n is the sum of n (< 2^31), n_chunks the sum of the chunks; a->results / verdicts / umem /
// xdp are ignored (each ring has its own).  `ents` is read before the call returns.  0, -EIO, -ENOMEM.
// With a->ev_count (infw_classify_xdp_rings_ex) the records this call appended get pkt_index = the flat index of the
// frame's head (ents[r].flat0 + i) and ifId from the ring's own ifindex; with `samples` too, their perf samples are
// written from the table already in scratch (slots [count before, min(count after, a->ev_cap)), no others).
// With `split` (infw_classify_xdp_rings_split; null: the launches and the scratch are the plain call's) n_pass is
// zeroed on the stream first — also when n_ents == 0 — and after the frames kernel each ring is partitioned by its
// frames' verdicts into split->ents[r].pass / .fill, n_pass[split->ents[r].ring] = the ring's passed descriptors.
int infw_launch_classify_xdp_rings(const infw_launch_args *a, const infw_xdp_ring_ent *ents, uint32_t n_ents,
                                   uint32_t n_chunks, infw_event_sample *samples, const infw_xdp_split_args *split);
// infw_events_capture_xdp_rings (xdpchain.hip): samples[k] for k < min(*count, cap) over the same `ents` (total = the
// sum of their n): a record's ring is found from its flat pkt_index, its chain walked inside that ring.  One
// allocation from `pool` (48 B per entry).  Asynchronous.  0, -EIO, -ENOMEM.
int infw_launch_event_samples_xdp_rings(const infw_xdp_ring_ent *ents, uint32_t n_ents, uint64_t total,
                                        const infw_event_rec *ev, uint64_t cap, const uint64_t *count,
                                        infw_event_sample *samples, uint32_t cus, hipMemPool_t pool, hipStream_t stream);
// infw_events_capture_xdp (xdpchain.hip): samples[k] for k < min(*count, cap), each record's first `captured` frame
// bytes gathered across the descriptor chain that starts at its pkt_index.  Asynchronous.  0, -EIO.
int infw_launch_event_samples_xdp(const uint8_t *umem, const infw_xdp_desc *descs, uint64_t n,
                                  const infw_event_rec *ev, uint64_t cap, const uint64_t *count,
                                  infw_event_sample *samples, uint32_t cus, hipStream_t stream);
// infw_events_decode (evdecode.hip): decoded[k] from samples[k] for k < min(*count, cap), one record per lane, the
// parse of infw_evdecode.h over the wave's slots staged in LDS.  Asynchronous.  0, -EIO.
int infw_launch_events_decode(const infw_event_sample *samples, uint64_t cap, const uint64_t *count,
                              infw_event_decoded *decoded, uint32_t cus, hipStream_t stream);
// infw_events_sort (evsort.hip): events[0 .. min(*count, cap)) stably by min(pkt_index, bound) (bound 0: the whole
// key), an LSD radix sort over (key, slot) pairs in scratch from `pool` — 40 B per slot, 48 B when bound is 0 or above
// 2^32 - 1, and 1 KiB per tile of INFW_EVSORT_TILE slots — with ceil(bits(bound) / 8) passes of three launches each.
// cap < 2^32.  Asynchronous.  0, -EIO on a launch error, -ENOMEM when there is no pool or the scratch cannot be had.
int infw_launch_events_sort(infw_event_rec *events, uint64_t cap, const uint64_t *count, uint64_t bound,
                            hipMemPool_t pool, hipStream_t stream);
}
#define INFW_EVSORT_TILE 2048
// The chain pass's tiling: descriptors per workgroup of the reduce / emit kernels, tile summaries per round of the
// carry kernel (infw/_native.py mirrors them for the tests' ring shapes).
#define INFW_XDP_CHAIN_TILE 256
#define INFW_XDP_CHAIN_CARRY 512
