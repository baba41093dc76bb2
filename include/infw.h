/*
 * infw.h — C ABI of the MI355X-native batched ingress-firewall classifier.
 *
 * This is the drop-in boundary for the hot path of pbmoses/ingress-node-firewall:
 * the XDP program bpf/ingress_node_firewall_kernel.c and the map-population API
 * of pkg/ebpf (cilium *ebpf.Map calls on ingress_node_firewall_table_map and
 * ingress_node_firewall_statistics_map).  A cgo build of pkg/ebpf binds these
 * symbols; every entry point below names the reference
 * interface it replaces.
 *
 * Conventions (mirroring bpf(2), which is what the reference's Go code sees):
 *   - return 0 on success or a negative errno (-EINVAL, -ENOENT, -EEXIST,
 *     -ENOSPC, -ENOMEM, -ENODEV, -EIO);
 *   - opaque handle, caller-owned buffers, no callbacks;
 *   - threads: control-plane calls (infw_table_*, infw_table_commit,
 *     infw_table_import/export, infw_stats_reset, infw_set_option,
 *     infw_set_launch, infw_debug_lookup_set, infw_debug_keys_clear) are
 *     externally serialised, like ebpfsyncer.go:62,72-73 (e.mu).  The data
 *     path and the readers — infw_classify* (infw_classify_xdp_rings
 *     among them), infw_pack_frames*,
 *     infw_events_sort, infw_events_capture*, infw_events_decode,
 *     infw_stats_read*, infw_table_info,
 *     infw_debug_walk, infw_debug_keys_read, infw_classify_variant — may run
 *     on any number of other threads concurrently with them and with each
 *     other; each batch observes exactly one committed table epoch;
 *   - the library reads no environment variable: everything that selects a
 *     table form or a kernel is a per-context option (infw_set_option), and
 *     no option changes a result word, a verdict or a counter.
 *
 * No torch types, no HIP types: device buffers and streams are plain pointers.
 */
#ifndef INFW_H
#define INFW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Constants — bpf/ingress_node_firewall.h:4-23                              */
/* ------------------------------------------------------------------------ */
#define INFW_MAX_TARGETS 1024          /* ingress_node_firewall.h:13 (stats map size)   */
#define INFW_MAX_RULES_PER_TARGET 100  /* ingress_node_firewall.h:14                    */
#define INFW_MAX_EVENT_DATA 256        /* ingress_node_firewall.h:15                    */
#define INFW_INVALID_RULE_ID 0         /* ingress_node_firewall.h:16                    */
#define INFW_XDP_ABORTED 0             /* UNDEF, ingress_node_firewall.h:10             */
#define INFW_XDP_DROP 1                /* DENY,  ingress_node_firewall.h:11             */
#define INFW_XDP_PASS 2                /* ALLOW, ingress_node_firewall.h:12             */
#define INFW_MAX_PREFIXLEN 160         /* 8 * sizeof(ifindex + ip_data): LPM data bits   */

/* BPF map update flags (uapi/linux/bpf.h), accepted by infw_table_update.   */
#define INFW_BPF_ANY 0
#define INFW_BPF_NOEXIST 1
#define INFW_BPF_EXIST 2

/* Result word: ingress_node_firewall.h:18-23 (SET_ACTIONRULE_RESPONSE).     */
#define INFW_RESULT(action, rule_id) \
    ((uint32_t)((((uint32_t)(rule_id)) & 0xFFFFFFu) << 8 | ((action) & 0xFFu)))
#define INFW_GET_ACTION(r) ((uint8_t)((r) & 0xFFu))
#define INFW_GET_RULE_ID(r) ((uint16_t)(((r) >> 8) & 0xFFFFFFu))

/* ------------------------------------------------------------------------ */
/* Struct ABI — byte-identical to bpf/ingress_node_firewall.h:45-91 and to   */
/* the bpf2go mirrors pkg/ebpf/bpf_bpfel.go:16-51 as marshalled by           */
/* cilium/ebpf sysenc (packed, little-endian).  Skipped if the reference     */
/* header was included first.                                                */
/* ------------------------------------------------------------------------ */
#ifndef __INGRESS_NODE_FIREWALL__
struct ruleStatistics_st {            /* ingress_node_firewall.h:45-54, 32 B */
    struct allow_stats_st {
        uint64_t packets;
        uint64_t bytes;
    } allow_stats;
    struct deny_stats_st {
        uint64_t packets;
        uint64_t bytes;
    } deny_stats;
};

struct event_hdr_st {                 /* ingress_node_firewall.h:58-64, 8 B  */
    uint16_t ifId;
    uint16_t ruleId;
    uint8_t action;
    uint8_t pad;
    uint16_t pktLength;
} __attribute__((packed));

struct ruleType_st {                  /* ingress_node_firewall.h:69-77, 12 B */
    uint32_t ruleId;
    uint8_t protocol;
    uint16_t dstPortStart;
    uint16_t dstPortEnd;
    uint8_t icmpType;
    uint8_t icmpCode;
    uint8_t action;
} __attribute__((packed));

struct lpm_ip_key_st {                /* ingress_node_firewall.h:83-87, 24 B */
    uint32_t prefixLen;
    uint32_t ingress_ifindex;
    uint8_t ip_data[16];
} __attribute__((packed));

struct rulesVal_st {                  /* ingress_node_firewall.h:89-91, 1200 B */
    struct ruleType_st rules[INFW_MAX_RULES_PER_TARGET];
} __attribute__((packed));
#endif /* __INGRESS_NODE_FIREWALL__ */

/* ------------------------------------------------------------------------ */
/* Packet batch: struct-of-arrays header tuples, 32 B per packet.            */
/* One tuple carries exactly the frame bytes kernel.c reads                  */
/* (ingress_node_firewall_main :412-457, ip_extract_l4info :95-174):         */
/*   saddr   16 B  frame[26..29] (IPv4, bytes 4..15 ignored) or frame[22..37] */
/*   ifindex  4 B  xdp_md.ingress_ifindex                                     */
/*   pkt_len  4 B  bpf_xdp_get_buff_len(ctx) (stats byte count)               */
/*   meta     4 B  bits 0..15 ethertype (frame[12]<<8|frame[13]),             */
/*                 bits 16..23 L3 next-proto (frame[23] v4 / frame[20] v6),   */
/*                 bits 24..31 min(linear length, 255) (truncation checks)    */
/*   l4word   4 B  frame[L4..L4+3] little-endian, L4 = 34 (v4) / 54 (v6),     */
/*                 bytes past the linear length read as 0                     */
/* All pointers are device pointers on the device the batch is classified on. */
/* saddr must be 16-byte aligned.                                             */
/* ------------------------------------------------------------------------ */
struct infw_batch_soa {
    const uint8_t *saddr;
    const uint32_t *ifindex;
    const uint32_t *pkt_len;
    const uint32_t *meta;
    const uint32_t *l4word;
};

#define INFW_META(ethertype, proto, caplen)                                    \
    ((uint32_t)((ethertype) & 0xFFFFu) | ((uint32_t)((proto) & 0xFFu) << 16) | \
     ((uint32_t)((caplen) > 255u ? 255u : (caplen)) << 24))

/* Raw frames in device memory (NIC -> HBM ingestion): frame i */
/* starts at frames + (offsets ? offsets[i] : i * stride); only its first     */
/* linear_len[i] bytes are read (xdp data .. data_end).                       */
struct infw_frame_batch {
    const uint8_t *frames;
    const uint64_t *offsets;      /* NULL: fixed-stride chunks (AF_XDP umem style)   */
    uint64_t stride;
    const uint32_t *linear_len;   /* data_end - data                                  */
    const uint32_t *pkt_len;      /* bpf_xdp_get_buff_len(); NULL: = linear_len       */
    const uint32_t *ifindex;
};
/* Writable SoA destination of infw_pack_frames (same layout as infw_batch_soa). */
struct infw_batch_soa_out {
    uint8_t *saddr;
    uint32_t *ifindex;
    uint32_t *pkt_len;
    uint32_t *meta;
    uint32_t *l4word;
};

/* Family-compact layout of the same bytes (infw_classify_c): the 12 address   */
/* bytes only IPv6 packets have are stored only for them.                     */
/*   saddr4   4 B per packet: frame[26..29] (IPv4) or frame[22..25] (IPv6)     */
/*   v6tail   per group g of INFW_V6_GROUP packets, a 12*INFW_V6_GROUP-byte   */
/*            block at g * 12 * INFW_V6_GROUP: frame[26..37] of the group's    */
/*            packets whose meta ethertype is 0x86DD, in packet order, packed */
/*            from the start of the block (4-byte aligned)                     */
/*   ifindex, pkt_len, meta, l4word as in infw_batch_soa                       */
/* A reader touches only the first 12 * (IPv6 packets of the group) bytes of  */
/* a block: 4 + 12 * (IPv6 share) address bytes per packet instead of 16.      */
#define INFW_V6_GROUP 64
struct infw_batch_soa_c {
    const uint32_t *saddr4;
    const uint8_t *v6tail;
    const uint32_t *ifindex;
    const uint32_t *pkt_len;
    const uint32_t *meta;
    const uint32_t *l4word;
};

/* Writable family-compact destination of infw_pack_frames_c.                */
struct infw_batch_soa_c_out {
    uint32_t *saddr4;
    uint8_t *v6tail;
    uint32_t *ifindex;
    uint32_t *pkt_len;
    uint32_t *meta;
    uint32_t *l4word;
};

typedef struct infw_ctx infw_ctx;

/* ------------------------------------------------------------------------ */
/* Lifecycle — replaces NewIngNodeFwController (loader.go:56-112) and Close */
/* (loader.go:306-333) for the table + statistics maps.                      */
/* ------------------------------------------------------------------------ */
/* hip_devices: HIP device ordinals the context replicates its tables onto;   */
/* NULL/n_dev=0 means {current device}.  max_entries: LPM capacity (the       */
/* reference's MAX_TARGETS=1024 at kernel.c:54; 0 selects 1<<22).            */
/* Without INFW_F_HOST_ONLY, -ENODEV when no HIP device is visible: there is   */
/* no CPU classification path.                                                */
#define INFW_F_HOST_ONLY 0x1u   /* control plane only: map API + compile, no    */
                                /* device tables; infw_classify -> -ENODEV     */
#define INFW_F_KEEP_HOST_IMAGE 0x2u /* accepted for compatibility: the host    */
                                    /* image is always kept (incremental       */
                                    /* commits patch it; infw_debug_walk reads) */
#define INFW_F_FULL_COMMIT 0x4u     /* every commit recompiles the whole epoch  */
int infw_create(infw_ctx **out, const int *hip_devices, int n_dev,
                uint32_t max_entries, uint32_t flags);
void infw_destroy(infw_ctx *ctx);
int infw_num_devices(const infw_ctx *ctx);

/* ------------------------------------------------------------------------ */
/* Table map — ingress_node_firewall_table_map (kernel.c:50-57, LPM_TRIE     */
/* key 24 B / value 1200 B).  Calls edit the PENDING set with the kernel's   */
/* LPM-trie map semantics; infw_table_commit publishes it to the GPUs.       */
/* ------------------------------------------------------------------------ */
/* Map.Update(key, val, flags)   loader.go:203  (addOrUpdateRules)           */
/*   -EINVAL prefixLen>160, flags>BPF_EXIST; -EEXIST / -ENOENT per NOEXIST  */
/*           / EXIST.  prefixLen<32 (a partial ifindex, never produced by     */
/*           BuildEBPFKey, loader.go:543) is accepted like lpm_trie does: it  */
/*           covers every ifindex whose key bytes start with its bits, below  */
/*           the interface's own entries (commits with one are full compiles) */
/*   -ENOSPC when a new key would exceed max_entries.                        */
int infw_table_update(infw_ctx *ctx, const struct lpm_ip_key_st *key,
                      const struct rulesVal_st *val, uint64_t flags);
/* Batch form (BPF_MAP_UPDATE_BATCH): val_index==NULL -> keys[i]:vals[i],     */
/* else keys[i]:vals[val_index[i]].  Stops at the first error; *done (may be  */
/* NULL) receives the number of keys applied.                                 */
int infw_table_update_batch(infw_ctx *ctx, const struct lpm_ip_key_st *keys,
                            const struct rulesVal_st *vals, const uint32_t *val_index,
                            uint64_t n, uint64_t flags, uint64_t *done);
/* Map.Delete(key)               loader.go:640  (purgeKeys): exact prefix.    */
int infw_table_delete(infw_ctx *ctx, const struct lpm_ip_key_st *key);
/* Batch form (BPF_MAP_DELETE_BATCH): stops at the first error (-ENOENT for a */
/* key not in the map); *done (may be NULL) receives the keys deleted.         */
int infw_table_delete_batch(infw_ctx *ctx, const struct lpm_ip_key_st *keys, uint64_t n, uint64_t *done);
/* Map.Iterate() key walk        loader.go:293,558 (getStaleKeys,            */
/* GetBPFMapContentForTest): key==NULL or absent -> first key; -ENOENT at end. */
/* Order is the LPM trie's post-order (children before parents, 0-bit first). */
int infw_table_get_next_key(infw_ctx *ctx, const struct lpm_ip_key_st *key,
                            struct lpm_ip_key_st *next);
/* Map.Lookup(key, &val): longest-prefix match over entries with              */
/* prefixLen <= key->prefixLen (BPF LPM trie lookup semantics).               */
int infw_table_lookup(infw_ctx *ctx, const struct lpm_ip_key_st *key,
                      struct rulesVal_st *val);
int infw_table_count(infw_ctx *ctx, uint64_t *n_entries);
/* End of IngressNodeFwRulesLoader (loader.go:189-193): publish the pending   */
/* set as the next epoch; in-flight batches finish on the old one.            */
/* Incremental by default: only the keys edited since the   */
/* last commit are turned into table bytes (DIR-24-8 words / tbl8 groups,     */
/* IPv6 buckets, appended rule lists), copied into the device's spare image,  */
/* which then becomes live — each device keeps two images, so a batch always  */
/* reads exactly one epoch.  Layout changes (new ifindex, overflowed IPv6     */
/* groups, > 1/4 of the keys edited, ...) fall back to a full compile;        */
/* infw_table_info reports which one ran and why.                             */
int infw_table_commit(infw_ctx *ctx);

/* ------------------------------------------------------------------------ */
/* Data path — replaces the per-frame XDP entry ingress_node_firewall_process */
/* (kernel.c:459-462) with one batched launch.                                */
/*   result_words[i] = the `result` of ingress_node_firewall_main (:418-442): */
/*                     (ruleId & 0xFFFFFF) << 8 | action, 0 = UNDEF;          */
/*   xdp_verdicts[i] = XDP return code (1 DROP / 2 PASS);                     */
/*   statistics      = per-rule allow/deny packets+bytes added on the device  */
/*                     (kernel.c:361-390), one slot per device.               */
/* Either output may be NULL.  stream: hipStream_t (NULL = default stream).   */
/* The call is asynchronous with respect to the host.                         */
/* ------------------------------------------------------------------------ */
int infw_classify(infw_ctx *ctx, int dev, const struct infw_batch_soa *in, uint64_t n,
                  uint32_t *result_words, uint8_t *xdp_verdicts, void *stream);
/* infw_classify over the family-compact layout (identical results).          */
int infw_classify_c(infw_ctx *ctx, int dev, const struct infw_batch_soa_c *in, uint64_t n,
                    uint32_t *result_words, uint8_t *xdp_verdicts, void *stream);
/* Standard -> family-compact address layout on the device: saddr4 (n words) */
/* and v6tail (ceil(n / INFW_V6_GROUP) blocks); the other streams are shared.  */
int infw_soa_compact(infw_ctx *ctx, int dev, const struct infw_batch_soa *in, uint64_t n,
                     uint32_t *saddr4, uint8_t *v6tail, void *stream);

/* Launch shape of the classify kernel (default 768 / 0 / 2 = 24 waves per CU). */
/* scan_group 0 = first-match decision tables in one of the shapes           */
/* (block x blocks_per_cu) 768x2, 512x2, 512x3, 512x4, 256x6; scan_group      */
/* 1|4|8 = the one-lane-per-rule ballot scan (kernel.c:222-258 in rule order) */
/* with that many packets in flight, 512x3 or 256x6.  -EINVAL for any other   */
/* shape.  The family-compact layout runs non-default shapes as decision       */
/* tables 512x3; frames and sideband launches have fixed shapes.               */
int infw_set_launch(infw_ctx *ctx, int block, int scan_group, int blocks_per_cu);
/* The launch shape infw_classify uses (default or set above; bench reporting). */
int infw_get_launch(infw_ctx *ctx, int *block, int *scan_group, int *blocks_per_cu);

/* Per-context options.  Each selects among bit-exact forms of the same table */
/* epoch (full compiles read them), how the classify launch reads it, or      */
/* tracing — results, verdicts and counters never depend on them.  value -1   */
/* means "chosen per epoch" where an option has that.  -EINVAL for an unknown */
/* name or a value out of range (nothing changes then).                       */
/*   short_table      -1 auto (DIR-24-8 while ifindexes x 128 MiB <= 4 GiB),   */
/*                    0 DIR-24-8, 1 compressed 16-8-8 (next full compile)      */
/*   d16              -1 auto, 0 off, 1 on: /16 words in front of DIR-24-8      */
/*   dt_half          -1 auto, 0 off, 1 on: half-first decision-line reads      */
/*   dt_parts         0 auto, or 1|2|4|8|16 value parts per (list, class)        */
/*   dt_adapt         1 per-list cut codes (<= 4096 lists), 2 the same without  */
/*                    the skewed cuts, 0 uniform parts                           */
/*   dt_budget_mb     64..1048576 (2048): entry lines of one image at most        */
/*   compile_threads  0 hardware threads (<= 16), or 1..16                        */
/*   split            -1 auto, 0 off, 1 on: two-phase classify (many lists)       */
/*   split_min_mb     0..1048576 (1024): auto splits past this many MiB of lines  */
/*   stat_flush_tiles 1..1024 (1024): LDS counter flush period in tiles           */
/*   trace            bit mask to stderr: 1 compile, 2 incremental patch,          */
/*                    4 commit timing, 8 infw_classify_xdp_host pipeline timing    */
/*   host_threads     0 the CPUs the process may run on (affinity mask, cgroup     */
/*                    CPU quota; <= 16), or 1..64: infw_classify_xdp_host packers  */
int infw_set_option(infw_ctx *ctx, const char *name, int64_t value);
int infw_get_option(infw_ctx *ctx, const char *name, int64_t *value);
/* Name of option i (0-based), NULL past the last.                             */
const char *infw_option_name(int i);

/* Which kernel instantiation(s) a launch would run (introspection; nothing is */
/* launched, no device needed — host-only contexts answer from their image).  */
/* input: INFW_INPUT_* (XDP: infw_classify_xdp); flags: INFW_VARIANT_EVENTS   */
/* for an infw_classify_ex event stream (not with COMPACT or XDP); the debug   */
/* sideband follows infw_debug_lookup_set.  name is a registry name           */
/* (infw_kernel_variant_name); two-phase launches name both kernels joined by */
/* '+'.  -ERANGE when cap is too small.                                        */
#define INFW_INPUT_SOA 0
#define INFW_INPUT_COMPACT 1
#define INFW_INPUT_FRAMES 2
#define INFW_INPUT_XDP 3
#define INFW_VARIANT_EVENTS 0x1u
int infw_classify_variant(infw_ctx *ctx, int dev, int input, uint32_t flags, char *name, size_t cap);
/* Registry of every kernel instantiation the library launches: name of entry */
/* i (0-based), NULL past the last.                                            */
const char *infw_kernel_variant_name(int i);
/* Launch counters of device slot `dev` since infw_create: counts[0] two-phase */
/* launches (phase 1 + decide), counts[1] launches the selector made two-phase */
/* that ran the fused kernel because the scratch could not be allocated (no    */
/* pool, or the pool out of memory) — results are the same either way.        */
int infw_launch_counts(infw_ctx *ctx, int dev, uint64_t counts[2]);

/* Frame headers -> SoA tuples on the device (the packer of the batch format  */
/* above, run as a kernel over frames already in HBM).  Asynchronous.          */
int infw_pack_frames(infw_ctx *ctx, int dev, const struct infw_frame_batch *frames, uint64_t n,
                     const struct infw_batch_soa_out *out, void *stream);
/* infw_pack_frames into the family-compact layout (the production feed of     */
/* infw_classify_c): v6tail blocks of groups with fewer IPv6 packets are only  */
/* written up to their last tail.                                             */
int infw_pack_frames_c(infw_ctx *ctx, int dev, const struct infw_frame_batch *frames, uint64_t n,
                       const struct infw_batch_soa_c_out *out, void *stream);

/* infw_classify straight from the frames (no SoA batch written or read: the  */
/* kernel builds infw_pack_header()'s tuple from each frame's bytes [10, 58)  */
/* in LDS — the XDP program's own input, kernel.c:412-462 per frame).          */
/* Identical results and counters to infw_pack_frames + infw_classify.        */
/* Reads are whole 16-byte aligned blocks that hold a byte of                  */
/* [frame + 10, frame + min(linear_len, 58)): no block outside a frame's own   */
/* bytes' blocks is touched (the packer's rule, infw_pack_frames).             */
int infw_classify_frames(infw_ctx *ctx, int dev, const struct infw_frame_batch *frames, uint64_t n,
                         uint32_t *result_words, uint8_t *xdp_verdicts, void *stream);

/* An AF_XDP socket's RX ring as the feed (the NIC side of   */
/* the frames path): descriptors as the kernel writes them into the ring      */
/* (linux/if_xdp.h struct xdp_desc), frames in the socket's umem.  Frame i's  */
/* bytes start at umem + (addr & (2^48 - 1)) + (addr >> 48) — aligned mode,    */
/* and unaligned mode's offset in bits 48..63 (XSK_UNALIGNED_BUF_OFFSET_SHIFT) */
/* — and len is both its linear length (xdp data .. data_end) and             */
/* bpf_xdp_get_buff_len(): single-buffer frames (a multi-buffer frame's first */
/* descriptor is classified on its own bytes and length).  One ring belongs  */
/* to one interface queue, so every frame carries `ifindex`.  umem and descs  */
/* must be device-accessible: HBM, or pinned host memory (hipHostMalloc), which */
/* the kernel reads in place over PCIe — one 64-B header window and one 16-B  */
/* descriptor per frame.  descs 16-byte aligned.  Identical results and       */
/* counters to infw_classify_frames over the same frames.  Asynchronous.      */
struct infw_xdp_desc {
    uint64_t addr;
    uint32_t len;
    uint32_t options;
};
/* umem and descs are checked with hipPointerGetAttributes: -EFAULT when either */
/* is ordinary (pageable, unregistered) host memory, which the GPU cannot read  */
/* — register such a mapping with infw_host_register first, or use            */
/* infw_classify_xdp_host, which reads it on the CPU.  options is ignored: a    */
/* socket bound with XDP_USE_SG feeds infw_classify_xdp_mb instead.            */
int infw_classify_xdp(infw_ctx *ctx, int dev, const uint8_t *umem, const struct infw_xdp_desc *descs, uint64_t n,
                      uint32_t ifindex, uint32_t *result_words, uint8_t *xdp_verdicts, void *stream);

/* A multi-buffer ring (socket bound with XDP_USE_SG; the reference program is */
/* SEC("xdp.frags"), kernel.c:459): one frame per descriptor chain.            */
/*   - descriptor i is a HEAD iff i == 0 or descriptor i-1 has PKT_CONTD clear; */
/*   - a frame is a head plus the descriptors after it, up to and including    */
/*     the first with PKT_CONTD clear; a chain still open at n-1 ends there    */
/*     with what it has — pass whole frames;                                   */
/*   - the frame is classified on the head's bytes only: linear length = the   */
/*     head's len, frame length (bpf_xdp_get_buff_len(), the counters' bytes,  */
/*     kernel.c:446, :450) = the sum of the chain's len, modulo 2^32;          */
/*   - it is counted once in the per-rule counters;                            */
/*   - a continuation descriptor's addr is never dereferenced (the one call    */
/*     that reads a continuation's bytes is infw_events_capture_xdp, below);   */
/*   - every descriptor of the chain receives the head's result word and       */
/*     verdict (result_words[i] / xdp_verdicts[i] stay per descriptor, so each */
/*     buffer can be released or forwarded);                                   */
/*   - other options bits are ignored.                                         */
/* With every options == 0 it computes what infw_classify_xdp computes.        */
/* Memory checks, alignment and errnos as infw_classify_xdp; -EINVAL for       */
/* n >= 2^31, -ENOMEM when the per-call scratch (29 B per descriptor, 33 B     */
/* with the event stream of infw_classify_xdp_mb_ex; stream-ordered from the   */
/* context's pool) cannot be had.  Asynchronous on `stream`.  Deny events:     */
/* infw_classify_xdp_mb_ex (declared with the sidebands below).  Every ring of  */
/* a poll in one call: infw_classify_xdp_rings, below.  The host-fed calls     */
/* below are single-buffer (they ignore options, as infw_classify_xdp does).   */
#define INFW_XDP_PKT_CONTD (1u << 0)   /* linux/if_xdp.h XDP_PKT_CONTD */
int infw_classify_xdp_mb(infw_ctx *ctx, int dev, const uint8_t *umem, const struct infw_xdp_desc *descs, uint64_t n,
                         uint32_t ifindex, uint32_t *result_words, uint8_t *xdp_verdicts, void *stream);

/* AF_XDP RX rings over a HOST umem, read by the CPU (the host-fed path): the */
/* context's packer threads (option host_threads) read each frame's header    */
/* window where the NIC left it and write the family-compact tuple            */
/* (infw_batch_soa_c, without the ifindex stream: one ring = one interface)    */
/* into pinned slots, which go to the device in bulk copies — ~28 B per packet */
/* over PCIe instead of one 64-B read request per frame.  Pipelined per chunk  */
/* of `chunk` descriptors (0 = 512K; rounded up to 512): packing of chunk k+1  */
/* || H2D of k || classify of k-1 || D2H of k-2, chunks running on from one    */
/* ring into the next.  umem and descs may be any memory the process can read  */
/* (the socket's mmapped RX ring and umem as they are); results / verdicts are */
/* host memory (pinned or infw_host_register'ed for the full rate), per ring   */
/* in descriptor order, either may be NULL.  Frames are read exactly as        */
/* infw_classify_xdp reads them (same result words, verdicts and counters).    */
/* Synchronous; the whole call reads one table epoch.  One call at a time per  */
/* device (concurrent calls queue).                                            */
struct infw_xdp_ring {
    const uint8_t *umem;                 /* frame i at umem + (addr & (2^48-1)) + (addr >> 48) */
    const struct infw_xdp_desc *descs;   /* n RX descriptors                                    */
    uint64_t n;
    uint32_t ifindex;                    /* the interface the socket is bound to                 */
    uint32_t flags;                      /* 0                                                    */
    uint32_t *results;                   /* n result words, or NULL                              */
    uint8_t *verdicts;                   /* n XDP verdicts, or NULL                              */
};
int infw_classify_xdp_host(infw_ctx *ctx, int dev, const struct infw_xdp_ring *rings, uint32_t n_rings,
                           uint64_t chunk);
/* The device-read path over every ring of a poll (one socket per NIC queue,   */
/* several queues per interface, several interfaces) in one call: what         */
/*   infw_classify_xdp_mb(ctx, dev, rings[r].umem, rings[r].descs, rings[r].n, */
/*                        rings[r].ifindex, rings[r].results,                  */
/*                        rings[r].verdicts, stream)                           */
/* computes for r = 0 .. n_rings-1 on one stream against one table epoch —     */
/* result words, verdicts and counters — with one scratch allocation and one   */
/* set of launches for all of them.  One frame per descriptor chain, classified */
/* on the head's bytes with the chain's summed length and counted once; every  */
/* descriptor receives its frame's result word and verdict.                    */
/*   - descriptor 0 of every ring is a head; a chain still open at a ring's    */
/*     last descriptor ends there: no descriptor of another ring is read or    */
/*     summed for it;                                                          */
/*   - a continuation's addr is never dereferenced;                            */
/*   - rings with n == 0 are skipped; a ring's NULL results or verdicts is     */
/*     skipped for that ring only;                                             */
/*   - `rings` is an ordinary host array, read during the call: it may be      */
/*     reused as soon as the call returns.  The pointers in it are as for      */
/*     infw_classify_xdp_mb: umem and descs device-accessible (HBM, pinned or  */
/*     registered host memory), descs 16-byte aligned, results / verdicts      */
/*     device-writable or NULL;                                                */
/*   - asynchronous on `stream`; the call does not wait for work already       */
/*     queued on it.                                                           */
/* -EINVAL: n_rings > INFW_XDP_RINGS_MAX, a ring's flags != 0, 2^31            */
/* descriptors or more in all, a NULL or misaligned pointer in a ring with     */
/* n > 0.  -EFAULT: a ring's umem or descs in memory the GPU cannot read (the  */
/* check of infw_classify_xdp).  -ENOMEM: no per-call scratch from the         */
/* context's pool — 29 B per descriptor, 4 B per chunk (64 descriptors of one  */
/* ring; a ring of n has ceil(n / 64)), 8 B per 4 chunks, 48 B per non-empty   */
/* ring and 4 B, each array rounded up to 16 B.  -ENODEV: host-only context.   */
/* Nothing is launched when an error is returned; n_rings == 0 returns 0.      */
/* Deny events and their perf samples: infw_classify_xdp_rings_ex and           */
/* infw_events_capture_xdp_rings (declared with the sidebands below).          */
#define INFW_XDP_RINGS_MAX 1024
int infw_classify_xdp_rings(infw_ctx *ctx, int dev, const struct infw_xdp_ring *rings, uint32_t n_rings,
                            void *stream);
/* infw_classify_xdp_rings plus the step a daemon takes next, on the device:    */
/* every ring partitioned by its frames' verdicts into a forward list and a    */
/* fill list.  With the same `rings` it computes what infw_classify_xdp_rings  */
/* computes (result words, verdicts, counters, each frame counted once, a      */
/* ring's NULL results or verdicts skipped — both may be NULL: the call then   */
/* classifies and splits only) and, on the same stream against the same epoch, */
/* for ring r:                                                                 */
/*   - split[r].pass[0 .. n_pass[r]): the descriptors of ring r whose frame's  */
/*     verdict is INFW_XDP_PASS, in ring order, copied verbatim (addr, len,    */
/*     options).  Every descriptor of a chain has its head's verdict, so       */
/*     chains stay whole and contiguous; a chain left open at the ring's last  */
/*     descriptor is copied as it is;                                          */
/*   - split[r].fill[0 .. rings[r].n - n_pass[r]): addr & (2^48 - 1)           */
/*     (xsk_umem__extract_addr; the kernel masks it to the chunk in aligned    */
/*     mode) of every other descriptor — DROP and ABORTED — in ring order;     */
/*   - n_pass[r], written for every r: 0 for a ring with n == 0;               */
/*   - a NULL pass or fill skips that list for that ring only, its count is    */
/*     still written; slots at or past the counts are not written.             */
/* pass, fill and n_pass are device-writable; pass 16-byte, fill 8-byte,       */
/* n_pass 4-byte aligned; a ring's lists hold rings[r].n slots each.  `rings`  */
/* and `split` are ordinary host arrays, free when the call returns;           */
/* asynchronous, no host-side wait.  Errnos as infw_classify_xdp_rings, plus   */
/* -EINVAL for a NULL split or n_pass with n_rings > 0 and for a misaligned    */
/* pass or fill in a ring with n > 0.  -ENOMEM: the scratch of                 */
/* infw_classify_xdp_rings plus 8 B per chunk (its pass mask), 32 B per        */
/* non-empty ring (the output table) and 4 B, each array rounded up to 16 B.   */
/* Nothing is launched when an error is returned (n_pass is not zeroed         */
/* either); n_rings == 0 returns 0.                                            */
struct infw_xdp_ring_split {             /* one per ring, same order as rings[] */
    struct infw_xdp_desc *pass;          /* rings[r].n slots, 16-B aligned, or NULL */
    uint64_t *fill;                      /* rings[r].n slots, 8-B aligned, or NULL  */
};
int infw_classify_xdp_rings_split(infw_ctx *ctx, int dev, const struct infw_xdp_ring *rings,
                                  const struct infw_xdp_ring_split *split, uint32_t n_rings,
                                  uint32_t *n_pass /* device, n_rings words */, void *stream);
/* The host packer of infw_classify_xdp_host alone, on the calling thread: one */
/* ring's frames -> the family-compact streams in host memory (the layout       */
/* infw_classify_c reads; out->ifindex may be NULL, else it is filled with      */
/* `ifindex`), for a caller that moves the tuples itself.  Pure host function:  */
/* no context or device.  Every stream 4-byte aligned.                          */
int infw_pack_xdp_host(const uint8_t *umem, const struct infw_xdp_desc *descs, uint64_t n, uint32_t ifindex,
                       const struct infw_batch_soa_c_out *out);

/* ------------------------------------------------------------------------ */
/* Sidebands of the data path, opt-in per batch (infw_classify_ex).          */
/*  - Deny events (kernel.c:392-399, ingress_node_firewall_events_map): one  */
/*    record per DROP-by-rule packet: the 8-B event_hdr_st the program       */
/*    emits plus where the min(len, 256) packet bytes of the perf record     */
/*    live (the batch index).  Records are appended with one atomic per      */
/*    wave; order across waves is unspecified, like perf records across      */
/*    CPUs; *events_count counts every event, also those beyond events_cap   */
/*    (perf "lost samples").                                                  */
/* ------------------------------------------------------------------------ */
struct infw_event_rec {
    struct event_hdr_st hdr;      /* ifId, ruleId, action (1), pad, pktLength (u16 truncations) */
    uint32_t captured;            /* min(pkt_len, INFW_MAX_EVENT_DATA)                          */
    uint32_t reserved;
    uint64_t pkt_index;           /* batch index of the packet the record belongs to             */
};

struct infw_classify_ex {
    uint32_t size;                /* sizeof(struct infw_classify_ex)                              */
    uint32_t flags;               /* reserved, 0                                                 */
    struct infw_event_rec *events;   /* device buffer, or NULL: no event stream                  */
    uint64_t events_cap;
    uint64_t *events_count;       /* device u64, incremented by the kernel                       */
};

int infw_classify_ex(infw_ctx *ctx, int dev, const struct infw_batch_soa *in, uint64_t n,
                     uint32_t *result_words, uint8_t *xdp_verdicts,
                     const struct infw_classify_ex *ex, void *stream);
/* infw_classify_frames with the sidebands: the event records' pkt_index is   */
/* the frame's index in the batch, so infw_events_capture over the same       */
/* frames writes the perf samples.                                            */
int infw_classify_frames_ex(infw_ctx *ctx, int dev, const struct infw_frame_batch *frames, uint64_t n,
                            uint32_t *result_words, uint8_t *xdp_verdicts,
                            const struct infw_classify_ex *ex, void *stream);

/* infw_classify_xdp_mb with the sidebands; ex == NULL is infw_classify_xdp_mb */
/* itself (same result words, verdicts and counters either way).  With         */
/* ex->events it appends one record per frame (descriptor chain) a rule        */
/* denies, with infw_classify_frames_ex's discipline (one atomic per wave,     */
/* order across waves unspecified, *events_count counts past events_cap):      */
/* hdr.ifId = (u16)ifindex, hdr.ruleId, hdr.action = 1, hdr.pktLength =        */
/* (u16)(sum of the chain's len) — bpf_xdp_get_buff_len(), kernel.c:372 —,     */
/* captured = min(sum, 256), and pkt_index = the RING index of the frame's     */
/* head descriptor, which is what infw_events_capture_xdp takes.  Records      */
/* already in the buffer (below *events_count at the call) are not touched.    */
/* A ring whose options are all 0 is a single-buffer ring: this is the event   */
/* stream of infw_classify_xdp too.  ex is validated as in                     */
/* infw_classify_frames_ex (-EINVAL); other errnos as infw_classify_xdp_mb.    */
int infw_classify_xdp_mb_ex(infw_ctx *ctx, int dev, const uint8_t *umem, const struct infw_xdp_desc *descs,
                            uint64_t n, uint32_t ifindex, uint32_t *result_words, uint8_t *xdp_verdicts,
                            const struct infw_classify_ex *ex, void *stream);

/*  - Deny-event payload: the perf sample each record stands for, as the      */
/*    reader receives it (kernel.c:392-399: bpf_perf_event_output(ctx, map,   */
/*    BPF_F_CURRENT_CPU | min(len, 256) << 32, &hdr, 8); events.go:77-96       */
/*    reads perf.Record.RawSample).  Slot k of `samples` belongs to record k    */
/*    of the event ring: `size` is perf's raw-size field,                       */
/*    round_up(8 + captured + 4, 8) - 4, and raw[0 .. size) is event_hdr_st,    */
/*    then the frame's first `captured` bytes, then perf's alignment pad        */
/*    (written as zeros; the kernel leaves stale ring bytes there).  Frame     */
/*    bytes past the frame's linear length (XDP multi-buffer frags, which HBM  */
/*    frames do not carry) are written as zeros.  Bytes past `size` are zero.  */
#define INFW_EVENT_SAMPLE_BYTES 272   /* 4 + round_up(8 + 256 + 4, 8) - 4       */
struct infw_event_sample {
    uint32_t size;
    uint8_t raw[INFW_EVENT_SAMPLE_BYTES - 4];
};
/* Fill samples[k] for k < min(*events_count, events_cap) — the records       */
/* infw_classify_ex wrote — from the n_frames frames the batch was packed     */
/* from (record.pkt_index = frame index; a record whose index is >= n_frames  */
/* gets its header and no frame bytes).  Stream-ordered after the classify: the */
/* count is read on the device, no host synchronisation.  samples: device     */
/* memory of events_cap slots.                                                 */
int infw_events_capture(infw_ctx *ctx, int dev, const struct infw_frame_batch *frames, uint64_t n_frames,
                        const struct infw_event_rec *events, uint64_t events_cap,
                        const uint64_t *events_count, struct infw_event_sample *samples, void *stream);

/* The same for the records of infw_classify_xdp_mb_ex over the same ring: the */
/* reference program is SEC("xdp.frags") and bpf_perf_event_output copies the  */
/* sample's bytes across the frame's fragments, so slot k holds the first      */
/* `captured` bytes of the CONCATENATION of the chain's buffers, in            */
/* infw_events_capture's layout (size word, header, bytes, zeros to 272).  The */
/* chain is descriptor h = pkt_index and the descriptors after it, up to and   */
/* including the first with PKT_CONTD clear, or n-1.  Frame byte b is byte     */
/* b - S_j of descriptor j, where S_j is the sum of len over h..j-1 and        */
/* S_j <= b < S_j + len_j, read at                                             */
/* umem + (addr_j & (2^48-1)) + (addr_j >> 48) + (b - S_j).  Zero-length       */
/* descriptors contribute nothing.  A record with pkt_index >= n (a record of  */
/* another batch) gets its size and header and no frame bytes.  No byte        */
/* outside [buffer_j, buffer_j + len_j) of a chain member and no descriptor at */
/* index >= n is read, and the walk stops once `captured` bytes are placed.    */
/* This is the one call that dereferences a continuation descriptor's addr.    */
/* Stream-ordered after the classify (the count is read on the device).        */
/* Memory checks, alignment and -EFAULT as infw_classify_xdp_mb; samples:      */
/* device memory of events_cap slots, 8-byte aligned.                          */
int infw_events_capture_xdp(infw_ctx *ctx, int dev, const uint8_t *umem, const struct infw_xdp_desc *descs,
                            uint64_t n, const struct infw_event_rec *events, uint64_t events_cap,
                            const uint64_t *events_count, struct infw_event_sample *samples, void *stream);

/* infw_classify_xdp_rings with the deny-event stream.  ex == NULL or           */
/* ex->events == NULL is infw_classify_xdp_rings itself (same result words,    */
/* verdicts and counters either way).  With ex->events it appends one record   */
/* per frame (descriptor chain) a rule denies, with infw_classify_xdp_mb_ex's  */
/* discipline (one atomic per wave, order across waves unspecified,            */
/* *events_count counts past events_cap; records already in the buffer are not */
/* touched): hdr.ifId = (u16) the ring's own ifindex, hdr.pktLength = (u16)    */
/* the chain's summed len, captured = min(sum, 256), and pkt_index = the FLAT  */
/* index of the frame's head descriptor: the sum of rings[q].n over q < r,     */
/* plus i, for descriptor i of rings[r] (empty rings add nothing; the caller   */
/* gets ring and i back with its own prefix sums).                             */
/* With ex->samples too (the fused capture) the call also writes samples[k]    */
/* for the records it appended — slots [count before, min(count after,         */
/* events_cap)) — from the ring table it already has on the device; slots of   */
/* earlier records are left as they are.  samples: device memory of events_cap */
/* slots, 8-byte aligned.  Sample bytes as infw_events_capture_xdp defines     */
/* them, the chain bounded by its OWN ring: it ends at the first descriptor    */
/* with PKT_CONTD clear or at the ring's last descriptor; no descriptor of     */
/* another ring is read, and no byte outside [buffer_j, buffer_j + len_j) of a */
/* chain member.  A caller who wants the samples in packet order                */
/* (infw_events_sort) uses the stand-alone capture after the sort, not the     */
/* fused `samples`: the fused samples lie in the order the records were        */
/* appended.                                                                   */
/* Errnos as infw_classify_xdp_rings, plus -EINVAL for size <                  */
/* sizeof(struct infw_xdp_rings_ex), flags != 0, events without events_count,  */
/* samples without events, samples not 8-byte aligned.  -ENOMEM: the scratch   */
/* of infw_classify_xdp_rings plus, with events, 4 B per descriptor and 8 B.   */
/* Nothing is launched when an error is returned.                              */
struct infw_xdp_rings_ex {
    uint32_t size;                      /* sizeof(struct infw_xdp_rings_ex) */
    uint32_t flags;                     /* 0 */
    struct infw_event_rec *events;      /* device buffer, or NULL: no event stream */
    uint64_t events_cap;
    uint64_t *events_count;             /* device u64 */
    struct infw_event_sample *samples;  /* device, events_cap slots, 8-B aligned, or NULL */
};
int infw_classify_xdp_rings_ex(infw_ctx *ctx, int dev, const struct infw_xdp_ring *rings, uint32_t n_rings,
                               const struct infw_xdp_rings_ex *ex, void *stream);
/* The stand-alone capture, for a caller that sizes `samples` after reading    */
/* the count: the same `rings` array in the same order, samples[k] for every   */
/* k < min(*events_count, events_cap).  Stream-ordered after the classify (the */
/* count is read on the device).  A record with pkt_index >= the sum of the    */
/* rings' n (a record of another batch) gets its size and header and no frame  */
/* bytes.  Rings validated as by infw_classify_xdp_rings (results / verdicts   */
/* are not used); -EINVAL also for events_cap != 0 with a NULL events,         */
/* events_count or samples, or samples not 8-byte aligned; -ENOMEM: no scratch */
/* for the ring table (48 B per non-empty ring from the context's pool).       */
int infw_events_capture_xdp_rings(infw_ctx *ctx, int dev, const struct infw_xdp_ring *rings, uint32_t n_rings,
                                  const struct infw_event_rec *events, uint64_t events_cap,
                                  const uint64_t *events_count, struct infw_event_sample *samples, void *stream);

/*  - Decoded deny events: what the events reader makes of each perf sample     */
/*    before it prints (events.go:77-166): the sample's header, the packet cut   */
/*    to PktLength, and gopacket's eager Ethernet -> IPv4 / IPv6 -> TCP / UDP /  */
/*    SCTP / ICMP decode of it, for the first layer of each type the syslog      */
/*    lines carry.  infw/events.py (decode_sample, gopacket_layers) is the       */
/*    specification, quirks included: IPv4, IPv6, TCP, UDP and SCTP layers exist */
/*    even when their decode fails (nil addresses / zero ports), ICMP layers     */
/*    only on success, IPv4 payloads are cut to the total length, fragments stop */
/*    at the IPv4 layer, IPv6 extension headers are not followed.  A 64-B record */
/*    per 272-B sample: the host is left with the formatting.                    */
#define INFW_EVL_IPV4   0x01u   /* a layer of that type exists (Packet.Layer(t) != nil) */
#define INFW_EVL_IPV6   0x02u
#define INFW_EVL_TCP    0x04u
#define INFW_EVL_UDP    0x08u
#define INFW_EVL_SCTP   0x10u
#define INFW_EVL_ICMPV4 0x20u
#define INFW_EVL_ICMPV6 0x40u
#define INFW_EVL_IP4_ADDRS 0x100u  /* ip4_src/ip4_dst hold addresses (else Go's nil: "<nil>") */
#define INFW_EVL_IP6_ADDRS 0x200u
#define INFW_EVL_SHORT  0x40000000u /* body shorter than pktLength: binary.Read fails, no lines */
#define INFW_EVL_BADHDR 0x80000000u /* size < 8: "Parsing perf event header" */
struct infw_event_decoded {          /* 64 B, no holes; arrays of it 16-B aligned */
    struct event_hdr_st hdr;         /*  0 copied from the sample (zeros with BADHDR) */
    uint32_t layers;                 /*  8 INFW_EVL_* */
    uint16_t body;                   /* 12 size - 8: bytes behind the header (0 -> "EOF", else "unexpected EOF"); */
                                     /*    a size above 268 counts as 268, 0 with BADHDR */
    uint8_t icmp_type, icmp_code;    /* 14 first ICMPv4 / ICMPv6 layer */
    uint16_t sport, dport;           /* 16 first TCP / UDP / SCTP layer, host order; 0/0 when its decode failed */
    uint8_t ip4_src[4], ip4_dst[4];  /* 20 first IPv4 layer */
    uint8_t ip6_src[16], ip6_dst[16];/* 28 first IPv6 layer */
    uint8_t pad[4];                  /* 60 zero */
};
/* decoded[k] for k < min(*events_count, events_cap), from samples[k] alone: no */
/* other slot of either array is read or written, and a written record is       */
/* written whole (unused fields and pad zero).  A record with SHORT or BADHDR   */
/* has no layer bits.  Nothing a sample holds makes the call read outside that  */
/* sample's 272 bytes.  Stream-ordered after the capture: the count is read on  */
/* the device, no host synchronisation; asynchronous.  samples, decoded: device */
/* memory of events_cap slots, 8-byte and 16-byte aligned.  -EINVAL: a NULL     */
/* samples, events_count or decoded with events_cap != 0, or a misaligned       */
/* samples / decoded; -ENODEV: a host-only context; events_cap == 0 returns 0   */
/* and launches nothing.  The host form is infw_events_decode_host              */
/* (infw_host.h): byte-identical records.                                       */
int infw_events_decode(infw_ctx *ctx, int dev, const struct infw_event_sample *samples, uint64_t events_cap,
                       const uint64_t *events_count, struct infw_event_decoded *decoded, void *stream);

/*  - Deny events in packet order: the records of a buffer sorted on the device,  */
/*    between the classify that appended them and the capture that reads them.   */
/*    One AF_XDP ring is one NIC queue and one CPU, whose perf records reach the */
/*    reader in arrival order (kernel.c:392-399, events.go:77-96); the classify  */
/*    kernels append in no order across waves (above).                           */
/* Ordering: let m = min(*events_count, events_cap), read on the device.         */
/* Afterwards events[0 .. m) holds the same m records, ordered by                */
/* key = min(pkt_index, index_bound) ascending; each record is written whole     */
/* (24 B, `reserved` included).                                                  */
/* Stability: records with equal keys keep their relative order, so the records  */
/* of several calls that share a buffer stay grouped as appended, and records of */
/* another batch (pkt_index >= index_bound) end up last, in their original       */
/* order.                                                                        */
/* index_bound: the caller's exclusive bound on pkt_index — the batch's n, or    */
/* the rings' flat total.  It lets the host choose the number of 8-bit digit     */
/* passes (ceil(bits(index_bound) / 8)) without reading anything back;           */
/* index_bound == 0 means the full 64-bit key (8 passes).                        */
/* Untouched memory: events[m .. events_cap) and *events_count are neither read  */
/* nor written.  If records were lost (*events_count > events_cap) the set that  */
/* was kept stays whatever the classify kept; the sort only orders it.           */
/* Stream order: after the classify, before the capture — infw_events_capture*   */
/* and infw_events_decode work slot by slot from events[k], so samples and       */
/* decoded records then come out in packet order.  Asynchronous: the count is    */
/* read on the device, no host synchronisation, no wait for work already queued. */
/* -EINVAL: a NULL events or events_count with events_cap != 0, events not       */
/* 8-byte aligned, events_cap >= 2^32.  -ENODEV: a host-only context.  -ENOMEM:  */
/* no per-call scratch from the context's pool — 40 B per slot of events_cap     */
/* (the record's copy and two 8-B {key, slot} pairs; 48 B when index_bound is 0  */
/* or above 2^32 - 1), 1 KiB per 2048 slots and 1 KiB, each array rounded up to  */
/* 16 B; nothing of it outlives the call.  -EIO: a launch error.  events_cap ==  */
/* 0 returns 0 and launches nothing.  Nothing is launched when an error is       */
/* returned.                                                                     */
int infw_events_sort(infw_ctx *ctx, int dev, struct infw_event_rec *events, uint64_t events_cap,
                     const uint64_t *events_count, uint64_t index_bound, void *stream);

/* Host-resident batch: the SoA streams, result words and verdicts live in   */
/* host memory (as a cgo caller hands them over).  The batch goes through    */
/* the device in chunks of `chunk` packets (0 = 4M) with three HIP streams:  */
/* the H2D copy of chunk k+1 and the D2H copy of chunk k-1 overlap the       */
/* kernel on chunk k; two sets of chunk buffers per device are owned by the  */
/* context.  The whole batch reads one table epoch.  Synchronous: returns    */
/* when every result is in host memory.  Full PCIe rate needs pinned or      */
/* registered host memory (hipHostMalloc / infw_host_register); pageable     */
/* memory is correct but staged by the HIP runtime.  Statistics accumulate   */
/* in the device's slot exactly as for infw_classify.                         */
int infw_classify_host(infw_ctx *ctx, int dev, const struct infw_batch_soa *host_in, uint64_t n,
                       uint32_t *host_results, uint8_t *host_verdicts, uint64_t chunk);
/* Page-lock (hipHostRegister) / release a host range for infw_classify_host. */
int infw_host_register(infw_ctx *ctx, void *ptr, uint64_t bytes);
int infw_host_unregister(infw_ctx *ctx, void *ptr);

/* ------------------------------------------------------------------------ */
/* Statistics — ingress_node_firewall_statistics_map (kernel.c:36-41,        */
/* PERCPU_ARRAY[1024] of ruleStatistics_st).  One slot per device plays the  */
/* role of one per-CPU slot; readers sum slots like statistics.go:126-157.   */
/*                                                                          */
/* Where the multi-GPU sum happens — the library never runs a collective:   */
/*  - one process, one context over N devices (the node daemon's shape):    */
/*    each device slot counts its own batches; infw_stats_read returns the  */
/*    N per-slot values (the []BpfRuleStatisticsSt of one per-CPU lookup)   */
/*    and the caller sums them, as statistics.go:132-156 does;              */
/*    infw_stats_read_all returns that sum (u64 wrap-around) for all rules; */
/*  - one process per GPU (torch.distributed / RCCL ranks): each rank's     */
/*    context has one slot; a caller that wants node totals binds the slot  */
/*    to its own device buffer (infw_stats_bind) and all-reduces it with    */
/*    its communicator (bench.py: an async RCCL all-reduce), or reads each  */
/*    rank's slot and sums on the host — the per-CPU sum again.             */
/* Reads are snapshots: a lookup copies the slot on a stream of its own and  */
/* waits for nothing queued on other streams (batches in flight keep adding,*/
/* like XDP on other CPUs while statistics.go polls).                       */
/* ------------------------------------------------------------------------ */
/* Map.Lookup(uint32(rule), &[]BpfRuleStatisticsSt)  statistics.go:127       */
/* per_slot must hold infw_num_devices() entries; -ENOENT for rule >= 1024.   */
int infw_stats_read(infw_ctx *ctx, uint32_t rule_id, struct ruleStatistics_st *per_slot,
                    int *n_slots);
/* All 1024 rules summed over slots (u64 wrap-around like the kernel).        */
int infw_stats_read_all(infw_ctx *ctx, struct ruleStatistics_st out[INFW_MAX_TARGETS]);
int infw_stats_reset(infw_ctx *ctx);
/* Redirect device `dev`'s statistics slot to caller-owned device memory of   */
/* 1024*32 B (e.g. a tensor that an RCCL all-reduce then sums across GPUs).   */
/* NULL restores the context-owned slot.  Contents are not copied.            */
int infw_stats_bind(infw_ctx *ctx, int dev, uint64_t *device_stats);
/* Device pointer of device `dev`'s current statistics slot.                  */
int infw_stats_device_ptr(infw_ctx *ctx, int dev, uint64_t **device_stats);

/* ------------------------------------------------------------------------ */
/* Debug lookup capture — ingress_node_firewall_dbg_map (kernel.c:59-64,     */
/* HASH of lpm_ip_key_st -> lpm_ip_key_st, 16384 entries) filled with        */
/* bpf_map_update_elem(key, key, BPF_NOEXIST) for every lookup key while the */
/* load-time constant debug_lookup != 0 (kernel.c:78, :214-216, :297-299;    */
/* loader.go:72-83 sets it from ENABLE_EBPF_LPM_LOOKUP_DBG).                 */
/* Key inserted: packets whose L4 header was extracted (not UNDEF), before   */
/* the LPM: {prefixLen 64, ifindex, saddr, 12 zero bytes} for IPv4,          */
/* {160, ifindex, saddr[16]} for IPv6.  Existing keys are left alone; once   */
/* INFW_DBG_MAX_ENTRIES distinct keys are held, new keys are dropped.        */
/* One set per device (like one map per node); reads return their union,    */
/* capped at INFW_DBG_MAX_ENTRIES.  Keys are deduplicated on the device by a */
/* 64-bit fingerprint of the 24-B key.  Which keys fill the last places when */
/* more arrive at once is decided by the device's atomic order (the          */
/* reference's by the CPUs' order).                                          */
/* ------------------------------------------------------------------------ */
#define INFW_DBG_MAX_ENTRIES 16384
/* debug_lookup rewrite at load (loader.go:72-83).  Non-zero allocates the   */
/* per-device key sets on first use; 0 stops capturing (keys are kept).      */
int infw_debug_lookup_set(infw_ctx *ctx, uint32_t debug_lookup);
/* Map iteration of the dbg map: copies up to cap keys, *n = keys held.       */
/* Waits for work queued on the devices.                                      */
int infw_debug_keys_read(infw_ctx *ctx, struct lpm_ip_key_st *keys, uint32_t cap, uint32_t *n);
/* Delete every key of the dbg map (all devices).                             */
int infw_debug_keys_clear(infw_ctx *ctx);

/* ------------------------------------------------------------------------ */
/* Control-plane encoders — the Go helpers whose byte output is the contract */
/* of the table map.  Pure host functions (no device needed).                */
/* ------------------------------------------------------------------------ */
/* BuildEBPFKey(ifID, cidr)  loader.go:530-547.  -EINVAL on a bad CIDR.      */
int infw_build_ebpf_key(uint32_t if_id, const char *cidr, struct lpm_ip_key_st *key);
/* One IngressNodeFirewallProtocolRule -> rulesVal_st slot [order]            */
/* (makeIngressFwRulesMap loader.go:435-515, utils.go:13-60).                 */
/*   protocol: "TCP","UDP","SCTP","ICMP","ICMPv6" or "" (no protocolConfig)   */
/*   ports:    "N" or "A-B" (TCP/UDP/SCTP), NULL/"" otherwise                 */
/*   action:   "Allow" or "Deny"                                              */
/* -EINVAL for the cases the Go code rejects; -E2BIG for order >= 100 (the Go */
/* code panics on an out-of-range array index there, loader.go:437).          */
int infw_make_rule(struct rulesVal_st *val, uint32_t order, const char *protocol,
                   const char *ports, uint8_t icmp_type, uint8_t icmp_code,
                   const char *action);

/* ------------------------------------------------------------------------ */
/* Introspection for tests and the bench.                                     */
/* ------------------------------------------------------------------------ */
struct infw_table_info {
    uint64_t epoch;            /* number of successful commits                */
    uint64_t n_entries;        /* committed LPM entries                       */
    uint32_t n_if_slots;       /* distinct ingress ifindexes                  */
    uint32_t n_lists;          /* interned rule lists                         */
    uint64_t n_rules;          /* GPU rule records over all lists/classes     */
    uint64_t n_tbl8_groups;    /* DIR-24-8 second-level groups                */
    uint32_t n_long_levels;    /* distinct IPv6 prefix lengths > /32          */
    uint64_t n_long_entries;   /* long-prefix hash entries incl. markers      */
    uint64_t device_bytes;     /* table bytes resident per device             */
    double compile_ms;         /* host compile time of the last commit        */
    double upload_ms;          /* H2D time of the last commit                 */
    uint64_t n_v6_groups;      /* (ifindex, /32) groups of IPv6 long prefixes */
    uint64_t n_v6_overflow;    /* groups in the Waldvogel table (> 3 long      */
                               /* prefixes; > 2 in the two-choice slot form)  */
    uint32_t commit_mode;      /* INFW_COMMIT_*: how the last commit ran      */
    uint32_t dt_parts;         /* value parts per (list, class) decision table */
    uint64_t patch_bytes;      /* bytes copied to the devices by it           */
    uint64_t dead_lists;       /* compiled lists no entry references (GC'd by */
                               /* the next full compile)                      */
    char full_reason[48];      /* why the last full compile was needed        */
    uint64_t reserved0;        /* zero (ABI 3: the removed two-choice IPv6     */
                               /* slot form)                                   */
    uint32_t short_mode;       /* <= /32 key space: 0 DIR-24-8, 1 compressed   */
                               /* 16-8-8, 2 none                               */
    uint32_t reserved1;        /* zero (ABI 3: the removed range form)         */
    /* ABI 3: commit timing per device slot (the slots upload / patch in        */
    /* parallel, one host thread each) and room to grow without another break.  */
    double device_ms_max;      /* slowest slot's upload / patch of the last     */
                               /* commit (wall, host thread of that slot)      */
    uint32_t n_device_slots;   /* slots the last commit published to            */
    uint32_t imported;         /* 1: the epoch came from infw_table_import      */
    uint32_t d16;              /* 1: /16 words in front of DIR-24-8 (sparse     */
                               /* short tables; chosen per full compile)       */
    uint32_t d16_permille;     /* of the /16s holding a prefix longer than /16, */
                               /* those a /16 word answers alone               */
    uint32_t split;            /* 1: the epoch classifies in two phases (LPM   */
                               /* -> decision-line address per packet, then   */
                               /* the decision lines as independent gathers):  */
                               /* many distinct rule lists (option split)      */
    uint32_t dt_half_reads;    /* 1: decision lines read half-first (nearly all */
                               /* compact leaves of <= 9 segments; dt_half)    */
    uint64_t reserved[12];     /* zero; future fields come out of this         */
};
#define INFW_COMMIT_FULL 0u        /* compile + upload of a fresh image           */
#define INFW_COMMIT_INCREMENTAL 1u /* patched ranges copied into the spare image  */
#define INFW_COMMIT_REUPLOAD 2u    /* patched host image, re-uploaded (grew)     */
int infw_table_info(infw_ctx *ctx, struct infw_table_info *info);
/* Verification hook for tests/ only — never called by infw_classify: walks     */
/* the last committed HOST table image (INFW_F_HOST_ONLY or                      */
/* INFW_F_KEEP_HOST_IMAGE contexts) with the same lookup code the kernel runs,   */
/* so the table compiler can be checked against the oracle on a CPU-only box.   */
/* tuples: n x 8 u32 {saddr[4], ifindex, pkt_len, meta, l4word}.                */
/* out: result words (same meaning as infw_classify's).  -ENODATA w/o image.    */
int infw_debug_walk(infw_ctx *ctx, const uint32_t *tuples, uint64_t n, uint32_t *out);
/* Last error string of this thread (static storage).                          */
const char *infw_last_error(void);
/* ABI version (bumped on incompatible change).  3: struct infw_table_info     */
/* grew (and now ends in reserved space), infw_build_id, table export/import. */
/* 4: per-context options replace environment variables, infw_set_launch      */
/* accepts only the registered shapes, kernel-variant introspection.          */
#define INFW_ABI_VERSION 4
int infw_abi_version(void);
/* Identity of the code this library was built from: a hash of the kernel and */
/* table-layout sources and the flags they were compiled with (Makefile).       */
/* Profiles taken on one build are only valid for the same build id.           */
const char *infw_build_id(void);

/* ------------------------------------------------------------------------ */
/* Compiled-epoch images: compile once, install on many contexts.  The        */
/* reference has one daemon per node driving one map (ebpfsyncer.go:70-125);  */
/* here one process per GPU each holds a context, and instead of every rank    */
/* compiling the same 1M-entry set, one exports its committed epoch (the      */
/* entry set, the compiled host tables and the incremental-commit state) and  */
/* the others import it.                                                       */
/* ------------------------------------------------------------------------ */
/* Serialise the last committed epoch.  buf == NULL: *size = bytes needed.     */
/* -EBUSY when the pending set has uncommitted edits, -ENOSPC when cap is too  */
/* small (*size says how much is needed).                                      */
int infw_table_export(infw_ctx *ctx, void *buf, uint64_t cap, uint64_t *size);
/* Install an exported epoch into a context whose map is empty: the entries    */
/* become the committed set (get_next_key / lookup / later incremental commits */
/* work as after a commit) and every device slot gets the image — no compile.  */
/* -EBUSY: the context holds entries or uncommitted edits (one whose entries   */
/* were all removed and committed counts as empty); -EINVAL: not an image of  */
/* this library build (infw_build_id), truncated, a payload that does not     */
/* match the header's XXH64, or compiled tables that fail the structural      */
/* checks (an index outside its buffer, a probe table without a free slot) —  */
/* nothing is installed or uploaded then; -ENOSPC: more entries than          */
/* max_entries.                                                               */
int infw_table_import(infw_ctx *ctx, const void *buf, uint64_t size);

#ifdef __cplusplus
}
#endif
#endif /* INFW_H */
