// infw_evdecode.h — one perf sample (include/infw.h: infw_event_sample) -> one decoded record (infw_event_decoded).
//
// The step of the events reader behind the sample (pkg/ebpf/ingress_node_firewall_events.go:77-166): the sample's
// header, the packet cut to PktLength, and gopacket's eager decode of it for the layers the syslog lines carry.
// infw/events.py (decode_sample + gopacket_layers) is the specification; this restates it once, over a byte reader,
// for the host (infw_events_decode_host, hostfeed.cpp) and for the device (evdecode.hip, the reader over LDS).
//
// The reader R addresses the 272-B slot by byte offset:
//   uint32_t R::byte(uint32_t o)   the byte at o
//   uint32_t R::word(uint32_t o)   the 4 bytes at o .. o + 3 as a little-endian word (any alignment)
// Every offset handed to it is below 12 + min(pktLength, body, 260) <= 272 (12 = size word + header; the size and
// header words themselves are at 0, 4 and 8), and that is checked before the read: the parse cannot leave the slot
// whatever the sample holds.  A size word above 268 (no writer of the layout produces one) counts as 268, which is
// what the slot can hold; garbage decodes to a garbage record, never to a read elsewhere.
//
// The record comes back as its 16 little-endian words (the layout is include/infw.h's):
//   0-1 hdr   2 layers   3 body | icmp_type << 16 | icmp_code << 24   4 sport | dport << 16
//   5 ip4_src   6 ip4_dst   7-10 ip6_src   11-14 ip6_dst   15 pad (0)
// Usable from host C++ and from HIP device code.
#pragma once
#include <stdint.h>

#include "../../include/infw.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define INFW_EVD_FN __host__ __device__ __forceinline__
#define INFW_EVD_MEMBER __host__ __device__ __forceinline__
#else
#define INFW_EVD_FN static inline
#define INFW_EVD_MEMBER inline
#endif

#define INFW_EVD_WORDS 16  // sizeof(struct infw_event_decoded) / 4
// IP headers one packet can nest: a body holds at most 260 bytes, 14 of them Ethernet, and every IP layer that lets
// the decode go on is at least 20 bytes: 12 whole headers, and one more that is cut short (it can still add the other
// family's layer, with nil addresses).  gopacket recurses; this loops, at most that many times.
#define INFW_EVD_MAX_IP 13
#define INFW_EVD_MAX_OPTS 40  // option bytes behind an IPv4 header (IHL 15): each step of the walk eats at least one

INFW_EVD_FN uint32_t infw_evd_be16(uint32_t two_bytes) {  // bytes b0 | b1 << 8 in memory order -> b0 << 8 | b1
    return (two_bytes & 0xFFu) << 8 | (two_bytes >> 8 & 0xFFu);
}

template <class R>
INFW_EVD_FN void infw_event_decode(const R &rd, uint32_t w[INFW_EVD_WORDS]) {
    for (int i = 0; i < INFW_EVD_WORDS; i++) w[i] = 0;
    uint32_t size = rd.word(0);
    if (size > INFW_EVENT_SAMPLE_BYTES - 4) size = INFW_EVENT_SAMPLE_BYTES - 4;
    if (size < 8) {  // binary.Read of the 8-B header fails
        w[2] = INFW_EVL_BADHDR;
        return;
    }
    w[0] = rd.word(4);
    w[1] = rd.word(8);
    const uint32_t body = size - 8, n = w[1] >> 16;  // n: pktLength
    w[3] = body;
    if (body < n) {  // binary.Read of PktLength bytes fails
        w[2] = INFW_EVL_SHORT;
        return;
    }
    // the packet: bytes [0, n) of the body, n <= 260; packet byte i is slot byte 12 + i
    if (n <= 14) return;  // < 14: "Ethernet packet too small"; == 14: no payload, no next decoder
    const uint32_t et = rd.byte(12 + 12) << 8 | rd.byte(12 + 13);
    uint32_t kind = et == 0x0800 ? 4u : et == 0x86DD ? 6u : 0u;
    uint32_t layers = 0, p = 14, end = n;  // the current layer's bytes: [p, end), never empty at the loop's head
    for (int depth = 0; depth < INFW_EVD_MAX_IP && kind; depth++) {
        uint32_t len = end - p, proto;
        if (kind == 4) {  // decodeIPv4: the layer is added before the error checks
            const bool first = !(layers & INFW_EVL_IPV4);
            layers |= INFW_EVL_IPV4;
            if (len < 20) break;
            if (first) {
                layers |= INFW_EVL_IP4_ADDRS;
                w[5] = rd.word(12 + p + 12);
                w[6] = rd.word(12 + p + 16);
            }
            const uint32_t h0 = rd.word(12 + p), h1 = rd.word(12 + p + 4), ihl4 = (h0 & 0xFu) * 4;
            const uint32_t ff = infw_evd_be16(h1 >> 16);
            uint32_t length = infw_evd_be16(h0 >> 16);
            proto = rd.byte(12 + p + 9);
            if (length == 0) length = len;  // TSO: the data's length (<= 260, so & 0xFFFF changes nothing)
            if (length < 20 || ihl4 < 20 || ihl4 > length) break;
            if (len > length) {
                end = p + length;
                len = length;
            } else if (len < length && ihl4 > len) {
                break;
            }
            // IPv4.DecodeFromBytes option walk over [p + 20, p + ihl4), ihl4 <= len: its errors end the decode
            uint32_t o = p + 20;
            const uint32_t oe = p + ihl4;
            bool bad = false;
            for (int step = 0; step < INFW_EVD_MAX_OPTS && o < oe; step++) {
                const uint32_t t = rd.byte(12 + o);
                if (t == 0) break;
                if (t == 1) {
                    o++;
                    continue;
                }
                if (oe - o < 2) {
                    bad = true;
                    break;
                }
                const uint32_t ol = rd.byte(12 + o + 1);
                if (oe - o < ol || ol <= 2) {
                    bad = true;
                    break;
                }
                o += ol;
            }
            if (bad) break;
            if ((ff >> 13 & 1u) || (ff & 0x1FFFu)) break;  // IPv4MoreFragments / FragOffset: a Fragment layer
            p += ihl4;
        } else {  // decodeIPv6
            const bool first = !(layers & INFW_EVL_IPV6);
            layers |= INFW_EVL_IPV6;
            if (len < 40) break;
            if (first) {
                layers |= INFW_EVL_IP6_ADDRS;
                for (uint32_t i = 0; i < 8; i++) w[7 + i] = rd.word(12 + p + 8 + 4 * i);
            }
            const uint32_t h1 = rd.word(12 + p + 4), plen = infw_evd_be16(h1);
            proto = h1 >> 16 & 0xFFu;
            if (proto == 0 || plen == 0) break;  // hop-by-hop / jumbogram handling: not restated
            p += 40;
            if (end - p > plen) end = p + plen;
        }
        // eagerPacket.NextDecoder: an empty payload ends the decode
        len = end - p;
        kind = 0;
        if (len == 0) break;
        if (proto == 4) {
            kind = 4;
        } else if (proto == 41) {
            kind = 6;
        } else if (proto == 6 || proto == 17 || proto == 132) {  // the layer always, its ports when the header fits
            layers |= proto == 6 ? INFW_EVL_TCP : proto == 17 ? INFW_EVL_UDP : INFW_EVL_SCTP;
            if (len >= (proto == 6 ? 20u : proto == 17 ? 8u : 12u)) {
                const uint32_t pw = rd.word(12 + p);
                w[4] = infw_evd_be16(pw) | infw_evd_be16(pw >> 16) << 16;
            }
        } else if ((proto == 1 && len >= 8) || (proto == 58 && len >= 4)) {  // decodingLayerDecoder: only on success
            layers |= proto == 1 ? INFW_EVL_ICMPV4 : INFW_EVL_ICMPV6;
            w[3] |= rd.byte(12 + p) << 16 | rd.byte(12 + p + 1) << 24;
        }
    }
    w[2] = layers;
}

// The reader over a slot in ordinary memory (the host form; any alignment).
struct infw_evd_mem_reader {
    const uint8_t *s;
    INFW_EVD_MEMBER uint32_t byte(uint32_t o) const { return s[o]; }
    INFW_EVD_MEMBER uint32_t word(uint32_t o) const {
        return (uint32_t)s[o] | (uint32_t)s[o + 1] << 8 | (uint32_t)s[o + 2] << 16 | (uint32_t)s[o + 3] << 24;
    }
};
