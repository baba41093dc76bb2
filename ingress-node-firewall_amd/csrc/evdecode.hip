// evdecode.hip — infw_events_decode: perf samples -> decoded deny-event records on the device (gfx950).
//
// The samples lie where infw_events_capture* wrote them, 272 B per record; the events reader's next step
// (events.go:77-166: header, packet cut to PktLength, gopacket's Ethernet -> IP -> L4 decode) is a byte-level parse per
// record with data-dependent offsets.  One record per lane, and the parse is infw_evdecode.h's, the same text the host
// form runs; what this file adds is how the bytes reach the lane:
//
//   stage   a wave's 64 slots are 17,408 contiguous bytes = 1088 16-B words.  The wave loads them coalesced — word
//           j = 64 t + lane in trip t of 17, consecutive lanes on consecutive words — and puts word j of slot j / 17
//           into the wave's LDS image at slot * 69 + 4 * (j % 17) dwords.  Words of slots at or past the record count
//           are not loaded (the tail wave), so no byte of another slot is read.
//   image   69 dwords per slot: 68 of sample and one of pad.  The stride is odd, so the 64 lanes of a wave, each at
//           the same offset of its own slot, read 64 distinct banks; and the pad is the high dword of an unaligned
//           word read at offset 268 (its bytes are shifted out, never used).
//   parse   per lane over its own slot in LDS: bytes are ds_read_u8, 4-byte fields (addresses, the header words,
//           the ports) two aligned dword reads and v_alignbyte.  No lane touches global memory in the parse.
//   store   the record's 16 words as four 16-B non-temporal stores per lane, the record whole (pads included).
//
// One wave per workgroup: the image is 17,664 B, so LDS allows 9 workgroups = 9 waves per CU (the remark of
// -Rpass-analysis=kernel-resource-usage states VGPRs and LDS; DESIGN.md §6.2 has the figures), each with 17 KiB of
// loads in flight per trip, which is what a streaming kernel needs.  The grid is min(waves the capacity needs, 9 per
// CU), grid-stride over min(*count, cap) read on the device.  The hand-offs through LDS are inside the wave:
// wave-scope fences and no workgroup barrier (a workgroup is one wave, and waves run different trip counts).
//
// No fault is possible from data: the staging addresses depend on the record count alone, and every offset of the parse
// is bounded by min(pktLength, body, 260) before the read (a size word above 268 counts as 268, infw_evdecode.h), so
// the largest LDS byte offset inside a slot is 271 and the largest dword read is index 68 of 69.  Garbage samples
// decode to garbage records; they never read outside their slot.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "../../include/infw.h"
#include "infw_evdecode.h"
#include "infw_launch.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a8 __attribute__((aligned(8)));  // samples are 8-byte aligned (include/infw.h), not 16

constexpr uint32_t kSlotWords16 = INFW_EVENT_SAMPLE_BYTES / 16;   // 17
constexpr uint32_t kSlotDwords = INFW_EVENT_SAMPLE_BYTES / 4 + 1;  // 69: odd, and one dword behind offset 268
constexpr uint32_t kWaveLds = 64 * kSlotDwords * 4;                // 17,664 B
static_assert(INFW_EVENT_SAMPLE_BYTES % 16 == 0 && (kSlotDwords & 1) == 1, "whole 16-B words, odd dword stride");
static_assert(sizeof(infw_event_decoded) == 64 && sizeof(infw_event_decoded) == 4 * INFW_EVD_WORDS, "four 16-B stores");
constexpr uint32_t kWavesPerCu = 160 * 1024 / kWaveLds;            // 9: the CU's 160 KiB of LDS

// The lane's slot in the wave's LDS image.
struct LdsReader {
    const uint32_t *dw;
    __device__ __forceinline__ uint32_t byte(uint32_t o) const { return reinterpret_cast<const uint8_t *>(dw)[o]; }
    __device__ __forceinline__ uint32_t word(uint32_t o) const {
        const uint32_t lo = dw[o >> 2], hi = dw[(o >> 2) + 1];
        return __builtin_amdgcn_alignbyte(hi, lo, o & 3u);
    }
};

__device__ __forceinline__ void wave_lds_handoff() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(64) void events_decode_kernel(const uint8_t *__restrict__ samples, uint64_t cap,
                                                           const uint64_t *__restrict__ count,
                                                           uint8_t *__restrict__ decoded) {
    __shared__ uint32_t s_img[64 * kSlotDwords];
    const uint32_t lane = threadIdx.x;
    const uint64_t c = *count, n_rec = c < cap ? c : cap;
    for (uint64_t r0 = (uint64_t)blockIdx.x * 64; r0 < n_rec; r0 += (uint64_t)gridDim.x * 64) {
        const uint64_t left = n_rec - r0;
        const uint32_t slots = left < 64 ? (uint32_t)left : 64u;  // wave-uniform
        const u32x4_a8 *__restrict__ src = reinterpret_cast<const u32x4_a8 *>(samples + r0 * INFW_EVENT_SAMPLE_BYTES);
#pragma unroll
        for (uint32_t t = 0; t < kSlotWords16; t++) {
            const uint32_t j = t * 64 + lane, slot = j / kSlotWords16, k = j - slot * kSlotWords16;
            if (slot < slots) {
                const u32x4 v = __builtin_nontemporal_load(src + j);
                uint32_t *const d = s_img + slot * kSlotDwords + 4 * k;
                d[0] = v[0], d[1] = v[1], d[2] = v[2], d[3] = v[3];
            }
        }
        wave_lds_handoff();
        if (lane < slots) {
            uint32_t w[INFW_EVD_WORDS];
            infw_event_decode(LdsReader{s_img + lane * kSlotDwords}, w);
            u32x4 *const out = reinterpret_cast<u32x4 *>(decoded + (r0 + lane) * sizeof(infw_event_decoded));
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const u32x4 v = {w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
                __builtin_nontemporal_store(v, out + q);
            }
        }
        wave_lds_handoff();  // the next trip rewrites the image
    }
}

}  // namespace

extern "C" int infw_launch_events_decode(const infw_event_sample *samples, uint64_t cap, const uint64_t *count,
                                         infw_event_decoded *decoded, uint32_t cus, hipStream_t stream) {
    if (cap == 0) return 0;
    const uint64_t waves = (cap + 63) / 64, lim = (uint64_t)kWavesPerCu * cus;
    hipLaunchKernelGGL(events_decode_kernel, dim3((uint32_t)(waves < lim ? waves : lim)), dim3(64), 0, stream,
                       reinterpret_cast<const uint8_t *>(samples), cap, count, reinterpret_cast<uint8_t *>(decoded));
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
