"""ctypes bindings of libinfw.so (include/infw.h) and libinfw_workload.so.

The shared objects are built in-tree by `make` (or __graft_entry__.build()) into
ingress-node-firewall_amd/lib/.  There is no fallback: if the library is
missing, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(_PKG_DIR, "lib")
LIB_PATH = os.environ.get("INFW_LIB") or os.path.join(LIB_DIR, "libinfw.so")  # INFW_LIB: A/B builds (tools/)
WL_LIB_PATH = os.path.join(LIB_DIR, "libinfw_workload.so")

MAX_TARGETS = 1024
MAX_RULES_PER_TARGET = 100
XDP_ABORTED, XDP_DROP, XDP_PASS = 0, 1, 2
BPF_ANY, BPF_NOEXIST, BPF_EXIST = 0, 1, 2
F_HOST_ONLY = 0x1
F_KEEP_HOST_IMAGE = 0x2
F_FULL_COMMIT = 0x4
COMMIT_FULL, COMMIT_INCREMENTAL, COMMIT_REUPLOAD = 0, 1, 2
HDR_SNAP = 80


class LpmIpKeySt(C.Structure):
    """struct lpm_ip_key_st (bpf/ingress_node_firewall.h:83-87), BpfLpmIpKeySt."""
    _pack_ = 1
    _fields_ = [("prefixLen", C.c_uint32), ("ingress_ifindex", C.c_uint32), ("ip_data", C.c_uint8 * 16)]

    def tobytes(self) -> bytes:
        return bytes(self)

    def __eq__(self, other):  # reflect.DeepEqual on the Go struct == byte equality
        return isinstance(other, LpmIpKeySt) and bytes(self) == bytes(other)

    def __hash__(self):
        return hash(bytes(self))

    def __repr__(self):
        return f"LpmIpKeySt(prefixLen={self.prefixLen}, ifindex={self.ingress_ifindex}, ip={bytes(self.ip_data).hex()})"


class RuleTypeSt(C.Structure):
    """struct ruleType_st (ingress_node_firewall.h:69-77), BpfRuleTypeSt, 12 B packed."""
    _pack_ = 1
    _fields_ = [("ruleId", C.c_uint32), ("protocol", C.c_uint8), ("dstPortStart", C.c_uint16),
                ("dstPortEnd", C.c_uint16), ("icmpType", C.c_uint8), ("icmpCode", C.c_uint8),
                ("action", C.c_uint8)]


class RulesValSt(C.Structure):
    """struct rulesVal_st (ingress_node_firewall.h:89-91), BpfRulesValSt, 1200 B."""
    _pack_ = 1
    _fields_ = [("rules", RuleTypeSt * MAX_RULES_PER_TARGET)]

    def __eq__(self, other):
        return isinstance(other, RulesValSt) and bytes(self) == bytes(other)

    def __hash__(self):
        return hash(bytes(self))


class RuleStatisticsSt(C.Structure):
    """struct ruleStatistics_st (ingress_node_firewall.h:45-54), BpfRuleStatisticsSt."""
    _fields_ = [("allow_packets", C.c_uint64), ("allow_bytes", C.c_uint64),
                ("deny_packets", C.c_uint64), ("deny_bytes", C.c_uint64)]


class BatchSoa(C.Structure):
    """struct infw_batch_soa (include/infw.h)."""
    _fields_ = [("saddr", C.c_void_p), ("ifindex", C.c_void_p), ("pkt_len", C.c_void_p),
                ("meta", C.c_void_p), ("l4word", C.c_void_p)]


class BatchSoaC(C.Structure):
    """struct infw_batch_soa_c (include/infw.h): the family-compact address layout."""
    _fields_ = [("saddr4", C.c_void_p), ("v6tail", C.c_void_p), ("ifindex", C.c_void_p), ("pkt_len", C.c_void_p),
                ("meta", C.c_void_p), ("l4word", C.c_void_p)]


V6_GROUP = 64  # INFW_V6_GROUP


class FrameBatch(C.Structure):
    """struct infw_frame_batch (include/infw.h)."""
    _fields_ = [("frames", C.c_void_p), ("offsets", C.c_void_p), ("stride", C.c_uint64), ("linear_len", C.c_void_p),
                ("pkt_len", C.c_void_p), ("ifindex", C.c_void_p)]


class XdpDesc(C.Structure):
    """struct infw_xdp_desc (include/infw.h) = linux/if_xdp.h struct xdp_desc, 16 B."""
    _fields_ = [("addr", C.c_uint64), ("len", C.c_uint32), ("options", C.c_uint32)]


class XdpRing(C.Structure):
    """struct infw_xdp_ring (include/infw.h): one AF_XDP RX ring (infw_classify_xdp_host, infw_classify_xdp_rings)."""
    _fields_ = [("umem", C.c_void_p), ("descs", C.c_void_p), ("n", C.c_uint64), ("ifindex", C.c_uint32),
                ("flags", C.c_uint32), ("results", C.c_void_p), ("verdicts", C.c_void_p)]


class XdpRingSplit(C.Structure):
    """struct infw_xdp_ring_split (include/infw.h): one ring's forward and fill lists (infw_classify_xdp_rings_split)."""
    _fields_ = [("pass_", C.c_void_p), ("fill", C.c_void_p)]


class FrameBurst(C.Structure):
    """struct infw_frame_burst (include/infw_host.h): a DPDK-style burst of frames in host memory, one pointer each."""
    _fields_ = [("frames", C.c_void_p), ("linear_len", C.c_void_p), ("pkt_len", C.c_void_p), ("n", C.c_uint64),
                ("ifindex", C.c_uint32), ("flags", C.c_uint32), ("results", C.c_void_p), ("verdicts", C.c_void_p)]


class EventHdrSt(C.Structure):
    """struct event_hdr_st (ingress_node_firewall.h:58-64), 8 B packed."""
    _pack_ = 1
    _fields_ = [("ifId", C.c_uint16), ("ruleId", C.c_uint16), ("action", C.c_uint8), ("pad", C.c_uint8),
                ("pktLength", C.c_uint16)]


class EventRec(C.Structure):
    """struct infw_event_rec (include/infw.h), 24 B."""
    _fields_ = [("hdr", EventHdrSt), ("captured", C.c_uint32), ("reserved", C.c_uint32),
                ("pkt_index", C.c_uint64)]


class ClassifyEx(C.Structure):
    """struct infw_classify_ex (include/infw.h)."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("events", C.c_void_p), ("events_cap", C.c_uint64),
                ("events_count", C.c_void_p)]


class XdpRingsEx(C.Structure):
    """struct infw_xdp_rings_ex (include/infw.h)."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("events", C.c_void_p), ("events_cap", C.c_uint64),
                ("events_count", C.c_void_p), ("samples", C.c_void_p)]


EVENT_SAMPLE_BYTES = 272  # INFW_EVENT_SAMPLE_BYTES: u32 perf raw size + raw sample (hdr, <= 256 B, pad)


class EventDecoded(C.Structure):
    """struct infw_event_decoded (include/infw.h), 64 B: what the events reader makes of one perf sample."""
    _fields_ = [("hdr", EventHdrSt), ("layers", C.c_uint32), ("body", C.c_uint16), ("icmp_type", C.c_uint8),
                ("icmp_code", C.c_uint8), ("sport", C.c_uint16), ("dport", C.c_uint16), ("ip4_src", C.c_uint8 * 4),
                ("ip4_dst", C.c_uint8 * 4), ("ip6_src", C.c_uint8 * 16), ("ip6_dst", C.c_uint8 * 16),
                ("pad", C.c_uint8 * 4)]


# INFW_EVL_*: the layers of a decoded record
EVL_IPV4, EVL_IPV6, EVL_TCP, EVL_UDP, EVL_SCTP, EVL_ICMPV4, EVL_ICMPV6 = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40
EVL_IP4_ADDRS, EVL_IP6_ADDRS, EVL_SHORT, EVL_BADHDR = 0x100, 0x200, 0x40000000, 0x80000000


class TableInfo(C.Structure):
    _fields_ = [("epoch", C.c_uint64), ("n_entries", C.c_uint64), ("n_if_slots", C.c_uint32),
                ("n_lists", C.c_uint32), ("n_rules", C.c_uint64), ("n_tbl8_groups", C.c_uint64),
                ("n_long_levels", C.c_uint32), ("n_long_entries", C.c_uint64),
                ("device_bytes", C.c_uint64), ("compile_ms", C.c_double), ("upload_ms", C.c_double),
                ("n_v6_groups", C.c_uint64), ("n_v6_overflow", C.c_uint64),
                ("commit_mode", C.c_uint32), ("dt_parts", C.c_uint32), ("patch_bytes", C.c_uint64),
                ("dead_lists", C.c_uint64), ("full_reason", C.c_char * 48), ("reserved0", C.c_uint64),
                ("short_mode", C.c_uint32), ("reserved1", C.c_uint32),
                ("device_ms_max", C.c_double), ("n_device_slots", C.c_uint32), ("imported", C.c_uint32),
                ("d16", C.c_uint32), ("d16_permille", C.c_uint32), ("split", C.c_uint32),
                ("dt_half_reads", C.c_uint32), ("reserved", C.c_uint64 * 12)]


assert C.sizeof(LpmIpKeySt) == 24 and C.sizeof(RuleTypeSt) == 12
assert C.sizeof(RulesValSt) == 1200 and C.sizeof(RuleStatisticsSt) == 32

# Every symbol include/infw.h declares (checked by tests/test_abi_cpu.py).
DBG_MAX_ENTRIES = 16384  # include/infw.h INFW_DBG_MAX_ENTRIES (kernel.c:63)

ABI_SYMBOLS = [
    "infw_classify_ex", "infw_pack_frames", "infw_create", "infw_destroy", "infw_num_devices", "infw_table_update", "infw_table_update_batch",
    "infw_table_delete", "infw_table_get_next_key", "infw_table_lookup", "infw_table_count",
    "infw_table_commit", "infw_classify", "infw_stats_read", "infw_stats_read_all", "infw_stats_reset",
    "infw_stats_bind", "infw_stats_device_ptr", "infw_build_ebpf_key", "infw_make_rule",
    "infw_table_info", "infw_debug_walk", "infw_set_launch", "infw_last_error", "infw_abi_version",
    "infw_debug_lookup_set", "infw_debug_keys_read", "infw_debug_keys_clear", "infw_classify_host",
    "infw_host_register", "infw_host_unregister", "infw_classify_c", "infw_soa_compact", "infw_pack_frames_c", "infw_classify_frames",
    "infw_classify_frames_ex",
    "infw_get_launch", "infw_events_capture", "infw_build_id", "infw_table_export", "infw_table_import",
    "infw_table_delete_batch", "infw_set_option", "infw_get_option", "infw_option_name", "infw_classify_variant",
    "infw_kernel_variant_name", "infw_classify_xdp", "infw_classify_xdp_mb", "infw_classify_xdp_mb_ex",
    "infw_events_capture_xdp", "infw_classify_xdp_host", "infw_classify_xdp_rings",
    "infw_classify_xdp_rings_ex", "infw_events_capture_xdp_rings", "infw_classify_xdp_rings_split",
    "infw_pack_xdp_host", "infw_launch_counts", "infw_xdp_host_events", "infw_classify_bursts_host",
    "infw_pack_burst_host", "infw_burst_host_events", "infw_events_decode", "infw_events_decode_host",
    "infw_events_sort",
]
ABI_VERSION = 4  # include/infw.h INFW_ABI_VERSION
INPUT_SOA, INPUT_COMPACT, INPUT_FRAMES, INPUT_XDP = 0, 1, 2, 3  # INFW_INPUT_*
VARIANT_EVENTS = 0x1  # INFW_VARIANT_EVENTS
XDP_PKT_CONTD = 1  # INFW_XDP_PKT_CONTD (linux/if_xdp.h): the frame continues in the next descriptor
# csrc/infw_launch.h: descriptors per workgroup of infw_classify_xdp_mb's chain pass, tile summaries per carry round
XDP_CHAIN_TILE, XDP_CHAIN_CARRY = 256, 512
XDP_RINGS_MAX = 1024  # INFW_XDP_RINGS_MAX: rings per infw_classify_xdp_rings call


# torch (device memory, streams, RCCL) ships its own libamdhip64.so.7; loading it
# first makes libinfw bind to that same HIP runtime (same SONAME), so device
# pointers and streams are shared by one runtime in the process.
try:  # pragma: no cover - import side effect only
    import torch as _torch  # noqa: F401
except Exception:  # torch absent: libinfw uses /opt/rocm's runtime
    _torch = None


def _load(path: str) -> C.CDLL:
    if not os.path.exists(path):
        raise ImportError(f"{path} not built: run `make` (or __graft_entry__.build()); "
                          "there is no non-native fallback")
    return C.CDLL(path)


lib = _load(LIB_PATH)
P = C.POINTER
_sig = {
    "infw_create": (C.c_int, [P(C.c_void_p), P(C.c_int), C.c_int, C.c_uint32, C.c_uint32]),
    "infw_destroy": (None, [C.c_void_p]),
    "infw_num_devices": (C.c_int, [C.c_void_p]),
    "infw_table_update": (C.c_int, [C.c_void_p, P(LpmIpKeySt), P(RulesValSt), C.c_uint64]),
    "infw_table_update_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                          C.c_uint64, P(C.c_uint64)]),
    "infw_table_delete": (C.c_int, [C.c_void_p, P(LpmIpKeySt)]),
    "infw_table_delete_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_uint64)]),
    "infw_table_get_next_key": (C.c_int, [C.c_void_p, P(LpmIpKeySt), P(LpmIpKeySt)]),
    "infw_table_lookup": (C.c_int, [C.c_void_p, P(LpmIpKeySt), P(RulesValSt)]),
    "infw_table_count": (C.c_int, [C.c_void_p, P(C.c_uint64)]),
    "infw_table_commit": (C.c_int, [C.c_void_p]),
    "infw_classify": (C.c_int, [C.c_void_p, C.c_int, P(BatchSoa), C.c_uint64, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    "infw_classify_ex": (C.c_int, [C.c_void_p, C.c_int, P(BatchSoa), C.c_uint64, C.c_void_p, C.c_void_p,
                                   P(ClassifyEx), C.c_void_p]),
    "infw_pack_frames": (C.c_int, [C.c_void_p, C.c_int, P(FrameBatch), C.c_uint64, P(BatchSoa), C.c_void_p]),
    "infw_classify_host": (C.c_int, [C.c_void_p, C.c_int, P(BatchSoa), C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.c_uint64]),
    "infw_classify_c": (C.c_int, [C.c_void_p, C.c_int, P(BatchSoaC), C.c_uint64, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "infw_pack_frames_c": (C.c_int, [C.c_void_p, C.c_int, P(FrameBatch), C.c_uint64, P(BatchSoaC), C.c_void_p]),
    "infw_classify_frames": (C.c_int, [C.c_void_p, C.c_int, P(FrameBatch), C.c_uint64, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "infw_classify_frames_ex": (C.c_int, [C.c_void_p, C.c_int, P(FrameBatch), C.c_uint64, C.c_void_p, C.c_void_p,
                                          P(ClassifyEx), C.c_void_p]),
    "infw_events_capture": (C.c_int, [C.c_void_p, C.c_int, P(FrameBatch), C.c_uint64, C.c_void_p, C.c_uint64,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "infw_soa_compact": (C.c_int, [C.c_void_p, C.c_int, P(BatchSoa), C.c_uint64, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "infw_host_register": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "infw_host_unregister": (C.c_int, [C.c_void_p, C.c_void_p]),
    "infw_stats_read": (C.c_int, [C.c_void_p, C.c_uint32, P(RuleStatisticsSt), P(C.c_int)]),
    "infw_stats_read_all": (C.c_int, [C.c_void_p, P(RuleStatisticsSt)]),
    "infw_stats_reset": (C.c_int, [C.c_void_p]),
    "infw_stats_bind": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "infw_stats_device_ptr": (C.c_int, [C.c_void_p, C.c_int, P(C.c_void_p)]),
    "infw_build_ebpf_key": (C.c_int, [C.c_uint32, C.c_char_p, P(LpmIpKeySt)]),
    "infw_make_rule": (C.c_int, [P(RulesValSt), C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint8, C.c_uint8,
                                 C.c_char_p]),
    "infw_table_info": (C.c_int, [C.c_void_p, P(TableInfo)]),
    "infw_debug_walk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "infw_set_launch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "infw_get_launch": (C.c_int, [C.c_void_p, P(C.c_int), P(C.c_int), P(C.c_int)]),
    "infw_debug_lookup_set": (C.c_int, [C.c_void_p, C.c_uint32]),
    "infw_debug_keys_read": (C.c_int, [C.c_void_p, P(LpmIpKeySt), C.c_uint32, P(C.c_uint32)]),
    "infw_debug_keys_clear": (C.c_int, [C.c_void_p]),
    "infw_last_error": (C.c_char_p, []),
    "infw_abi_version": (C.c_int, []),
    "infw_build_id": (C.c_char_p, []),
    "infw_table_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_uint64)]),
    "infw_table_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "infw_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "infw_get_option": (C.c_int, [C.c_void_p, C.c_char_p, P(C.c_int64)]),
    "infw_option_name": (C.c_char_p, [C.c_int]),
    "infw_classify_variant": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_char_p, C.c_size_t]),
    "infw_kernel_variant_name": (C.c_char_p, [C.c_int]),
    "infw_launch_counts": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "infw_xdp_host_events": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_uint64, C.POINTER(C.c_uint64)]),
    "infw_classify_bursts_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint64]),
    "infw_pack_burst_host": (C.c_int, [C.c_void_p, C.c_void_p]),
    "infw_burst_host_events": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "infw_classify_xdp": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "infw_classify_xdp_mb": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "infw_classify_xdp_mb_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                          C.c_void_p, C.c_void_p, P(ClassifyEx), C.c_void_p]),
    "infw_events_capture_xdp": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                          C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "infw_classify_xdp_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint64]),
    "infw_pack_xdp_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, P(BatchSoaC)]),
    "infw_classify_xdp_rings": (C.c_int, [C.c_void_p, C.c_int, P(XdpRing), C.c_uint32, C.c_void_p]),
    "infw_classify_xdp_rings_ex": (C.c_int, [C.c_void_p, C.c_int, P(XdpRing), C.c_uint32, P(XdpRingsEx), C.c_void_p]),
    "infw_events_capture_xdp_rings": (C.c_int, [C.c_void_p, C.c_int, P(XdpRing), C.c_uint32, C.c_void_p, C.c_uint64,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "infw_events_decode": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "infw_events_decode_host": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "infw_events_sort": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "infw_classify_xdp_rings_split": (C.c_int, [C.c_void_p, C.c_int, P(XdpRing), P(XdpRingSplit), C.c_uint32,
                                                C.c_void_p, C.c_void_p]),
}
for _name, (_res, _args) in _sig.items():
    _f = getattr(lib, _name)
    _f.restype = _res
    _f.argtypes = _args


def last_error() -> str:
    return (lib.infw_last_error() or b"").decode(errors="replace")


class InfwError(OSError):
    pass


def check(rc: int, what: str) -> int:
    if rc < 0:
        raise InfwError(-rc, f"{what}: {os.strerror(-rc)} ({last_error()})")
    return rc


# ---------------------------------------------------------------- workload lib
class GenPrefix(C.Structure):
    _fields_ = [("addr", C.c_uint8 * 16), ("ifindex", C.c_uint32), ("plen", C.c_uint8),
                ("family", C.c_uint8), ("pad", C.c_uint8 * 2)]


class GenParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("prefixes", C.c_void_p), ("zipf_cdf", C.c_void_p),
                ("n_prefixes", C.c_uint32), ("hit_permille", C.c_uint32), ("v6_permille", C.c_uint32),
                ("cross_permille", C.c_uint32), ("p_tcp", C.c_uint32), ("p_udp", C.c_uint32),
                ("p_icmp", C.c_uint32), ("p_sctp", C.c_uint32), ("p_special", C.c_uint32),
                ("n_special", C.c_uint32), ("special_ports", C.c_uint16 * 16), ("n_icmp", C.c_uint32),
                ("icmp_tc", C.c_uint16 * 16), ("len_min", C.c_uint32), ("len_max", C.c_uint32),
                ("p_nonip", C.c_uint32), ("p_trunc", C.c_uint32), ("n_ifindex", C.c_uint32),
                ("ifindexes", C.c_uint32 * 8)]


wl = _load(WL_LIB_PATH)
_wsig = {
    "infw_wl_create": (C.c_int, [P(C.c_void_p), C.c_int, C.c_uint64, C.c_uint32, C.c_uint32]),
    "infw_wl_destroy": (None, [C.c_void_p]),
    "infw_wl_line_rates": (C.c_int, [C.c_int, P(C.c_double)]),
    "infw_wl_n_entries": (C.c_uint64, [C.c_void_p]),
    "infw_wl_keys": (C.c_void_p, [C.c_void_p]),
    "infw_wl_val_index": (C.c_void_p, [C.c_void_p]),
    "infw_wl_n_templates": (C.c_uint32, [C.c_void_p]),
    "infw_wl_templates": (C.c_void_p, [C.c_void_p]),
    "infw_wl_params": (P(GenParams), [C.c_void_p]),
    "infw_wl_set_packet_seed": (None, [C.c_void_p, C.c_uint64]),
    "infw_wl_uniform_sources": (None, [C.c_void_p]),
    "infw_wl_frames": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_int]),
    "infw_wl_tuples": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int]),
    "infw_wl_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "infw_wl_upload": (C.c_int, [C.c_void_p, C.c_int]),
    "infw_wl_gen_soa": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "infw_wl_gen_frames": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
}
for _name, (_res, _args) in _wsig.items():
    _f = getattr(wl, _name)
    _f.restype = _res
    _f.argtypes = _args

assert C.sizeof(EventHdrSt) == 8 and C.sizeof(EventRec) == 24 and C.sizeof(XdpRing) == 48
assert C.sizeof(XdpRingSplit) == 16 and C.sizeof(EventDecoded) == 64
if lib.infw_abi_version() != ABI_VERSION:
    raise ImportError(f"{LIB_PATH}: ABI {lib.infw_abi_version()}, these bindings are ABI {ABI_VERSION}: rebuild (make)")


def option_names() -> list:
    """Every per-context option the library knows (infw_option_name)."""
    out, i = [], 0
    while (n := lib.infw_option_name(i)) is not None:
        out.append(n.decode())
        i += 1
    return out


def kernel_variants() -> list:
    """The registry of every kernel instantiation the library launches (infw_kernel_variant_name)."""
    out, i = [], 0
    while (n := lib.infw_kernel_variant_name(i)) is not None:
        out.append(n.decode())
        i += 1
    return out


def build_id() -> str:
    """infw_build_id(): hash of the kernel / table-layout sources and flags this library was built from."""
    return lib.infw_build_id().decode()
