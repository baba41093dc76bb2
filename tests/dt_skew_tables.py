"""Hand-built rule lists for the decision lines' cut codes (csrc/infw_tables.h infw_dt_cut), shared by
test_dt_skew_cpu.py and test_gpu_dt_skew.py.

Every list sits on one IPv4 /24 and one IPv6 /48 of interface IFX.  Per list the (TCP, UDP) cut codes the compiler
must choose -- the cut of the fewest lines whose every line holds <= 20 segments, the uniform one on a tie:
  a   TCP: 12 exact ports below 1024 (25 segments there) and 4 ranges above 4096.  No uniform cut fits -- its part 0
      is [0, 4096) at best -- and of the skewed ones only 512-value low lines do: code 7, 12 lines.
  b   TCP: 30 exact ports, one every 2048 values (61 segments: 31 per half, 16 per quarter): the uniform code 2,
      whatever the skewed codes offer; UDP: shape a again, in the same list.
  c   TCP: 3 rules, one line: code 0.  It also carries the SCTP, ICMP and ICMPv6 rules of the set.
  d   TCP: 25 exact ports below 4096 and nothing above: 51 segments in a uniform cut's part 0, 13 per 1024-value
      line of code 6 (8 lines), a constant high side.
Shape d alone makes the image's regions 16 lines (choose_dt_plog2), which the skewed codes need.
"""
import numpy as np

import goenc
from frames import frame, snapshots
from infw import workloads as W

IFX = 9
LOW12 = [22, 53, 80, 110, 143, 179, 389, 443, 515, 636, 873, 993]           # shape a: every 512-value line <= 13 segments
HIGH4 = [(5000, 5010), (20000, 20100), (40000, 40001), (60000, 65535)]      # [start, end): above 4096
EVEN30 = [1000 + 2048 * i for i in range(30)]                                # shape b
LOW25 = [40 + 160 * i for i in range(25)]                                    # shape d: 40 .. 3880
FEW3 = [(80, 0), (8000, 8100), (443, 0)]                                     # shape c

EXPECT = {"a": (7, 0), "b": (2, 7), "c": (0, 0), "d": (6, 0)}                # list -> (TCP code, UDP code)
EXPECT_UNIFORM = {"a": (4, 0), "b": (2, 4), "c": (0, 0), "d": (4, 0)}        # dt_adapt = 2


def _rules(spec):
    """spec: (protocol, start, end) in scan order -> rules in slots 1.. with ruleId = slot, Allow / Deny alternating."""
    icmp = (1, 58)  # for these (protocol, type, code)
    return [{"slot": i + 1, "ruleId": i + 1, "protocol": p, "dstPortStart": 0 if p in icmp else s,
             "dstPortEnd": 0 if p in icmp else e, "icmpType": s if p in icmp else 0, "icmpCode": e if p in icmp else 0,
             "action": 1 + (i & 1)} for i, (p, s, e) in enumerate(spec)]


def _shape_a(proto):
    return [(proto, p, 0) for p in LOW12] + [(proto, s, e) for s, e in HIGH4]


SPECS = {
    "a": _shape_a(6),
    "b": [(6, p, 0) for p in EVEN30] + _shape_a(17),
    "c": [(6, s, e) for s, e in FEW3] + [(132, 3000, 3900), (1, 8, 0), (58, 128, 0)],
    "d": [(6, p, 0) for p in LOW25],
}
# (one IPv6 /32 group each: a group of more than 3 prefixes would overflow and take the epoch off the lean kernels)
NETS = {"a": ("10.1.1.0/24", "2001:db1:1::/48"), "b": ("10.1.2.0/24", "2001:db2:2::/48"),
        "c": ("10.1.3.0/24", "2001:db3:3::/48"), "d": ("10.1.4.0/24", "2001:db4:4::/48")}
SRC = {k: (v4.replace("0/24", "7"), v6.replace("/48", "5")) for k, (v4, v6) in NETS.items()}


def entries(names="abcd"):
    """(key bytes, value bytes) of the lists' prefixes."""
    out = []
    for name in names:
        val = goenc.raw_value(_rules(SPECS[name]))
        out += [(goenc.build_key(IFX, net), val) for net in NETS[name]]
    return out


def probe_values(name):
    """Every cut edge of every code and every rule edge of list `name`, ascending."""
    v = {0, 65535}
    for shift in (9, 10, 11, 12, 13, 14, 15):            # line boundaries of the uniform and skewed cuts, +- 1
        v.update(x + d for x in range(1 << shift, 65536, 1 << shift) for d in (-1, 0, 1) if shift >= 12 or x <= 4096)
    for p, s, e in SPECS[name]:
        if p in (1, 58):
            s, e = s << 8 | e, 0                          # the class's value: type << 8 | code
        last = e if e else s + 1                          # [s, e), or the single port s
        v.update((s - 1, s, last - 1, last))
    return sorted(x for x in v if 0 <= x <= 65535)


def probe_frames(names="abcd", at_least=0):
    """Frames of every list's probe values x {TCP, UDP, SCTP, ICMP} x {IPv4, IPv6} (ICMP: the value as type << 8
    | code, protocol 1 on IPv4 and 58 on IPv6), repeated from the start up to at_least frames:
    (hdr, caplen, pkt_len, ifindex, tuples)."""
    fr = []
    for name in names:
        for src in SRC[name]:
            for proto in ("tcp", "udp", "sctp", "icmp"):
                if proto == "icmp" and ":" in src:
                    proto = "icmpv6"
                for x in probe_values(name):
                    fr.append(frame(src, proto=proto, dport=x, icmp_type=x >> 8, icmp_code=x & 0xFF,
                                    length=60 + x % 1400))
    while len(fr) < at_least:
        fr += fr[:at_least - len(fr)]
    hdr, cap, pl = snapshots(fr)
    ifx = np.full(len(fr), IFX, np.uint32)
    return hdr, cap, pl, ifx, W.pack_frames(hdr, cap, pl, ifx)
