"""infw_events_decode / infw_events_decode_host: perf samples -> 64-B decoded records, against the consumer in
infw/events.py (decode_sample + gopacket_layers, the specification): format_records over the records must give the
lines and log lines drain gives over the samples, and the host and device records must be the same bytes."""
import ctypes as C
import struct

import numpy as np
import pytest

import goenc
import infw
from frames import frame
from infw import _native as N
from infw import events as E

SB, DB = N.EVENT_SAMPLE_BYTES, 64
NAMES = {1: "eth0", 2: "bond0"}.get  # ifindex 3 is unknown: the lookup error


def slot(pkt, ifid=1, pkt_len=None, size=None):
    """The 272-B slot of a frame: size word, event_hdr_st, the first 256 bytes, zeros (infw_events_capture's layout)."""
    cap = bytes(pkt[:256])
    size = ((8 + len(cap) + 4 + 7) & ~7) - 4 if size is None else size
    pkt_len = len(pkt) if pkt_len is None else pkt_len
    return (struct.pack("<IHHBBH", size, ifid, 7, 1, 0, pkt_len & 0xFFFF) + cap).ljust(SB, b"\0")


def edit(f, at, new):
    b = bytearray(f)
    b[at:at + len(new)] = new
    return bytes(b)


def ip4(proto, payload, total=None, src="10.0.0.1"):
    """Ethernet + a 20-B IPv4 header (total length: the real one unless given) + payload."""
    h = frame(src, "10.0.0.2", proto=proto)[:34]
    return edit(h, 16, struct.pack("!H", 20 + len(payload) if total is None else total)) + payload


TCP4 = frame("10.1.1.1", "192.0.2.4", "tcp", dport=80, sport=1234)
TCP4_IHL6 = edit(frame("10.1.1.1", "192.0.2.4", "tcp", dport=80, ihl=6), 16, struct.pack("!H", 44))
UDP6 = frame("2001:db8::5", "2001:db8::6", "udp", dport=53, sport=5353)
ICMP4 = frame("10.1.2.5", "192.0.2.1", "icmp", icmp_type=8, icmp_code=3)
ICMP6 = frame("2001:db8:0:0:1::5", "2001:db8::1", "icmpv6", icmp_type=128, icmp_code=0)
RNG = np.random.default_rng(7).integers(0, 256, SB, dtype=np.uint8).tobytes()
CASES = [
    # the six known answers of test_events_cpu.py::test_decode_known_answers
    ("tcp4", slot(frame("10.1.2.3", "192.0.2.9", "tcp", dport=80, sport=1234))),
    ("udp4", slot(frame("10.1.2.4", "198.51.100.7", "udp", dport=53, sport=5353))),
    ("icmp4-8B", slot(ICMP4)),
    ("sctp4", slot(frame("10.1.2.6", "192.0.2.1", "sctp", dport=3868, sport=2905), ifid=2)),
    ("icmp6", slot(ICMP6, ifid=2)),
    ("tcp6-mapped-dst", slot(frame("2001:db8::7", "::ffff:192.0.2.1", "tcp", dport=443, sport=50000), ifid=2)),
    ("fragment", slot(edit(TCP4, 20, b"\x20\x00"))),
    ("frag-offset", slot(edit(TCP4, 20, b"\x00\x09"))),
    ("total-24", slot(edit(TCP4, 16, struct.pack("!H", 24)))),
    ("total-0-tso", slot(edit(TCP4, 16, b"\0\0"))),
    ("ip4-short", slot(TCP4[:14 + 19])),
    ("ihl6-option", slot(edit(TCP4_IHL6, 34, b"\x94\x04\x00\x00"))),
    ("ihl6-nop-eol", slot(edit(TCP4_IHL6, 34, b"\x01\x00\x07\x01"))),
    ("ihl6-optlen-1", slot(edit(TCP4_IHL6, 34, b"\x94\x01\x00\x00"))),
    ("ihl4", slot(edit(TCP4, 14, b"\x44"))),
    ("total-cuts-tcp", slot(edit(TCP4, 16, struct.pack("!H", 39)))),
    ("ip4-in-ip4", slot(ip4(4, frame("10.5.5.5", "10.6.6.6", "udp", dport=99)[14:]))),
    ("ip4-ip6-udp", slot(ip4(41, UDP6[14:]))),
    ("ip6-in-ip6-short", slot(edit(UDP6, 20, b"\x29"))),
    ("nest-13", slot(frame("10.0.0.1")[:14] + ip4(4, b"", total=0, src="10.9.0.1")[14:] * 11
                     + ip4(41, b"\x60\x00", total=0)[14:])),
    ("ip6-nh-0", slot(edit(UDP6, 20, b"\0"))),
    ("ip6-plen-0", slot(edit(UDP6, 18, b"\0\0"))),
    ("ip6-short", slot(UDP6[:14 + 39])),
    ("icmp4-7B", slot(ICMP4[:41])),
    ("icmp6-3B", slot(ICMP6[:14 + 40 + 3])),
    ("icmp6-4B", slot(ICMP6[:14 + 40 + 4])),
    ("udp-7B", slot(frame("10.1.2.4", "198.51.100.7", "udp", dport=53)[:14 + 20 + 7])),
    ("frame-13", slot(TCP4[:13])),
    ("frame-14", slot(TCP4[:14])),
    ("arp", slot(frame("10.1.1.1", ethertype=0x0806))),
    ("unknown-if", slot(TCP4, ifid=3)),
    ("len-258", slot(frame("10.9.9.9", "192.0.2.2", "tcp", dport=22, length=258))),
    ("len-300-short", slot(frame("10.9.9.8", "192.0.2.2", "tcp", dport=22, length=300))),
    ("captured-0-eof", slot(b"", pkt_len=5, size=8)),
    ("size-4-badhdr", slot(TCP4, size=4)),
    ("random-size-max", b"\xff\xff\xff\xff" + RNG[4:]),
    ("random-ip4-260", b"\xff\xff\xff\xff" + edit(RNG[4:], 6, struct.pack("<H", 260) + RNG[12:24] + b"\x08\x00\x45")),
    ("random-ip6-260", b"\xff\xff\xff\xff" + edit(RNG[4:], 6, struct.pack("<H", 260) + RNG[12:24] + b"\x86\xdd")),
]
TABLE = np.frombuffer(b"".join(s for _, s in CASES), np.uint8).reshape(-1, SB).copy()


@pytest.fixture(scope="module")
def clf():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return infw.Classifier(devices=[0])


def on_device(clf, samples, count, cap, fill=None):
    """events_decode over host samples: the decoded tensor (prefilled with `fill`) copied back."""
    import torch
    dev = torch.device("cuda", 0)
    smp = torch.from_numpy(np.ascontiguousarray(samples)).to(dev)
    cnt = torch.tensor([count], dtype=torch.int64, device=dev)
    out = None if fill is None else torch.full((cap, DB), fill, dtype=torch.uint8, device=dev)
    got = clf.events_decode(smp, cnt, cap, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("impl", ["host", pytest.param("device", marks=pytest.mark.gpu)])
def test_decode_matches_consumer(impl, request):
    n = len(CASES)
    host = infw.events_decode_host(TABLE)
    got = host if impl == "host" else on_device(request.getfixturevalue("clf"), TABLE, n, n)
    want = E.drain(TABLE, n, NAMES)
    assert len(want[0]) > 2 * n and len(want[1]) >= 5  # the table reaches the lines and every kind of log line
    for (name, _), rec, s in zip(CASES, got, TABLE):
        assert E.format_records(rec, 1, NAMES) == E.drain(s[None], 1, NAMES), name
    assert E.format_records(got, n, NAMES) == want
    assert E.format_records(got[:5], n, NAMES) == E.drain(TABLE[:5], n, NAMES)  # a 5-slot ring: the lost-samples line
    assert got.tobytes() == host.tobytes()
    rec = got.view(E.DECODED)[:, 0]
    bad = (rec["layers"] & (E.EVL_SHORT | E.EVL_BADHDR)) != 0
    assert bad.sum() >= 4 and not (rec["layers"][bad] & 0xFFFF).any() and not rec["pad"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("n,cap,count", [(1, 1, 1), (63, 64, 63), (65, 128, 65), (129, 129, 400), (257, 300, 257)])
def test_decode_counts(clf, n, cap, count):
    """Whole waves, tail waves and more than one trip; nothing at or past min(count, cap) is written."""
    samples = np.resize(TABLE, (cap, SB))  # the table repeated
    got = on_device(clf, samples, count, cap, fill=0xAB)
    k = min(count, cap)
    assert k == n and got[:k].tobytes() == infw.events_decode_host(samples[:k]).tobytes()
    assert (got[k:] == 0xAB).all()


@pytest.mark.gpu
def test_classify_capture_decode_format(clf):
    """Deny table -> classify_frames with events -> events_capture -> events_decode -> format_records, against drain
    over the captured samples copied back."""
    import torch
    dev = torch.device("cuda", 0)
    deny = goenc.raw_value([{"slot": 1, "ruleId": 7, "protocol": 0, "dstPortStart": 0, "dstPortEnd": 0,
                             "icmpType": 0, "icmpCode": 0, "action": 1}])
    for ifx, cidr in ((1, "10.0.0.0/8"), (2, "10.0.0.0/8"), (2, "2001:db8::/32")):
        clf.update(infw.LpmIpKeySt.from_buffer_copy(goenc.build_key(ifx, cidr)), infw.RulesValSt.from_buffer_copy(deny))
    clf.commit()
    n, stride = 204, 128
    buf = np.zeros((n, stride), np.uint8)
    lens = np.zeros(n, np.uint32)
    for i in range(n):  # the six known-answer frames, over and over
        s = CASES[i % 6][1]
        lens[i] = struct.unpack_from("<H", s, 10)[0]
        buf[i, :lens[i]] = np.frombuffer(s[12:12 + lens[i]], np.uint8)
    t = lambda a: torch.from_numpy(a.view(np.int32)).to(dev)  # noqa: E731
    dbuf, dl, di = torch.from_numpy(buf).to(dev), t(lens), t(np.tile(np.array([1, 1, 1, 2, 2, 2], np.uint32), n // 6))
    ev = torch.zeros(n * C.sizeof(N.EventRec), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    smp = torch.zeros(n * SB, dtype=torch.uint8, device=dev)
    clf.classify_frames(dbuf, dl, di, n, stride=stride, events=ev, events_count=cnt)
    clf.events_capture(dbuf, dl, di, n, ev, cnt, smp, stride=stride)
    dec = clf.events_decode(smp, cnt, n)
    torch.cuda.synchronize()
    assert int(cnt.item()) == n
    want = E.drain(smp.cpu().numpy(), n, NAMES)
    assert E.format_records(dec.cpu().numpy(), n, NAMES) == want and len(want[0]) == 3 * n and want[1] == []


def test_arguments_host():
    assert C.sizeof(N.EventDecoded) == 64 and {"infw_events_decode", "infw_events_decode_host"} <= set(N.ABI_SYMBOLS)
    buf = (C.c_uint8 * 512)()
    a = C.addressof(buf)
    c = infw.Classifier(flags=infw.F_HOST_ONLY)
    assert N.lib.infw_events_decode(c._ctx, 0, a, 1, a + 288, a + 320, None) == -19  # ENODEV: host-only context
    assert N.lib.infw_events_decode_host(None, 1, a) == N.lib.infw_events_decode_host(a, 1, None) == -22
    assert N.lib.infw_events_decode_host(None, 0, None) == 0 and infw.events_decode_host(TABLE[:0]).shape == (0, 64)
    assert infw.events_decode_host(np.frombuffer(b"\0" + TABLE.tobytes(), np.uint8)[1:]).tobytes() == \
        infw.events_decode_host(TABLE).tobytes()  # no alignment asked of the host form


@pytest.mark.gpu
def test_arguments_device(clf):
    import torch
    mem = torch.zeros(1024, dtype=torch.uint8, device="cuda:0")
    a = mem.data_ptr()
    call = lambda s, cap, cnt, d: N.lib.infw_events_decode(clf._ctx, 0, s, cap, cnt, d, None)  # noqa: E731
    assert call(None, 1, a + 512, a + 640) == call(a, 1, None, a + 640) == call(a, 1, a + 512, None) == -22
    assert call(a + 4, 1, a + 512, a + 640) == call(a, 1, a + 512, a + 648) == -22  # samples 8-B, decoded 16-B aligned
    assert call(None, 0, None, None) == 0 and call(a, 0, a + 512, a + 640) == 0
    torch.cuda.synchronize()
    assert not mem.cpu().numpy().any()
