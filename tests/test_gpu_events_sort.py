"""infw_events_sort: deny-event records into packet order on the device.  Synthetic records against numpy's stable
argsort of the clamped key, byte for byte, around the wave and tile sizes and for every pass count and key width; then
classify -> sort -> capture (-> decode) against the oracle's packet-order events and the host builders, no host sort."""
import numpy as np
import pytest
import torch

import goenc
import infw
import orc
from frames import frame
from infw import _native as N

pytestmark = pytest.mark.gpu
T, SB, CANARY = 2048, N.EVENT_SAMPLE_BYTES, 0xC5C5C5C5C5C5C5C5  # T: evsort.hip's tile
BOUNDS = [200, 70_000, (1 << 24) + 5, (1 << 32) + 9, 0]  # 1 pass, 3 (odd), 4, 5 with the wide key, 8 over 64 bits
DENY = [(1, "10.0.0.0/8"), (2, "10.0.0.0/8"), (2, "2001:db8::/32")]


@pytest.fixture(scope="module")
def clf():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    c = infw.Classifier(devices=[0])
    val = goenc.raw_value([{"slot": 1, "ruleId": 7, "protocol": 0, "dstPortStart": 0, "dstPortEnd": 0, "icmpType": 0,
                            "icmpCode": 0, "action": 1}])
    m = orc.OracleMap(max_entries=64)
    for ifx, cidr in DENY:
        key = goenc.build_key(ifx, cidr)
        c.update(infw.LpmIpKeySt.from_buffer_copy(key), infw.RulesValSt.from_buffer_copy(val))
        assert m.update(key, val) == 0
    c.commit()
    c.oracle = m
    return c


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("cap,count", [(m + 40, m) for m in (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)] +
                         [(T + 100, T + 1100)])  # the last: records were lost, the kept ones are sorted
def test_sort_synthetic(clf, cap, count, bound):
    m = min(count, cap)
    rng = np.random.default_rng(1000 * m + bound % 997)
    key = rng.integers(0, bound or 1 << 64, m, dtype=np.uint64)  # bound 0: all 64 bits, the top byte too
    dup, far = rng.random(m) < 1 / 8, rng.random(m) < 1 / 8
    key[dup] = key[rng.integers(0, max(m, 1), int(dup.sum()))]
    if bound:  # records of another batch: they sort last, in their original order
        key[far] = np.uint64(bound) + rng.integers(0, 1 << 40, int(far.sum()), dtype=np.uint64)
    rec = np.full((cap + 8, 3), CANARY, np.uint64)
    slot = np.arange(m, dtype=np.uint64)
    rec[:m, 0] = slot << np.uint64(16) | np.uint64(0x0040_0001_0000_0002)  # hdr: a ruleId per slot
    rec[:m, 1] = slot + np.uint64(1) | np.uint64(9 << 32)                  # captured per slot, `reserved` set
    rec[:m, 2] = key
    want = rec[:m][np.argsort(np.minimum(key, np.uint64(bound)) if bound else key, kind="stable")]
    assert m < 256 or ((bound == 0) == bool((key >> np.uint64(56)).any()) and (far.any() or not bound))
    ev = torch.from_numpy(rec.view(np.int64)).to("cuda:0")
    cnt = torch.tensor([count], dtype=torch.int64, device="cuda:0")
    clf.events_sort(ev.view(torch.uint8).reshape(-1)[:cap * 24], cnt, cap, bound)
    torch.cuda.synchronize()
    got = ev.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:m], want) and (got[m:] == CANARY).all() and int(cnt.item()) == count


@pytest.mark.parametrize("path", ["frames", "rings"])
def test_classify_sort_capture(clf, path):
    n, stride, sizes = 600, 160, (250, 0, 350)
    ring_if, first = (1, 2, 2), [0, 250, 250, 600]
    ifx = np.repeat(np.array(ring_if, np.uint32), sizes)
    buf, lens = np.zeros((n, stride), np.uint8), 60 + np.arange(n, dtype=np.uint32) % 90
    for i in range(n):  # two frames of three are denied: 10/8 on either interface
        f = frame(f"{10 if i * 7 % 3 else 11}.{i >> 8}.{i & 255}.9", "192.0.2.1", "tcp", dport=80, length=int(lens[i]))
        buf[i, :lens[i]] = np.frombuffer(f, np.uint8)
    orec, osmp = clf.oracle.collect_event_samples(buf.reshape(-1), np.arange(n) * stride, lens, lens, ifx)
    k = orec.shape[0]
    assert 300 <= k < n  # events_cap = n: nothing is lost
    want = np.stack([orec[:, 1] | orec[:, 2] << 16 | orec[:, 3] << 32 | orec[:, 4] << 48, orec[:, 5], orec[:, 0]], axis=1)
    dev = lambda a: torch.from_numpy(a.view(np.int32)).to("cuda:0")  # noqa: E731
    dbuf, dl = torch.from_numpy(buf).to("cuda:0"), dev(lens)
    ev, cnt = torch.zeros(n * 24, dtype=torch.uint8, device="cuda:0"), torch.zeros(1, dtype=torch.int64, device="cuda:0")
    smp = torch.zeros(n * SB, dtype=torch.uint8, device="cuda:0")
    if path == "frames":
        clf.classify_frames(dbuf, dl, dev(ifx), n, stride=stride, events=ev, events_count=cnt)
        clf.events_sort(ev, cnt, n, n)
        clf.events_capture(dbuf, dl, dev(ifx), n, ev, cnt, smp, stride=stride)
        dec = clf.events_decode(smp, cnt, n)
        torch.cuda.synchronize()
        assert dec.cpu().numpy()[:k].tobytes() == infw.events_decode_host(osmp).tobytes()
    else:
        desc = np.zeros((n, 4), np.uint32)
        desc[:, 0], desc[:, 2] = np.arange(n) * stride, lens
        td, res = dev(desc), torch.zeros(n, dtype=torch.int32, device="cuda:0")
        rings = [(dbuf, td[a:b], b - a, q, res[a:b], None) for a, b, q in zip(first, first[1:], ring_if)]
        clf.classify_xdp_rings(rings, events=ev, events_count=cnt)
        clf.events_sort(ev, cnt, n, n)  # index_bound: the rings' flat total
        clf.events_capture_xdp_rings(rings, ev, cnt, smp)
        torch.cuda.synchronize()
        hres = res.cpu().numpy().view(np.uint32)
        host = [infw.xdp_host_events(buf.reshape(-1), desc[a:b], q, hres[a:b], b - a)
                for a, b, q in zip(first, first[1:], ring_if)]
        osmp = np.concatenate([s[:c] for s, c in host])  # the host builder's samples, ring after ring
    assert int(cnt.item()) == k
    assert np.array_equal(ev.cpu().numpy().view(np.uint64).reshape(-1, 3)[:k], want)
    assert smp.cpu().numpy().reshape(-1, SB)[:k].tobytes() == osmp.tobytes()
