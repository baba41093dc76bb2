"""Deny events of a multi-buffer AF_XDP ring (infw_classify_xdp_mb_ex) and their perf samples gathered across each
chain's buffers (infw_events_capture_xdp), bit for bit against the CPU oracle's records (pkt_index mapped to the head's
ring index) and samples built here from the umem.  The umem is random non-zero bytes, fragments start at every byte
alignment, and heads that must be denied are candidates the oracle denies at that linear length.  The 90-descriptor
chain is a 60-byte head (no rule can deny a 3-byte head) and 89 x 3 bytes: 249 bytes after the first 64 descriptors."""
import numpy as np
import pytest
import torch

import infw
from infw import _native as N
from infw import workloads as W

from parity import oracle_for

pytestmark = pytest.mark.gpu
T, CONTD, STRIDE, SB = infw.XDP_CHAIN_TILE, infw.XDP_PKT_CONTD, 2048, N.EVENT_SAMPLE_BYTES
FRAGS = [(255, 1), (256, 40), (100, 0, 200), (60, 17), (60,) + (3,) * 89] + [(0,)] * 40 + [(100, 50)]  # (0,): uncut


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    wl = W.Workload(W.CFG2_MIXED_1M, n_prefixes=20000, n_templates=64)
    clf = infw.Classifier(devices=[0], max_entries=wl.n_entries + 16)
    wl.load_into(clf)
    clf.commit()
    return wl, oracle_for(wl), clf


def _ring(wl, m, shape):
    """umem, descriptors, ifindex, the oracle's records as the device writes them and the expected samples."""
    rng = np.random.default_rng(11)
    chains, left = {"frags": FRAGS, "singles": [(0,)] * (2 * T + 19), "mixed": []}[shape], 3 * T + 77
    while shape == "mixed" and left:  # per frame the descriptor lens, the head's first (0: the frame's own length)
        k = min(int(rng.integers(1, 4)), left)
        chains.append(((0,) if k == 1 else (int(rng.choice([9, 30, 60, 100, 200])),)) + tuple(rng.integers(1, 301, k - 1)))
        left -= k
    hdr, _, pl, ifx = wl.frames(4242, 4096)
    ring_if = int(np.bincount(ifx).argmax())
    ifs = lambda k: np.full(k, ring_if, np.uint32)
    denied, pick = {}, []
    for f, ch in enumerate(chains):  # every other frame, and every frags chain: a candidate denied at that length
        L = ch[0]
        if L not in denied:
            denied[L] = m.collect_events(hdr, np.full(4096, L, np.uint32) if L else pl, pl, ifs(4096))[:, 0].tolist()
        c = next((c for c in denied[L] if c not in pick), None) if f % 2 == 0 or shape == "frags" else None
        pick.append(next(c for c in range(4096) if c not in pick) if c is None else c)
    ln = np.concatenate([np.array((int(pl[c]),) + ch[1:] if ch[0] == 0 else ch) for c, ch in zip(pick, chains)])
    n, klen = ln.size, np.array([len(ch) for ch in chains])
    starts = np.cumsum(klen) - klen
    opt = np.full(n, CONTD, np.uint32)
    opt[starts[1:] - 1] = 0
    opt[-1] = CONTD if shape == "frags" else 0  # frags: the last chain is left open at n - 1
    base = rng.permutation(n + 8)[:n].astype(np.uint64) * np.uint64(STRIDE) + rng.integers(0, 8, n).astype(np.uint64)
    off = (rng.integers(0, 100, n) | 1).astype(np.uint64)
    at = (base + off).astype(np.int64)
    umem = rng.integers(1, 256, (n + 9) * STRIDE, dtype=np.uint8)
    umem[at[starts][:, None] + np.arange(80)] = hdr[pick]
    desc = np.zeros((n, 4), np.uint32)
    desc[:, :2] = (base | off << np.uint64(48)).view(np.uint32).reshape(n, 2)
    desc[:, 2], desc[:, 3] = ln, opt
    total = np.add.reduceat(ln.astype(np.uint64), starts).astype(np.uint32)
    ev = m.collect_events(hdr[pick], ln[starts], total, ifs(len(chains)))
    assert ev.shape[0] >= (32 if shape == "mixed" else 1) and (shape != "frags" or ev.shape[0] == len(chains))
    rec = np.stack([ev[:, 1] | ev[:, 2] << 16 | ev[:, 3] << 32 | ev[:, 4] << 48, ev[:, 5],
                    starts[ev[:, 0].astype(int)].astype(np.uint64)], axis=1)
    smp = np.zeros((rec.shape[0], SB), np.uint8)
    for k, (f, cap) in enumerate(zip(ev[:, 0].astype(int), ev[:, 5].astype(int))):
        js = range(starts[f], starts[f] + klen[f])
        smp[k, :4] = np.frombuffer(np.uint32(((8 + cap + 4 + 7) & ~7) - 4).tobytes(), np.uint8)
        smp[k, 4:12] = np.frombuffer(rec[k, 0].tobytes(), np.uint8)
        smp[k, 12:12 + cap] = np.concatenate([umem[at[j]:at[j] + ln[j]] for j in js])[:cap]
    return umem, desc, ring_if, rec, smp, at


@pytest.mark.parametrize("shape,where,pre,div", [("mixed", "hbm", 0, 1), ("mixed", "host", 0, 1), ("frags", "hbm", 0, 1),
                                                 ("singles", "hbm", 0, 1), ("mixed", "hbm", 5, 1), ("mixed", "hbm", 5, 2)])
def test_xdp_mb_events_and_samples(env, shape, where, pre, div):
    # pre: sentinel records (pkt_index 2^40) already in the buffer; div 2: a capacity of pre + k // 2 records
    wl, m, clf = env
    umem, desc, ring_if, rec, want, at = _ring(wl, m, shape)  # asserts the guards before the device is touched
    n, k, cap = desc.shape[0], rec.shape[0], pre + rec.shape[0] // div
    tu, td = torch.from_numpy(umem), torch.from_numpy(desc.view(np.int32))
    tu, td = (tu.to("cuda:0"), td.to("cuda:0")) if where == "hbm" else (tu.pin_memory(), td.pin_memory())
    sent = np.array([[0x0001_0001_0007_0003 + s, 40, 1 << 40] for s in range(pre)], np.uint64).reshape(-1, 3)
    ev = torch.full(((n + 5) * 24,), 0xEE, dtype=torch.uint8, device="cuda:0")
    ev[:pre * 24] = torch.from_numpy(sent.view(np.uint8).reshape(-1))
    cnt = torch.full((1,), pre, dtype=torch.int64, device="cuda:0")
    smp = torch.full(((n + 5) * SB,), 0xEE, dtype=torch.uint8, device="cuda:0")
    outs = []
    for kw in ({}, dict(events=ev[:cap * 24], events_count=cnt)):  # the plain call, then the same ring with events
        res = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        ver = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
        clf.stats_reset()
        clf.classify_xdp_mb(tu, td, n, ring_if, results=res, verdicts=ver, **kw)
        torch.cuda.synchronize()
        outs.append((res.cpu().numpy(), ver.cpu().numpy(), clf.stats_read_all()))
    clf.events_capture_xdp(tu, td, n, ev[:cap * 24], cnt, smp)
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(*outs)) and int(cnt.item()) == pre + k
    grec, gs = ev.cpu().numpy().view(np.uint64).reshape(-1, 3), smp.cpu().numpy().reshape(-1, SB)
    assert np.array_equal(grec[:pre], sent) and (ev[cap * 24:] == 0xEE).all() and (gs[cap:] == 0xEE).all()
    for s in range(pre):  # a record of another batch: size and header, no frame bytes
        assert bytes(gs[s]) == bytes([52, 0, 0, 0]) + sent[s, 0].tobytes() + bytes(SB - 12)
    order = np.argsort(grec[pre:cap, 2], kind="stable")
    landed = np.isin(rec[:, 2], grec[pre:cap, 2])  # every record when the capacity allows, else distinct ones of them
    assert landed.sum() == cap - pre and np.array_equal(grec[pre:cap][order], rec[landed])
    assert np.array_equal(gs[pre:cap][order], want[landed])
    if shape == "singles":  # the existing kernel over the same frames as an infw_frame_batch
        old = torch.full(((n + 5) * SB,), 0xEE, dtype=torch.uint8, device="cuda:0")
        lens = torch.from_numpy(desc[:, 2].astype(np.int32)).to("cuda:0")  # ifindex is not read by the capture
        clf.events_capture(tu, lens, lens, n, ev[:cap * 24], cnt, old, offsets=torch.from_numpy(at).to("cuda:0"))
        assert torch.equal(old, smp)
