"""Deny events of every ring of a poll in one call (infw_classify_xdp_rings_ex) and their perf samples, fused into the
call or by infw_events_capture_xdp_rings, bit for bit against the CPU oracle's records over the frame lists of all rings
laid end to end (pkt_index -> the head's flat index) and samples built here from each ring's umem: random non-zero
bytes, fragments at every byte alignment, `descs` slices of one tensor (a walk that leaves its ring reads the next
ring's descriptors), must-deny heads picked from what the oracle denies at that length on that ring's interface."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import infw
from infw import _native as N

from test_gpu_xdp_mb import _random_chains
from test_gpu_xdp_mb_events import env  # noqa: F401  (the 20k-prefix workload, its oracle and a classifier)

pytestmark = pytest.mark.gpu
T, CONTD, STRIDE, SB = infw.XDP_CHAIN_TILE, infw.XDP_PKT_CONTD, 2048, N.EVENT_SAMPLE_BYTES
CASES = {"boundaries": lambda rng: [1, 63, 64, 65, 0, 200, 3 * T + 77, 2],
         "max_rings": lambda rng: rng.integers(1, 4, infw.XDP_RINGS_MAX), "one_ring": lambda rng: [2 * T + 19]}
MUST = {"boundaries": [], "max_rings": [0, 15, 16, infw.XDP_RINGS_MAX - 1], "one_ring": [0]}  # rings denied at their head
PARAMS = [("boundaries", md, pre, div) for md in ("fused", "standalone") for pre, div in ((0, 1), (5, 1), (5, 2))] + \
         [(c, md, 0, 1) for c in ("max_rings", "one_ring") for md in ("fused", "standalone")]
_fill = lambda n, v, t=torch.uint8: torch.full((n,), v, dtype=t, device="cuda:0")  # noqa: E731


@functools.lru_cache(None)
def _build(wl, m, case):
    """Per ring size, ifindex and umem; the flat descriptors; the oracle's records and samples.  Asserts the guards."""
    rng = np.random.default_rng(11)
    sizes = np.asarray(CASES[case](rng), np.int64)
    hdr, _, pl, ifx = wl.frames(4242, 4096)
    ring_if = np.argsort(-np.bincount(ifx))[:4][np.arange(sizes.size) % 4].astype(np.uint32)
    n, first, ring_of = int(sizes.sum()), np.cumsum(sizes) - sizes, np.repeat(np.arange(sizes.size), sizes)
    opt = np.concatenate([_random_chains(s, rng) for s in sizes])
    ln = rng.integers(1, 301, n).astype(np.uint32)
    fixed = {}  # head -> its linear length, where it is not the picked frame's own
    if case == "boundaries":
        opt[(first + sizes - 1)[sizes > 0]] = CONTD  # every ring ends on an open chain
        a, b = first[5], first[5] + sizes[5] - 3  # ring 5: 60 + 89 x 3 bytes first; 60 + 17 + 40 left open at its end
        opt[a:a + 89], opt[a + 89], ln[a + 1:a + 90] = CONTD, 0, 3
        opt[b - 1], opt[b:b + 3], ln[b + 1:b + 3] = 0, CONTD, (17, 40)
        fixed = {int(a): 60, int(b): 60}
    head = np.r_[True, (opt[:-1] & CONTD) == 0]
    head[first[sizes > 0]] = True
    starts = np.nonzero(head)[0]
    must, denied, pick = set(fixed) | {int(first[r]) for r in MUST[case]}, {}, []
    for f, h in enumerate(starts):  # every other frame and the frames that must be: a candidate denied at that length
        q, L = ring_if[ring_of[h]], fixed.get(int(h), 0)
        if (q, L) not in denied:
            denied[q, L] = m.collect_events(hdr, np.full(4096, L, np.uint32) if L else pl, pl,
                                            np.full(4096, q, np.uint32))[:, 0].astype(int)
        pick.append(denied[q, L][f % denied[q, L].size] if f % 2 == 0 or int(h) in must else f % 4096)
        ln[h] = L or pl[pick[-1]]
    shared, at, umems, desc = case == "max_rings", np.zeros(n, np.int64), [], np.zeros((n, 4), np.uint32)
    for ix in [np.arange(n)] if shared else [np.nonzero(ring_of == r)[0] for r in range(sizes.size)]:
        k = ix.size
        base, off = (x.astype(np.uint64) for x in (rng.permutation(k + 8)[:k] * STRIDE + rng.integers(0, 8, k),
                                                   rng.integers(0, 100, k) | 1))
        umem = rng.integers(1, 256, (k + 9) * STRIDE, dtype=np.uint8)
        at[ix] = (base + off).astype(np.int64)
        hs = ix[head[ix]]
        umem[at[hs][:, None] + np.arange(80)] = hdr[np.asarray(pick)[np.searchsorted(starts, hs)]]
        addr = base + off if len(umems) % 2 == 0 else base | off << np.uint64(48)  # odd umems: unaligned mode
        desc[ix, :2] = addr.view(np.uint32).reshape(k, 2)
        umems.append(umem)
    umems = umems * sizes.size if shared else umems
    desc[:, 2], desc[:, 3] = ln, opt
    total = np.add.reduceat(ln.astype(np.uint64), starts).astype(np.uint32)
    ev = m.collect_events(hdr[pick], ln[starts], total, ring_if[ring_of[starts]])
    fr = ev[:, 0].astype(int)
    rec = np.stack([ev[:, 1] | ev[:, 2] << 16 | ev[:, 3] << 32 | ev[:, 4] << 48, ev[:, 5],
                    starts[fr].astype(np.uint64)], axis=1)
    assert must <= set(starts[fr].tolist()) and rec.shape[0] >= (32 if case == "boundaries" else 1)
    if case == "boundaries":
        assert np.unique(ring_of[starts[fr]]).size >= 4 and np.unique(ev[:, 1]).size >= 2 and total[fr][starts[fr] == b] < 256
    smp = np.zeros((rec.shape[0], SB), np.uint8)
    for k, (f, cap) in enumerate(zip(fr, ev[:, 5].astype(int))):
        u = umems[ring_of[starts[f]]]
        smp[k, :4] = np.frombuffer(np.uint32(((8 + cap + 4 + 7) & ~7) - 4).tobytes(), np.uint8)
        smp[k, 4:12] = np.frombuffer(rec[k, 0].tobytes(), np.uint8)
        js = range(starts[f], np.r_[starts, n][f + 1])
        smp[k, 12:12 + cap] = np.concatenate([u[at[j]:at[j] + ln[j]] for j in js])[:cap]
    return sizes, first, ring_if, umems, desc, rec, smp


@pytest.mark.parametrize("case,mode,pre,div", PARAMS)
def test_xdp_rings_events_and_samples(env, case, mode, pre, div):
    # pre: sentinel records (pkt_index 2^40) already in the buffer; div 2: a capacity of pre + k // 2 records
    wl, m, clf = env
    sizes, first, ring_if, umems, desc, rec, want = _build(wl, m, case)  # its guards: before the device is touched
    n, k, cap = desc.shape[0], rec.shape[0], pre + rec.shape[0] // div
    td_at = {True: (td := torch.from_numpy(desc.view(np.int32))).to("cuda:0"), False: td.pin_memory()}
    hbm = [case != "boundaries" or r % 2 == 0 for r in range(sizes.size)]  # boundaries: HBM and pinned in turn
    put = {id(u): torch.from_numpy(u).to("cuda:0") for u in umems[:1 if case == "max_rings" else None]}  # shared: one
    tu = [put[id(u)] if h else torch.from_numpy(u).pin_memory() for u, h in zip(umems, hbm)]
    sent = np.array([[0x0001_0001_0007_0003 + s, 40, 1 << 40] for s in range(pre)], np.uint64).reshape(-1, 3)
    ev, smp, cnt = _fill((n + 5) * 24, 0xEE), _fill((n + 5) * SB, 0xEE), _fill(1, pre, torch.int64)
    ev[:pre * 24] = torch.from_numpy(sent.view(np.uint8).reshape(-1))
    evs, outs = dict(events=ev[:cap * 24], events_count=cnt, **(dict(samples=smp) if mode == "fused" else {})), []
    for kw in ({}, evs):  # the plain call, then the same rings with events
        res, ver = _fill(n, -1, torch.int32), _fill(n, 7)
        rings = [(tu[r], td_at[hbm[r]][f:f + s], int(s), int(ring_if[r]), res[f:f + s], ver[f:f + s])
                 for r, (f, s) in enumerate(zip(first, sizes))]
        before = clf.launch_counts(), len(infw.kernel_variants())
        clf.stats_reset()
        clf.classify_xdp_rings(rings, **kw)
        if kw and mode == "standalone":
            clf.events_capture_xdp_rings(rings, ev[:cap * 24], cnt, smp)
        torch.cuda.synchronize()
        assert (clf.launch_counts(), len(infw.kernel_variants())) == before
        outs.append((res.cpu().numpy(), ver.cpu().numpy(), clf.stats_read_all()))
    assert all(np.array_equal(x, y) for x, y in zip(*outs)) and int(cnt.item()) == pre + k
    grec, gs = ev.cpu().numpy().view(np.uint64).reshape(-1, 3), smp.cpu().numpy().reshape(-1, SB)
    assert np.array_equal(grec[:pre], sent) and (ev[cap * 24:] == 0xEE).all() and (gs[cap:] == 0xEE).all()
    # a record of another batch: untouched by the fused call, size and header alone otherwise
    assert all(bytes(gs[s]) == (bytes([0xEE] * SB) if mode == "fused" else bytes([52, 0, 0, 0]) + sent[s, 0].tobytes() +
                                bytes(SB - 12)) for s in range(pre))
    order = np.argsort(grec[pre:cap, 2], kind="stable")
    landed = np.isin(rec[:, 2], grec[pre:cap, 2])  # every record when the capacity allows, else distinct ones of them
    assert landed.sum() == cap - pre and np.array_equal(grec[pre:cap][order], rec[landed])
    assert np.array_equal(gs[pre:cap][order], want[landed])
    if case == "one_ring":  # what infw_classify_xdp_mb_ex + infw_events_capture_xdp give on the same tensors
        ev1, smp1, cnt1 = _fill(cap * 24, 0xEE), _fill(cap * SB, 0xEE), _fill(1, 0, torch.int64)
        clf.classify_xdp_mb(tu[0], td_at[True], n, int(ring_if[0]), events=ev1, events_count=cnt1)
        clf.events_capture_xdp(tu[0], td_at[True], n, ev1, cnt1, smp1)
        r1, s1 = ev1.cpu().numpy().view(np.uint64).reshape(-1, 3), smp1.cpu().numpy().reshape(-1, SB)
        o1 = np.argsort(r1[:, 2], kind="stable")
        assert np.array_equal(r1[o1], grec[:cap][order]) and np.array_equal(s1[o1], gs[:cap][order])


def test_xdp_rings_ex_bad_arguments_and_no_ops(env):
    wl, m, clf = env
    u, d, ev, smp = _fill(4096, 1), _fill(12, 0, torch.int32), _fill(96, 0xEE), _fill(4 * SB + 8, 0xEE)
    cnt, res = _fill(1, 3, torch.int64), _fill(2, -1, torch.int32)
    arr = clf._xdp_ring_array([(u, d, 2, 1, res, None)])
    size, e, c, s = C.sizeof(N.XdpRingsEx), ev.data_ptr(), cnt.data_ptr(), smp.data_ptr()
    for ex in ((size - 8, 0, e, 4, c, s), (size, 1, e, 4, c, s), (size, 0, None, 4, c, s), (size, 0, e, 4, None, s),
               (size, 0, e, 4, c, s + 4)):  # size, flags, samples without events, events without a count, misaligned
        assert N.lib.infw_classify_xdp_rings_ex(clf._ctx, 0, arr, 1, C.byref(N.XdpRingsEx(*ex)), None) == -22
    ok, empty = N.XdpRingsEx(size, 0, e, 4, c, s), clf._xdp_ring_array([(u, d, 0, 1, res, None)] * 3)
    for a, k, ex in ((arr, 0, None), (arr, 0, C.byref(ok)), (empty, 3, None), (empty, 3, C.byref(ok))):  # no ring; empty
        assert N.lib.infw_classify_xdp_rings_ex(clf._ctx, 0, a, k, ex, None) == 0
    assert N.lib.infw_events_capture_xdp_rings(clf._ctx, 0, empty, 3, e, 0, c, s, None) == 0
    assert int(cnt.item()) == 3 and (ev == 0xEE).all() and (smp == 0xEE).all() and (res == -1).all()
