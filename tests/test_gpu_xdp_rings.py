"""Every multi-buffer AF_XDP ring of a poll in one call (infw_classify_xdp_rings): per ring what infw_classify_xdp_mb
computes, on the ring's own umem, ifindex and outputs, no chain running into the next ring.  Reference: the CPU oracle
over the frame lists the host builds from each ring's options column (one oracle call over the lists laid end to end:
frames are classified independently, counters add up), bit for bit.  Continuations point at rule-matching decoys."""
import numpy as np
import pytest
import torch

import infw
from infw import _native as N
from infw import workloads as W

from parity import oracle_for
from test_gpu_xdp_mb import _random_chains

pytestmark = pytest.mark.gpu
T, K, CONTD = infw.XDP_CHAIN_TILE, infw.XDP_CHAIN_CARRY, infw.XDP_PKT_CONTD


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    wl = W.Workload(W.CFG2_MIXED_1M, n_prefixes=20000, n_templates=64)
    clf = infw.Classifier(devices=[0], max_entries=wl.n_entries + 16)
    wl.load_into(clf)
    clf.commit()
    hdr, _, pl, ifx = wl.frames(4242, 200000)
    return wl, oracle_for(wl), clf, (hdr, pl, ifx)


CASES = {  # name -> (ring sizes, umem stride, one umem for all rings)
    "boundaries": lambda rng: ([1, 63, 64, 65, 0, 200, 3 * T + 77, 2], 2048, False),
    "carry_rounds": lambda rng: (np.diff(np.r_[0, np.sort(rng.choice((2 * K + 37) * T, 36, replace=False)),
                                               (2 * K + 37) * T]), 128, False),  # 37 unequal sizes, tiles > 2 K
    "max_rings": lambda rng: (rng.integers(1, 4, infw.XDP_RINGS_MAX), 2048, True),
    "one_ring": lambda rng: ([2 * T + 19], 2048, False),
}


def _build(m, pool, case, rng):
    """Flat over all rings: descriptors, the oracle's answers and counters, the conditions against a vacuous pass."""
    (sizes, stride, shared), (hdr, pl, ifx) = CASES[case](rng), pool
    sizes = np.asarray(sizes, np.int64)
    top = np.argsort(-np.bincount(ifx))[:4]  # the workload's most frequent ifindexes, one per ring in turn
    ring_if = top[np.arange(sizes.size) % 4].astype(np.uint32)
    ring_of, first, n = np.repeat(np.arange(sizes.size), sizes), np.cumsum(sizes) - sizes, int(sizes.sum())
    opts = [_random_chains(s, rng) for s in sizes]
    for o in opts if case == "boundaries" else []:  # every ring ends on an open chain
        o[-1:] = CONTD
    if case == "carry_rounds":  # one chain over more than two whole tiles inside the largest ring
        opts[int(sizes.argmax())][100:100 + 3 * T + 50] = CONTD
    opt = np.concatenate(opts)
    src = np.empty(n, np.int64)  # frames of the ring's own interface for the heads, other ones of it for the decoys
    for q in top:
        own, sel = np.nonzero(ifx == q)[0], ring_if[ring_of] == q
        src[sel] = own[np.arange(sel.sum()) % own.size]
    decoy = hdr[np.roll(src, 1)]
    starts_of = lambda head: (np.cumsum(head) - 1, np.nonzero(head)[0])
    joined = np.r_[True, (opt[:-1] & CONTD) == 0]  # the heads if the rings were one ring
    head = joined.copy()
    head[first[sizes > 0]] = True
    frame_of, starts = starts_of(head)
    ln = np.where(head, pl[src], rng.integers(1, 1500, n)).astype(np.uint32)
    long_heads = starts[np.r_[np.diff(starts), n - starts[-1]] > 1]
    ln[long_heads[0::7]], ln[long_heads[1::7]] = 9, 30  # heads cut below 14 and below 34 bytes
    dif = ring_if[ring_of]

    def oracle(fo, st, ifindex):
        total = np.add.reduceat(ln.astype(np.uint64), st).astype(np.uint32)
        res, ver, stats, _ = m.classify_frames(hdr[src[st]], ln[st], total, ifindex, nthreads=8)
        return res[fo], ver[fo], stats
    want, wver, wst = oracle(frame_of, starts, dif[starts])
    dres = m.classify_frames(decoy, np.full(n, 80, np.uint32), ln, dif, nthreads=8)[0]
    # rule hits; a parsed continuation, ring 0's ifindex for every ring, the rings run together: each changes an answer
    seen = ((want[starts] & 0xFF).astype(bool).mean(), (((dres & 0xFF) != 0) & (dres != want) & ~head).any(),
            (oracle(frame_of, starts, np.full(starts.size, ring_if[0], np.uint32))[0] != want).any(),
            (oracle(*starts_of(joined), dif[np.nonzero(joined)[0]])[0] != want).any())
    desc, umems = np.zeros((n, 4), np.uint32), []
    for ix in ([np.arange(n)] if shared else [np.nonzero(ring_of == r)[0] for r in range(sizes.size)]):
        k = ix.size
        base = rng.permutation(k + 7)[:k].astype(np.uint64) * np.uint64(stride)
        off = rng.integers(0, stride - 96, k).astype(np.uint64) * np.uint64(len(umems) & 1)  # odd umems: unaligned mode
        umem = np.zeros((k + 7) * stride, np.uint8)
        umem[(base + off)[:, None] + np.arange(80, dtype=np.uint64)] = np.where(head[ix, None], hdr[src[ix]], decoy[ix])
        desc[ix, :2] = (base | off << np.uint64(48)).view(np.uint32).reshape(k, 2)
        umems.append(torch.from_numpy(umem))
    desc[:, 2], desc[:, 3] = ln, opt
    return sizes, first, ring_if, umems * (sizes.size if shared else 1), desc, want, wver, wst, seen


def _run(clf, call, n):
    res, ver = (torch.full((n,), v, dtype=t, device="cuda:0") for v, t in ((-1, torch.int32), (7, torch.uint8)))
    before = clf.launch_counts(), len(infw.kernel_variants())
    clf.stats_reset()
    call(res, ver)
    torch.cuda.synchronize()
    assert (clf.launch_counts(), len(infw.kernel_variants())) == before
    return res.cpu().numpy().view(np.uint32), ver.cpu().numpy(), clf.stats_read_all()


@pytest.mark.parametrize("case", list(CASES))
def test_xdp_rings_match_oracle(env, case):
    wl, m, clf, pool = env
    sizes, first, ring_if, umems, desc, want, wver, wst, seen = _build(m, pool, case, np.random.default_rng(11))
    assert seen[0] > 0.3 and seen[1] and (seen[2] or sizes.size == 1) and (seen[3] or case != "boundaries"), seen
    td = torch.from_numpy(desc.view(np.int32))
    td_at = {True: td.to("cuda:0"), False: td.pin_memory()}
    hbm = [case != "boundaries" or r % 2 == 0 for r in range(sizes.size)]  # boundaries: HBM and pinned in turn
    put = {id(u): u.to("cuda:0") for u in umems[:1 if case == "max_rings" else None]}  # one copy of a shared umem
    umems = [put.get(id(u)) if h else u.pin_memory() for u, h in zip(umems, hbm)]
    no_res, no_ver = (2, 5) if case == "boundaries" else (-1, -1)

    def rings(res, ver):
        return [(umems[r], td_at[hbm[r]][f:f + s], int(s), int(ring_if[r]), None if r == no_res else res[f:f + s],
                 None if r == no_ver else ver[f:f + s]) for r, (f, s) in enumerate(zip(first, sizes))]
    got, gver, gst = _run(clf, lambda res, ver: clf.classify_xdp_rings(rings(res, ver)), desc.shape[0])
    if case == "boundaries":  # a ring's NULL output is skipped for that ring only: its slots keep the sentinel
        want[first[no_res]:first[no_res + 1]], wver[first[no_ver]:first[no_ver + 1]] = 0xFFFFFFFF, 7
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (case, bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(gver, wver) and np.array_equal(gst, wst)
    if case == "one_ring":  # what infw_classify_xdp_mb computes on the same tensors
        u, d, s, q = umems[0], td_at[True], int(sizes[0]), int(ring_if[0])
        sres, sver, sst = _run(clf, lambda res, ver: clf.classify_xdp_mb(u, d, s, q, results=res, verdicts=ver), s)
        assert np.array_equal(sres, got) and np.array_equal(sver, gver) and np.array_equal(sst, gst)


def test_xdp_rings_bad_arguments_and_no_ops(env):
    wl, m, clf, pool = env
    u, d = (torch.zeros(k, dtype=t, device="cuda:0") for k, t in ((4096, torch.uint8), (12, torch.int32)))
    for rings in ([(u, d, 0, 1, None, None)] * (infw.XDP_RINGS_MAX + 1),  # 1025 rings; misaligned descriptors
                  [(u, d, 2, 1, None, None), (u, d[1:], 2, 1, None, None)]):
        with pytest.raises(infw.InfwError) as e:
            clf.classify_xdp_rings(rings)
        assert e.value.errno == 22, len(rings)
    flagged = (N.XdpRing * 1)(N.XdpRing(u.data_ptr(), d.data_ptr(), 2, 1, 1, None, None))
    assert N.lib.infw_classify_xdp_rings(clf._ctx, 0, flagged, 1, None) == -22
    for rings in ([], [(u, d, 0, 1, None, None)] * 3):  # no ring, and only empty rings
        got, gver, gst = _run(clf, lambda res, ver: clf.classify_xdp_rings([r[:4] + (res, ver) for r in rings]), 4)
        assert not gst.any() and (got == 0xFFFFFFFF).all() and (gver == 7).all()
