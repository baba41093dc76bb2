"""A multi-buffer AF_XDP ring (XDP_USE_SG) as the feed (infw_classify_xdp_mb): one frame per descriptor chain,
classified on the head's bytes with the chain's summed length and counted once; every descriptor of a chain receives
its frame's result word and verdict.  The reference is the CPU oracle over the frame list built on the host from the
options column, compared bit for bit (result words, verdicts, per-rule counters).  Every continuation descriptor points
at valid umem bytes holding another, rule-matching header: a kernel that parses one changes results and counters."""
import numpy as np
import pytest
import torch

import infw
from infw import workloads as W

from parity import oracle_for

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
    return wl, oracle_for(wl), clf


def _random_chains(n, rng):
    """options with chain lengths drawn from {1, 2, 3}, whole frames."""
    opt = np.full(n, CONTD, np.uint32)
    opt[np.cumsum(rng.integers(1, 4, n))[:n].clip(max=n) - 1] = 0
    return opt


def _spans(n, spans, open_tail=0):
    opt = np.zeros(n, np.uint32)
    for s, l in spans:
        opt[s:s + l - 1] = CONTD
    opt[n - open_tail:] = CONTD
    return opt


SHAPES = {  # name -> (options column, umem stride)
    "mixed": lambda rng: (_random_chains(3 * T + 77, rng), 2048),
    # chains across a 64-lane boundary, a wave boundary inside the workgroup and a tile boundary, one chain over two
    # whole tiles (tiles without a head), 2- and 3-chains after it, and a chain left open at n - 1
    "edges": lambda rng: (_spans(5 * T + 9, [(62, 4), (T // 2 - 2, 5), (T - 2, 4), (T + 44, 2 * T + T - 10),
                                              (4 * T + 40, 2), (4 * T + 42, 3)], open_tail=3), 2048),
    "carry_loop": lambda rng: (_random_chains((2 * K + 37) * T + 5, rng), 128),
    "singles": lambda rng: (np.zeros(2 * T + 19, np.uint32), 2048),
}


def _ring(wl, m, opt, stride, mode, rng):
    """umem, descriptors, ring ifindex and the oracle's per-descriptor answer for the options column."""
    n = opt.size
    hdr, _, pl, ifx = wl.frames(4242, n)
    decoy = wl.frames(900000, n)[0]
    ring_if = int(np.bincount(ifx).argmax())
    head = np.r_[True, (opt[:-1] & CONTD) == 0]
    frame_of, starts = np.cumsum(head) - 1, np.nonzero(head)[0]
    ln = np.where(head, pl, rng.integers(1, 1500, n)).astype(np.uint32)
    long_heads = starts[np.r_[np.diff(starts), n - starts[-1]] > 1]
    ln[long_heads[0::7]], ln[long_heads[1::7]] = 9, 30  # heads cut below 14 and below 34 bytes, large totals
    total = np.add.reduceat(ln.astype(np.uint64), starts).astype(np.uint32)
    ifx_all = np.full(starts.size, ring_if, np.uint32)
    want, wver, wst, _ = m.classify_frames(hdr[starts], ln[starts], total, ifx_all, nthreads=8)
    dres = m.classify_frames(decoy, np.full(n, 80, np.uint32), ln, np.full(n, ring_if, np.uint32), nthreads=8)[0]
    # the share of frames that hit a rule; whether a parsed continuation would show (it hits a rule other than its head's)
    seen = (want & 0xFF).astype(bool).mean(), (((dres & 0xFF) != 0) & (dres != want[frame_of]) & ~head).any()
    chunks = rng.permutation(n + 7)[:n].astype(np.uint64) * np.uint64(stride)
    off = rng.integers(0, stride - 96, n).astype(np.uint64) if mode == "unaligned" else np.zeros(n, np.uint64)
    base = chunks + np.uint64(0 if mode == "unaligned" or stride < 512 else 256)  # aligned: chunk + headroom
    umem = np.zeros((n + 7) * stride, np.uint8)
    umem[(base + off)[:, None] + np.arange(80, dtype=np.uint64)] = np.where(head[:, None], hdr, decoy)
    desc = np.zeros((n, 4), np.uint32)
    desc[:, :2] = (base | off << np.uint64(48)).view(np.uint32).reshape(n, 2)
    desc[:, 2], desc[:, 3] = ln, opt
    return umem, desc, ring_if, want[frame_of], wver[frame_of], wst, seen


def _run(clf, call, tu, td, n, ring_if):
    dev = torch.device("cuda", 0)
    res = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ver = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    before = clf.launch_counts(), len(infw.kernel_variants())
    clf.stats_reset()
    call(tu, td, n, ring_if, results=res, verdicts=ver)
    torch.cuda.synchronize()
    assert (clf.launch_counts(), len(infw.kernel_variants())) == before
    return res.cpu().numpy().view(np.uint32), ver.cpu().numpy(), clf.stats_read_all()


@pytest.mark.parametrize("shape,where,mode", [("mixed", w, a) for w in ("hbm", "host") for a in ("aligned", "unaligned")]
                         + [(s, "hbm", "aligned") for s in ("edges", "carry_loop", "singles")])
def test_xdp_mb_matches_oracle(env, shape, where, mode):
    wl, m, clf = env
    rng = np.random.default_rng(5)
    opt, stride = SHAPES[shape](rng)
    umem, desc, ring_if, want, wver, wst, seen = _ring(wl, m, opt, stride, mode, rng)
    assert seen[0] > 0.3 and (seen[1] or shape == "singles")
    tu, td = torch.from_numpy(umem), torch.from_numpy(desc.view(np.int32))
    tu, td = (tu.to("cuda:0"), td.to("cuda:0")) if where == "hbm" else (tu.pin_memory(), td.pin_memory())
    got, gver, gst = _run(clf, clf.classify_xdp_mb, tu, td, opt.size, ring_if)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (shape, bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(gver, wver)
    assert np.array_equal(gst, wst)
    if shape == "singles":  # all options clear: what infw_classify_xdp computes
        sres, sver, sst = _run(clf, clf.classify_xdp, tu, td, opt.size, ring_if)
        assert np.array_equal(sres, got) and np.array_equal(sver, gver) and np.array_equal(sst, gst)


def test_xdp_mb_small_rings_and_bad_arguments(env):
    wl, m, clf = env
    umem, desc, ring_if, want, wver, wst, _ = _ring(wl, m, np.full(1, CONTD, np.uint32), 2048, "aligned",
                                                    np.random.default_rng(1))
    tu, td = torch.from_numpy(umem).to("cuda:0"), torch.from_numpy(desc.view(np.int32)).to("cuda:0")
    got, gver, gst = _run(clf, clf.classify_xdp_mb, tu, td, 1, ring_if)  # one open descriptor is one frame
    assert got[0] == want[0] and gver[0] == wver[0] and np.array_equal(gst, wst)
    got, gver, gst = _run(clf, clf.classify_xdp_mb, tu, td, 0, ring_if)  # an empty ring is a no-op
    assert not gst.any()
    pad = torch.zeros(12, dtype=torch.int32, device="cuda:0")
    with pytest.raises(infw.InfwError) as e:  # descriptors not 16-byte aligned
        clf.classify_xdp_mb(tu, pad[1:], 2, ring_if)
    assert e.value.errno == 22
