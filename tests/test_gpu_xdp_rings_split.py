"""Every ring of a poll classified and split on the device (infw_classify_xdp_rings_split): ring r's descriptors whose
frame passed, verbatim and in ring order, in its pass list, addr & (2^48 - 1) of every other one in its fill list, the
pass count in n_pass[r], and no slot at or past the counts touched.  Reference: numpy over the CPU oracle's
per-descriptor verdicts, bit for bit; result words, verdicts and counters as test_gpu_xdp_rings asserts them."""
import numpy as np
import pytest
import torch

import infw

from test_gpu_xdp_rings import CASES, CONTD, _build, _run, env  # noqa: F401  (env: that module's fixture)

pytestmark = pytest.mark.gpu
MASK48 = np.uint64((1 << 48) - 1)


@pytest.mark.parametrize("case", list(CASES))  # boundaries, carry_rounds, max_rings, one_ring
def test_xdp_rings_split_matches_oracle(env, case):
    wl, m, clf, pool = env
    sizes, first, ring_if, umems, desc, want, wver, wst, _ = _build(m, pool, case, np.random.default_rng(11))
    n, R = desc.shape[0], sizes.size
    ok, ring_of = wver == 2, np.repeat(np.arange(R), sizes)
    want_n = np.bincount(ring_of, weights=ok, minlength=R).astype(np.int32)
    rel = np.arange(n) - first[ring_of]
    # against a vacuous pass: both lists in use; of several rings one ends on the pass side (one_ring's ends on the
    # other); where a ring has 64 descriptors, one such ring with both sides and a passed chain that runs over a
    # 64-descriptor chunk boundary
    assert ok.any() and not ok.all() and (R == 1 or ok[(first + sizes - 1)[sizes > 0]].any())
    if sizes.max() >= 64:
        assert ((sizes >= 64) & (want_n > 0) & (want_n < sizes)).any()
        assert (ok[1:] & (rel[1:] > 0) & (rel[1:] % 64 == 0) & ((desc[:-1, 3] & CONTD) != 0)).any()
    no_res, no_ver, no_pass, no_fill = (2, 5, 5, 7) if case == "boundaries" else (-1, -1, -1, -1)
    addr = np.ascontiguousarray(desc[:, :2]).view(np.uint64).ravel() & MASK48
    want_pass, want_fill = np.full((n, 4), 0xFFFFFFFF, np.uint32), np.full(n, 2**64 - 1, np.uint64)
    for r, (f, s, k) in enumerate(zip(first, sizes, want_n)):  # slots at or past the counts keep the sentinel
        if r != no_pass:
            want_pass[f:f + k] = desc[f:f + s][ok[f:f + s]]
        if r != no_fill:
            want_fill[f:f + s - k] = addr[f:f + s][~ok[f:f + s]]
    td = torch.from_numpy(desc.view(np.int32)).to("cuda:0")
    put = {id(u): u.to("cuda:0") for u in umems[:1 if case == "max_rings" else None]}  # one copy of a shared umem
    tp, tf, tn = (torch.full(shape, -1, dtype=t, device="cuda:0")
                  for shape, t in (((n, 4), torch.int32), ((n,), torch.int64), ((R,), torch.int32)))
    split = [(None if r == no_pass else tp[f:f + s], None if r == no_fill else tf[f:f + s])
             for r, (f, s) in enumerate(zip(first, sizes))]
    both_null = case == "one_ring"  # results and verdicts both NULL: classify and split only

    def call(res, ver):
        rings = [(put[id(umems[r])], td[f:f + s], int(s), int(ring_if[r]),
                  None if both_null or r == no_res else res[f:f + s],
                  None if both_null or r == no_ver else ver[f:f + s]) for r, (f, s) in enumerate(zip(first, sizes))]
        clf.classify_xdp_rings_split(rings, split, tn)
    got, gver, gst = _run(clf, call, n)  # also: launch counts and the variant registry unchanged
    if both_null:
        want[:], wver[:] = 0xFFFFFFFF, 7
    if case == "boundaries":
        want[first[no_res]:first[no_res + 1]], wver[first[no_ver]:first[no_ver + 1]] = 0xFFFFFFFF, 7
    assert np.array_equal(got, want) and np.array_equal(gver, wver) and np.array_equal(gst, wst)
    assert np.array_equal(tn.cpu().numpy(), want_n), (tn.cpu().numpy()[:8], want_n[:8])
    bad = np.nonzero((tp.cpu().numpy().view(np.uint32) != want_pass).any(1))[0]
    assert bad.size == 0, (case, bad[:5], ring_of[bad[:5]])
    bad = np.nonzero(tf.cpu().numpy().view(np.uint64) != want_fill)[0]
    assert bad.size == 0, (case, bad[:5], ring_of[bad[:5]])


def test_xdp_rings_split_bad_arguments_and_no_rings(env):
    wl, m, clf, pool = env
    u, d, tp, tf = (torch.zeros(k, dtype=t, device="cuda:0")
                    for k, t in ((4096, torch.uint8), (12, torch.int32), (12, torch.int32), (2, torch.int64)))
    tn = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    ring = [(u, d, 2, 1, None, None)]
    for split, n_pass in ((None, tn), ([(tp, tf)], None), ([(tp[1:], tf)], tn)):  # the last: pass not 16-B aligned
        with pytest.raises(infw.InfwError) as e:
            clf.classify_xdp_rings_split(ring, split, n_pass)
        torch.cuda.synchronize()
        assert e.value.errno == 22 and int(tn) == -1  # nothing was launched, not even the zeroing of n_pass
    clf.classify_xdp_rings_split([], [], tn)  # n_rings == 0 returns 0
