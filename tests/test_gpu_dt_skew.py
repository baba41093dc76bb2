"""The decision lines' skewed cut codes on the GPU: the hand-built tables of dt_skew_tables.py (classes that take the
codes 6 and 7, that stay uniform, that take one line) and a packet at every cut edge and every rule edge x {TCP, UDP,
SCTP, ICMP} x {IPv4, IPv6}, through every input form of the classify kernel and the two-phase form.  Result words,
verdicts and per-rule counters are bit-exact against the oracle."""
import numpy as np
import pytest
import torch

import infw
import orc
from infw.batch import SoaBatch

import dt_skew_tables as T

pytestmark = pytest.mark.gpu
STRIDE = 128


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def probes():
    hdr, cap, pl, ifx, tup = T.probe_frames(at_least=4096)
    m = orc.OracleMap()
    for k, v in T.entries():
        assert m.update(k, v) == 0
    res, ver, stats, _ = m.classify_frames(hdr, cap, pl, ifx, nthreads=4)
    return dict(hdr=hdr, cap=cap, pl=pl, ifx=ifx, tup=tup, res=res, ver=ver, stats=stats)


def _clf(**options):
    clf = infw.Classifier(devices=[0], options=options)
    for k, v in T.entries():
        clf.update(infw.LpmIpKeySt.from_buffer_copy(k), infw.RulesValSt.from_buffer_copy(v))
    clf.commit()
    assert clf.info()["dt_parts"] == 16
    return clf


def _check(clf, run, p, label):
    dev = torch.device("cuda", 0)
    n = len(p["res"])
    res = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ver = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    clf.stats_reset()
    run(res, ver)
    torch.cuda.synchronize()
    got = res.cpu().numpy().view(np.uint32)
    bad = np.nonzero(got != p["res"])[0]
    assert bad.size == 0, f"{label}: {bad.size} result words differ, first {bad[:6]}: {got[bad[:6]]} != {p['res'][bad[:6]]}"
    assert np.array_equal(ver.cpu().numpy(), p["ver"]), f"{label}: verdicts"
    assert np.array_equal(clf.stats_read_all(), p["stats"]), f"{label}: counters"


@pytest.mark.parametrize("split", [0, 1])
def test_every_input_form(probes, split):
    """classify, classify_c and classify_frames over the same packets: fused (split 0: the lean per-list kernel,
    its s_pl word in LDS) and two-phase (split 1: phase 1 computes the line, decide_kernel reads it)."""
    p = probes
    dev = torch.device("cuda", 0)
    n = len(p["res"])
    clf = _clf(split=split)
    assert clf.info()["split"] == split
    name = clf.variant()
    assert ".lean.pl" in name and ("+decide" in name) == bool(split), name
    batch = SoaBatch.from_tuples(p["tup"], dev)
    bc = clf.compact(batch)
    frames = np.zeros((n + 1, STRIDE), np.uint8)  # (one spare chunk behind the last frame)
    frames[:n, :p["hdr"].shape[1]] = p["hdr"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    dframes, lin, plen, fifx = torch.from_numpy(frames.reshape(-1)).to(dev), t(p["cap"]), t(p["pl"]), t(p["ifx"])
    before = clf.launch_counts()
    _check(clf, lambda r, v: clf.classify(batch, results=r, verdicts=v), p, f"classify split={split}")
    taken = tuple(a - b for a, b in zip(clf.launch_counts(), before))
    assert taken == ((1, 0) if split else (0, 0)), taken  # the launch took the form the name says
    _check(clf, lambda r, v: clf.classify_c(bc, results=r, verdicts=v), p, f"classify_c split={split}")
    _check(clf, lambda r, v: clf.classify_frames(dframes, lin, fifx, n, results=r, verdicts=v, pkt_len=plen,
                                                 stride=STRIDE), p, f"classify_frames split={split}")
    clf.close()


def test_uniform_only_option_gives_the_same_words(probes):
    """dt_adapt = 2, the same kernel over the uniform part counts alone."""
    p = probes
    clf = _clf(dt_adapt=2)
    batch = SoaBatch.from_tuples(p["tup"], torch.device("cuda", 0))
    _check(clf, lambda r, v: clf.classify(batch, results=r, verdicts=v), p, "dt_adapt=2")
    clf.close()
