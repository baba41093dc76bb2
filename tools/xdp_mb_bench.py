#!/usr/bin/env python3
"""Cost of infw_classify_xdp_mb's chain pass: one AF_XDP ring of N descriptors over a umem in HBM
(2048-B chunks, configs[2] frames, one ifindex), classified by infw_classify_xdp and by infw_classify_xdp_mb in
alternation in one process, HIP events around each call.  Single-descriptor frames first (both calls compute the same:
checked), then the same descriptors as chains of 3 (a third of the lookups).  Prints one JSON line.
--events: the same two rings also with a deny-event buffer of n records (infw_classify_xdp_mb_ex), alternated with the
plain calls, and infw_events_capture_xdp timed over the records the chains of 3 produced.

    python tools/xdp_mb_bench.py [--n 16777216] [--rounds 20] [--events]
"""
import ctypes as C
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ingress-node-firewall_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import infw  # noqa: E402
from infw import workloads as W  # noqa: E402

STRIDE = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--events", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    n, dev = args.n, torch.device("cuda", 0)
    wl = W.Workload(W.CFG2_MIXED_1M)
    clf = infw.Classifier(devices=[0], max_entries=wl.n_entries + 16)
    wl.load_into(clf)
    clf.commit()
    umem = torch.zeros(n * STRIDE, dtype=torch.uint8, device=dev)
    lin, plen, ifx = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    wl.gen_frames_device(umem, STRIDE, lin, plen, ifx, 0, 0)
    ring_if = int(torch.bincount(ifx).argmax())
    desc = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    addr = torch.arange(n, dtype=torch.int64, device=dev) * STRIDE
    desc[:, 0], desc[:, 1] = (addr & 0xFFFFFFFF).to(torch.int32), (addr >> 32).to(torch.int32)
    desc[:, 2] = torch.where(lin < 80, lin, plen)
    chains = desc.clone()
    chains[:, 3] = (torch.arange(n, device=dev) % 3 != 2).to(torch.int32) * infw.XDP_PKT_CONTD
    res, res2 = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    ver = torch.empty(n, dtype=torch.uint8, device=dev)
    calls = {"xdp": (clf.classify_xdp, desc, res), "xdp_mb": (clf.classify_xdp_mb, desc, res2),
             "xdp_mb_chains3": (clf.classify_xdp_mb, chains, res2)}
    n_rec = 0
    if args.events:
        rec = C.sizeof(infw._native.EventRec)
        ev = torch.zeros(n * rec, dtype=torch.uint8, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        evs = dict(events=ev, events_count=cnt)
        clf.classify_xdp_mb(umem, chains, n, ring_if, **evs)
        n_rec = int(cnt.item())  # the records of the chains of 3: one sample slot each
        smp = torch.empty(max(n_rec, 1) * infw._native.EVENT_SAMPLE_BYTES, dtype=torch.uint8, device=dev)
        calls.update({"xdp_mb_ev": (lambda *a, **k: clf.classify_xdp_mb(*a, **k, **evs), desc, res2),
                      "xdp_mb_chains3_ev": (lambda *a, **k: clf.classify_xdp_mb(*a, **k, **evs), chains, res2),
                      "capture_chains3": (lambda u, d, n, i, **k: clf.events_capture_xdp(u, d, n, ev[:n_rec * rec], cnt,
                                                                                         smp), chains, res2)})
    ms = {k: [] for k in calls}
    for rnd in range(-3, args.rounds):  # three warm-up rounds
        for k, (fn, d, r) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if k.endswith("_ev"):
                cnt.zero_()
            e0.record()
            fn(umem, d, n, ring_if, results=r, verdicts=ver)
            e1.record()
            e1.synchronize()
            if rnd >= 0:
                ms[k].append(e0.elapsed_time(e1))
        if rnd == -3:
            clf.classify_xdp_mb(umem, desc, n, ring_if, results=res2, verdicts=ver)
            assert torch.equal(res, res2), "single-descriptor frames: xdp_mb differs from xdp"
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps({"n": n, "rounds": args.rounds, "kernel": clf.variant(infw.INPUT_FRAMES), "capture_records": n_rec,
                      "median_ms": med,
                      "min_ms": {k: min(v) for k, v in ms.items()},
                      "max_ms": {k: max(v) for k, v in ms.items()},
                      "gdesc_per_s": {k: n / v / 1e6 for k, v in med.items()},
                      "xdp_over_xdp_mb": med["xdp"] / med["xdp_mb"],
                      "xdp_over_xdp_mb_chains3": med["xdp"] / med["xdp_mb_chains3"]}))


if __name__ == "__main__":
    main()
