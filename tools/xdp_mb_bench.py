#!/usr/bin/env python3
"""Cost of infw_classify_xdp_mb's chain pass: one AF_XDP ring of N descriptors over a umem in HBM
(2048-B chunks, configs[2] frames, one ifindex), classified by infw_classify_xdp and by infw_classify_xdp_mb in
alternation in one process, HIP events around each call.  Single-descriptor frames first (both calls compute the same:
checked), then the same descriptors as chains of 3 (a third of the lookups).  Prints one JSON line.
--events: the same two rings also with a deny-event buffer of n records (infw_classify_xdp_mb_ex), alternated with the
plain calls, and infw_events_capture_xdp timed over the records the chains of 3 produced.

--rings [R] --ring-n M: the shape a daemon polls — R rings (default 64) of M descriptors (default 2048), chains of 1-3,
each ring its own umem in HBM and the interfaces of the workload in turn — (a) as R calls of infw_classify_xdp_mb and
(b) as one infw_classify_xdp_rings, alternated over the same data (the answers are compared once); then one ring of
--n descriptors through both calls.  Per arm: HIP events around the group and the host's wall-clock time of issuing it.
With --events three more arms over the same rings, each with a deny-event buffer and sample slots for every descriptor:
per ring infw_classify_xdp_mb_ex then infw_events_capture_xdp; one infw_classify_xdp_rings_ex with fused samples; one
infw_classify_xdp_rings_ex then infw_events_capture_xdp_rings (the record counts of the three are compared once).
With --split two more arms over the same rings: one infw_classify_xdp_rings_split (forward and fill lists written on the
device), and infw_classify_xdp_rings followed by what a host does without it — a D2H of the verdict bytes, a wait, and
one numpy boolean index per ring and list on one thread (a C loop would be faster than this host form); its issue time
is the whole step.  The lists of the two are compared once.

--decode [N]: infw_events_decode alone over N (default 2^20) sample slots — see decode_mode.
--sort [N]: infw_events_sort alone over N (default 2^20) event records, beside torch's stable argsort — see sort_mode.

    python tools/xdp_mb_bench.py [--n 16777216] [--rounds 20] [--events] [--rings [64] --ring-n 2048 [--split]]
    python tools/xdp_mb_bench.py --decode [1048576] [--rounds 20]
    python tools/xdp_mb_bench.py --sort [1048576] [--rounds 20]
"""
import ctypes as C
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ingress-node-firewall_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import infw  # noqa: E402
from infw import workloads as W  # noqa: E402

STRIDE = 2048


def rings_mode(args, clf, wl):
    n, R, M, dev = args.n, args.rings, args.ring_n, torch.device("cuda", 0)
    assert R * M <= n and args.rounds >= 20, "the rings are cut from the large ring's umem; at least 20 timed rounds"
    umem = torch.zeros(n * STRIDE, dtype=torch.uint8, device=dev)
    lin, plen, ifx = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    wl.gen_frames_device(umem, STRIDE, lin, plen, ifx, 0, 0)
    ifs = torch.argsort(torch.bincount(ifx), descending=True).tolist()
    ifs = ifs[:int((torch.bincount(ifx) > 0).sum())]
    rng = np.random.default_rng(3)
    opt = np.full(n, infw.XDP_PKT_CONTD, np.int32)  # chain lengths drawn from {1, 2, 3}
    opt[np.cumsum(rng.integers(1, 4, n))[:n].clip(max=n) - 1] = 0
    desc = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    addr = torch.arange(n, dtype=torch.int64, device=dev) * STRIDE
    desc[:, 0], desc[:, 1] = (addr & 0xFFFFFFFF).to(torch.int32), (addr >> 32).to(torch.int32)
    desc[:, 2], desc[:, 3] = torch.where(lin < 80, lin, plen), torch.from_numpy(opt).to(dev)
    small = desc[:R * M].clone()  # ring r: descriptors [r M, (r + 1) M) over its own umem, addresses from 0
    small[:, 0], small[:, 1] = desc[:M, 0].repeat(R), desc[:M, 1].repeat(R)
    res, res2 = (torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(2))
    ver = torch.empty(n, dtype=torch.uint8, device=dev)

    def rings(out):
        return [(umem[r * M * STRIDE:(r + 1) * M * STRIDE], small[r * M:(r + 1) * M], M, ifs[r % len(ifs)],
                 out[r * M:(r + 1) * M], ver[r * M:(r + 1) * M]) for r in range(R)]
    ra, rb, extra = rings(res), rings(res2), {}
    arms = {"per_ring_calls": lambda: [clf.classify_xdp_mb(u, d, m, i, results=o, verdicts=v) for u, d, m, i, o, v in ra],
            "one_rings_call": lambda: clf.classify_xdp_rings(rb),
            "large_xdp_mb": lambda: clf.classify_xdp_mb(umem, desc, n, ifs[0], results=res, verdicts=ver),
            "large_xdp_rings": lambda: clf.classify_xdp_rings([(umem, desc, n, ifs[0], res2, ver)])}
    cnts = {}
    if args.events:
        rec, sb = C.sizeof(infw._native.EventRec), infw._native.EVENT_SAMPLE_BYTES
        evb = {k: torch.zeros(R * M * rec, dtype=torch.uint8, device=dev) for k in "abc"}
        smb = {k: torch.empty(R * M * sb, dtype=torch.uint8, device=dev) for k in "abc"}
        cnts = {k: torch.zeros(R if k == "a" else 1, dtype=torch.int64, device=dev) for k in "abc"}

        def per_ring_ev():
            for r, (u, d, m, i, o, v) in enumerate(ra):
                e, c = evb["a"][r * M * rec:(r + 1) * M * rec], cnts["a"][r:r + 1]
                clf.classify_xdp_mb(u, d, m, i, results=o, verdicts=v, events=e, events_count=c)
                clf.events_capture_xdp(u, d, m, e, c, smb["a"][r * M * sb:(r + 1) * M * sb])

        def rings_ev_then_capture():
            clf.classify_xdp_rings(rb, events=evb["c"], events_count=cnts["c"])
            clf.events_capture_xdp_rings(rb, evb["c"], cnts["c"], smb["c"])
        arms.update(per_ring_ev_capture=per_ring_ev, one_rings_ev_then_capture=rings_ev_then_capture,
                    one_rings_ev_fused=lambda: clf.classify_xdp_rings(rb, events=evb["b"], events_count=cnts["b"],
                                                                      samples=smb["b"]))
    if args.split:
        sp = torch.full((R * M, 4), -1, dtype=torch.int32, device=dev)
        sf = torch.full((R * M,), -1, dtype=torch.int64, device=dev)
        sn = torch.full((R,), -1, dtype=torch.int32, device=dev)
        lists = [(sp[r * M:(r + 1) * M], sf[r * M:(r + 1) * M]) for r in range(R)]
        desc_h = small.cpu().numpy()  # the host's own view of its rings, as a daemon has it
        addr_h = np.ascontiguousarray(desc_h[:, :2]).view(np.int64).ravel() & ((1 << 48) - 1)
        ver_h, host_out = torch.empty(R * M, dtype=torch.uint8).pin_memory(), {}

        def rings_then_host_split():
            clf.classify_xdp_rings(rb)
            ver_h.copy_(ver[:R * M], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            v = ver_h.numpy() == infw.XDP_PASS
            host_out["pass"] = [desc_h[r * M:(r + 1) * M][v[r * M:(r + 1) * M]] for r in range(R)]
            host_out["fill"] = [addr_h[r * M:(r + 1) * M][~v[r * M:(r + 1) * M]] for r in range(R)]
        # beside the plain small-rings arms, ahead of the 2^24-descriptor ones: an arm that follows those pays ~0.3 ms
        # more to issue (their 0.5-GB scratch blocks are then what the pool has to cut its 4 MB from — supposed)
        head = {k: arms.pop(k) for k in ("per_ring_calls", "one_rings_call")}
        arms = {**head, "one_rings_split_call": lambda: clf.classify_xdp_rings_split(rb, lists, sn),
                "one_rings_call_host_split": rings_then_host_split, **arms}
    dev_ms, host_ms = {k: [] for k in arms}, {k: [] for k in arms}
    for rnd in range(-3, args.rounds):  # three warm-up rounds
        for c in cnts.values():  # each event arm appends to its own buffer, once per round
            c.zero_()
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            t1 = time.perf_counter()
            e1.synchronize()
            if rnd >= 0:
                dev_ms[k].append(e0.elapsed_time(e1))
                host_ms[k].append((t1 - t0) * 1e3)
            if rnd == -3 and k in ("one_rings_call", "large_xdp_rings"):
                assert torch.equal(res, res2), k + ": differs from infw_classify_xdp_mb ring by ring"
                res.fill_(-1), res2.fill_(-1)
            if rnd == -3 and k == "one_rings_call_host_split":  # after the device split: the same lists
                cnt, gp, gf = sn.cpu().numpy(), sp.cpu().numpy(), sf.cpu().numpy()
                for r in range(R):
                    assert cnt[r] == len(host_out["pass"][r]) and 0 < cnt[r] < M, "split: pass counts"
                    assert np.array_equal(gp[r * M:r * M + cnt[r]], host_out["pass"][r]), "split: pass lists differ"
                    assert np.array_equal(gf[r * M:(r + 1) * M - cnt[r]], host_out["fill"][r]), "split: fill lists"
                extra = {**extra, "passed": int(cnt.sum())}
            if rnd == -3 and k == "one_rings_ev_fused":  # the last of the three event arms
                assert int(cnts["a"].sum()) == int(cnts["b"]) == int(cnts["c"]) > 0, "event counts differ"
                extra = {"event_records": int(cnts["b"])}
    stat = lambda t: {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in t.items()}
    d, h = stat(dev_ms), stat(host_ms)
    if args.events:
        extra.update({"per_ring_ev_over_fused_" + w: t["per_ring_ev_capture"]["median"] / t["one_rings_ev_fused"]["median"]
                      for w, t in (("event", d), ("host", h))})
    print(json.dumps({**extra, "rings": R, "ring_n": M, "n_large": n, "rounds": args.rounds,
                      "kernel": clf.variant(infw.INPUT_FRAMES), "event_ms": d, "host_issue_ms": h,
                      "per_ring_over_one_call_event": d["per_ring_calls"]["median"] / d["one_rings_call"]["median"],
                      "per_ring_over_one_call_host": h["per_ring_calls"]["median"] / h["one_rings_call"]["median"],
                      "large_mb_over_large_rings_event": d["large_xdp_mb"]["median"] / d["large_xdp_rings"]["median"],
                      "gdesc_per_s": {k: (n if k.startswith("large") else R * M) / v["median"] / 1e6
                                      for k, v in d.items()}}))


def decode_mode(args):
    """infw_events_decode over --decode records of the case-table mix of tests/test_events_decode.py, HIP events around
    each call; beside it the path it replaces (D2H of the 272-B slots, then events.drain on the host) and the new
    host side (D2H of the 64-B records, then events.format_records), the two Python loops over the first 65536 records."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_events_decode import NAMES, TABLE
    from infw import events as E
    n, dev, sub = args.decode, torch.device("cuda", 0), 1 << 16
    clf = infw.Classifier(devices=[0])
    smp = torch.from_numpy(np.resize(TABLE, (n, TABLE.shape[1]))).to(dev)
    cnt = torch.tensor([n], dtype=torch.int64, device=dev)
    out = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    smp_h, out_h = torch.empty(smp.shape, dtype=torch.uint8).pin_memory(), torch.empty(out.shape, dtype=torch.uint8).pin_memory()
    arms = {"decode": lambda: clf.events_decode(smp, cnt, n, out=out),
            "d2h_samples": lambda: smp_h.copy_(smp, non_blocking=True),
            "d2h_records": lambda: out_h.copy_(out, non_blocking=True)}
    ms = {k: [] for k in arms}
    for rnd in range(-3, args.rounds):  # three warm-up rounds
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rnd >= 0:
                ms[k].append(e0.elapsed_time(e1))
    assert np.array_equal(out_h.numpy()[:sub], infw.events_decode_host(smp_h.numpy()[:sub])), "device != host records"
    t0 = time.perf_counter()
    want = E.drain(smp_h.numpy()[:sub], sub, NAMES)
    t1 = time.perf_counter()
    got = E.format_records(out_h.numpy()[:sub], sub, NAMES)
    t2 = time.perf_counter()
    assert got == want, "format_records != drain"
    rates = W.line_rates(0)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    ns = med["decode"] * 1e6 / n
    print(json.dumps({"records": n, "rounds": args.rounds, "build_id": infw.build_id(), "event_ms_median": med,
                      "event_ms_min": {k: min(v) for k, v in ms.items()}, "event_ms_max": {k: max(v) for k, v in ms.items()},
                      "decode_ns_per_record": ns, "stream_GB_per_s": rates["stream_GB_per_s"],
                      "decode_fraction_of_stream": (272 + 64) / ns / rates["stream_GB_per_s"],
                      "d2h_samples_ns_per_record": med["d2h_samples"] * 1e6 / n,
                      "d2h_records_ns_per_record": med["d2h_records"] * 1e6 / n,
                      "host_drain_ns_per_record": (t1 - t0) * 1e9 / sub,
                      "host_format_records_ns_per_record": (t2 - t1) * 1e9 / sub}))


def sort_mode(args):
    """infw_events_sort over --sort records with random pkt_index below index_bound = 2^27 (4 digit passes), HIP events
    around each call, alternated with the yardstick a caller has without it: torch.argsort(key, stable=True) and an
    index_select of the records viewed as (n, 3) int64 — which also needs the count on the host, not timed here.  The
    sort is in place, so the unsorted records are copied back before each timed call, outside the events."""
    n, dev, bound = args.sort, torch.device("cuda", 0), 1 << 27
    clf = infw.Classifier(devices=[0])
    src = torch.randint(0, 1 << 62, (n, 3), dtype=torch.int64, device=dev, generator=torch.Generator(dev).manual_seed(5))
    src[:, 2] = src[:, 2] % bound
    ev, out = torch.empty_like(src), torch.empty_like(src)
    cnt = torch.tensor([n], dtype=torch.int64, device=dev)
    arms = {"events_sort": lambda: clf.events_sort(ev.view(torch.uint8).reshape(-1), cnt, n, bound),
            "torch_argsort_select": lambda: torch.index_select(ev, 0, torch.argsort(ev[:, 2], stable=True), out=out)}
    ms = {k: [] for k in arms}
    for rnd in range(-3, args.rounds):  # three warm-up rounds
        for k, fn in arms.items():
            ev.copy_(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rnd >= 0:
                ms[k].append(e0.elapsed_time(e1))
    ev.copy_(src)
    arms["events_sort"]()
    assert torch.equal(ev, out), "events_sort != stable argsort + index_select"
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps({"records": n, "index_bound": bound, "rounds": args.rounds, "build_id": infw.build_id(),
                      "event_ms_median": med, "event_ms_min": {k: min(v) for k, v in ms.items()},
                      "event_ms_max": {k: max(v) for k, v in ms.items()},
                      "sort_ns_per_record": med["events_sort"] * 1e6 / n,
                      "torch_over_events_sort": med["torch_argsort_select"] / med["events_sort"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--events", action="store_true")
    ap.add_argument("--rings", type=int, nargs="?", const=64, default=0)
    ap.add_argument("--ring-n", type=int, default=2048)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--decode", type=int, nargs="?", const=1 << 20, default=0)
    ap.add_argument("--sort", type=int, nargs="?", const=1 << 20, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    if args.decode:
        return decode_mode(args)
    if args.sort:
        return sort_mode(args)
    n, dev = args.n, torch.device("cuda", 0)
    wl = W.Workload(W.CFG2_MIXED_1M)
    clf = infw.Classifier(devices=[0], max_entries=wl.n_entries + 16)
    wl.load_into(clf)
    clf.commit()
    if args.rings:
        return rings_mode(args, clf, wl)
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
