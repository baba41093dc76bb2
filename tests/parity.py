"""Shared parity helpers for tests/ and __graft_entry__.smoke().

Builds the same table in the GPU classifier (through the C ABI) and in the
oracle, classifies the same packets both ways and compares result words,
XDP verdicts and per-rule counters bit for bit.
"""
from __future__ import annotations

import numpy as np

import infw
import orc
from infw import workloads as W


def oracle_for(wl: W.Workload) -> "orc.OracleMap":
    m = orc.OracleMap(max_entries=wl.n_entries + 16)
    for k, v in wl.entries():
        rc = m.update(k, v)
        assert rc == 0, rc
    return m


_REGISTER_REFUSED = []


def host_register_refused():
    """None where the HIP runtime page-locks memory the process already owns, else the runtime's own refusal as text.
    Asked of the runtime itself (hipHostRegister of one anonymous page through ctypes, on the libamdhip64 this process
    already runs), not of the library under test: where the runtime accepts the page, a failing infw_host_register
    fails its tests.  Some virtualised GPU hosts refuse every registration of a user mapping (shared or private,
    touched or not, any flag: hipErrorInvalidValue) although RLIMIT_MEMLOCK is unlimited, mlock() of the same page
    succeeds and hipHostMalloc works: the refusal is the platform's (no user-pointer mappings for the device there),
    not a locked-memory limit.  The probe's sticky error is consumed; asked once per process."""
    if not _REGISTER_REFUSED:
        import ctypes as C
        import mmap
        path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln)
        hip = C.CDLL(path)
        hip.hipHostRegister.argtypes = [C.c_void_p, C.c_size_t, C.c_uint]
        hip.hipHostUnregister.argtypes = [C.c_void_p]
        hip.hipGetErrorString.restype = C.c_char_p
        mm = mmap.mmap(-1, 4096)
        buf = C.c_char.from_buffer(mm)
        e = hip.hipHostRegister(C.addressof(buf), 4096, 0)
        if e == 0:
            assert hip.hipHostUnregister(C.addressof(buf)) == 0
            _REGISTER_REFUSED.append(None)
        else:
            hip.hipGetLastError()
            _REGISTER_REFUSED.append(f"hipHostRegister of one anonymous page: {hip.hipGetErrorString(e).decode()}")
        del buf
    return _REGISTER_REFUSED[0]


def need_host_register():
    """Skips the calling test, before it does any work, where the HIP runtime itself refuses to page-lock memory the
    process already owns (host_register_refused): infw_host_register cannot work there."""
    import pytest
    why = host_register_refused()
    if why:
        pytest.skip(f"needs hipHostRegister of the process's own memory, which the HIP runtime here refuses ({why})")


def pinned(a: np.ndarray) -> np.ndarray:
    """A copy of `a` in page-locked host memory allocated as such (hipHostMalloc, through torch); the array keeps its
    tensor alive."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()


def oracle_run(m, wl: W.Workload, start: int, n: int, threads: int = 8):
    hdr, cap, pl, ifx = wl.frames(start, n)
    res, ver, stats, _ = m.classify_frames(hdr, cap, pl, ifx, nthreads=threads)
    return res, ver, stats, (hdr, cap, pl, ifx)


def gpu_run(clf, batch, n: int, dev_index: int = 0):
    """Classify a device SoA batch; returns (results u32, verdicts u8) on the host."""
    import torch
    res = torch.empty(n, dtype=torch.int32, device=batch.device)
    ver = torch.empty(n, dtype=torch.uint8, device=batch.device)
    clf.classify(batch, results=res, verdicts=ver, dev=dev_index)
    torch.cuda.synchronize(batch.device)
    return res.cpu().numpy().view(np.uint32), ver.cpu().numpy()


def stats_from_results(results: np.ndarray, pkt_len: np.ndarray) -> np.ndarray:
    """Per-rule counters implied by result words (kernel.c:441-456, :376-387)."""
    out = np.zeros((1024, 4), np.uint64)
    act = results & 0xFF
    key = (results >> 8) & 0xFFFF
    for a, col in ((infw.XDP_PASS, 0), (infw.XDP_DROP, 2)):
        sel = (act == a) & (key < 1024)
        out[:, col] += np.bincount(key[sel], minlength=1024).astype(np.uint64)
        out[:, col + 1] += np.bincount(key[sel], weights=pkt_len[sel].astype(np.float64),
                                       minlength=1024).astype(np.uint64)
    return out


def check_cfg(cfg: int, n: int, n_prefixes: int = 0, n_templates: int = 0, start: int = 0, device=None,
              layout: str = "standard", launch=None):
    """End-to-end parity on one config: device-generated SoA vs host frames + oracle.
    layout "compact": the batch is re-laid out by infw_soa_compact and classified by infw_classify_c."""
    import torch
    from infw.batch import SoaBatch
    device = device or torch.device("cuda", 0)
    wl = W.Workload(cfg, n_prefixes=n_prefixes, n_templates=n_templates)
    clf = infw.Classifier(devices=[device.index or 0], max_entries=wl.n_entries + 16)
    wl.load_into(clf)
    clf.commit()
    if launch is not None:
        clf.set_launch(*launch)
    m = oracle_for(wl)
    ores, over, ostats, (hdr, cap, pl, ifx) = oracle_run(m, wl, start, n)
    batch = SoaBatch.empty(n, device)
    wl.gen_device(batch, start, device.index or 0)
    torch.cuda.synchronize(device)
    host_tuples = W.pack_frames(hdr, cap, pl, ifx)
    dev_tuples = batch.to_tuples()
    assert np.array_equal(dev_tuples, host_tuples), "device generator != host frames packed"
    clf.stats_reset()
    if layout == "compact":
        bc = clf.compact(batch)
        res = torch.empty(n, dtype=torch.int32, device=device)
        ver = torch.empty(n, dtype=torch.uint8, device=device)
        clf.classify_c(bc, results=res, verdicts=ver)
        torch.cuda.synchronize(device)
        gres, gver = res.cpu().numpy().view(np.uint32), ver.cpu().numpy()
    else:
        gres, gver = gpu_run(clf, batch, n)
    gstats = clf.stats_read_all()
    return dict(wl=wl, clf=clf, oracle=m, ores=ores, over=over, ostats=ostats, gres=gres, gver=gver,
                gstats=gstats, pkt_len=pl, batch=batch)


def assert_parity(r, label=""):
    bad = np.nonzero(r["gres"] != r["ores"])[0]
    assert bad.size == 0, f"{label}: {bad.size} result words differ, first {bad[:8]}: " \
                          f"gpu={r['gres'][bad[:8]]} oracle={r['ores'][bad[:8]]}"
    assert np.array_equal(r["gver"], r["over"]), f"{label}: verdicts differ"
    assert np.array_equal(r["gstats"], r["ostats"]), f"{label}: per-rule counters differ"
