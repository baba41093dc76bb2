"""Multi-GPU plumbing on the device (one MI355X).

- bench.py through its spawn launcher at N = 1 (`--gpus 1 --spawn`): one rank process, an RCCL (nccl backend)
  process group of one, the HIP kernel's counters through StatsExchange's asynchronous all-reduce — the line's
  stats_digest equals the standalone run's, and it reports rccl_world_size 1 and the rank's kernel time.
- A context over four device slots (devices=[0, 0, 0, 0], what a node-wide daemon driving every GPU from one
  process uses; one card here) built by importing a compiled image (infw_table_import: no compile), then
  incrementally committed: every slot classifies like the oracle after each epoch, the slots upload / patch on
  their own host threads (info: n_device_slots, device_ms_max).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import infw
from infw import workloads as W
from infw.batch import SoaBatch
from parity import gpu_run, oracle_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _bench(*a):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *a], cwd=ROOT, env=e, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def test_spawn_rccl_world1_digest_equals_standalone():
    common = ["--steps", "3", "--warmup", "1", "--batch", str(1 << 22), "--prefixes", "50000", "--templates", "256",
              "--no-cpu-baseline"]
    solo = _bench("--gpus", "1", *common)
    spawned = _bench("--gpus", "1", "--spawn", *common)
    assert solo["rccl_world_size"] is None and spawned["rccl_world_size"] == 1
    assert spawned["config"]["stats_digest"] == solo["config"]["stats_digest"]
    assert spawned["config"]["packets_counted_in_stats"] == solo["config"]["packets_counted_in_stats"] > 0
    assert len(spawned["per_rank"]) == 1 and spawned["per_rank"][0]["kernel_ms_avg"] > 0
    assert spawned["n_gpus"] == 1 and spawned["value"] > 0


N_SMALL = 1 << 18
SMALL = ["--prefixes", "50000", "--templates", "256", "--warmup", "1"]


@pytest.fixture(scope="module")
def small_oracle():
    """The oracle's result words and counters for packets [0, N_SMALL) of the small table the bench runs below use."""
    wl = W.Workload(W.CFG2_MIXED_1M, n_prefixes=50000, n_templates=256)
    hdr, cap, pl, ifx = wl.frames(0, N_SMALL)
    ores, _, ost, _ = oracle_for(wl).classify_frames(hdr, cap, pl, ifx, nthreads=8)
    return ores.astype(np.float64), ost.astype(np.float64)


def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path, small_oracle):
    """A plain run measures the headline alone (no CPU baseline, no line-rate probe: those are --full's), times
    exactly --steps steps, and --dump-outputs writes what the last timed step computed: every result word (the batch
    is smaller than the sample) in packet order, equal to the oracle's, and the step's per-rule counters, whose
    digest is the line's."""
    from bench import stats_digest
    n, steps = N_SMALL, 3
    d = _bench("--gpus", "1", "--steps", str(steps), "--batch", str(n), *SMALL, "--dump-outputs", str(tmp_path))
    assert d["cpu_baseline"] is None and d["roofline"]["line_rates"] is None
    assert d["steps"] == steps and d["config"]["packets_counted_in_stats"] % steps == 0
    # value (Mpps) and ms_per_step say the same thing; ms_per_step is rounded to 0.001 ms, value to 0.01
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - n / d["ms_per_step"] / 1e3) <= d["value"] * 0.0006 / d["ms_per_step"] + 0.01
    assert sorted(os.listdir(tmp_path)) == ["results.npy", "stats.npy"]
    res, st = np.load(tmp_path / "results.npy"), np.load(tmp_path / "stats.npy")
    assert res.dtype == np.float64 and res.shape == (n,) and st.dtype == np.float64 and st.shape == (1024, 4)
    ores, ost = small_oracle
    assert np.array_equal(res, ores)
    assert np.array_equal(st, ost)
    assert stats_digest(st) == d["config"]["stats_digest"]
    assert int(st[:, 0].sum() + st[:, 2].sum()) * steps == d["config"]["packets_counted_in_stats"]


def test_full_run_adds_cpu_baseline_and_line_rates():
    """--full: the line carries the CPU baseline, whose check of the device's words against the oracle passes, and the
    line rates measured in the run; --no-cpu-baseline / --no-line-rates drop either again."""
    common = ["--gpus", "1", "--steps", "2", "--batch", str(N_SMALL), *SMALL, "--full"]
    d = _bench(*common)
    cb = d["cpu_baseline"]
    assert cb["gpu_results_bitexact_on_sample"] is True and cb["value"] > 0 and cb["unit"] == "Mpps"
    assert cb["sample"].startswith(f"first {N_SMALL} packets")
    assert set(d["roofline"]["line_rates"]) == {"l2_hit_G_per_s", "l2_miss_G_per_s", "stream_GB_per_s"}
    assert all(v > 0 for v in d["roofline"]["line_rates"].values())
    d = _bench(*common, "--no-cpu-baseline", "--no-line-rates")
    assert d["cpu_baseline"] is None and d["roofline"]["line_rates"] is None


def test_in_process_dump_equals_the_rank_paths(tmp_path, small_oracle):
    """--in-process --dump-outputs: two slots of half the batch each write their own words; together they are the
    rank path's (the oracle's) for the whole batch, and the counters summed over the slots are the whole batch's."""
    d = _bench("--in-process", "--gpus", "2", "--slots-on-gpu0", "--steps", "2", "--batch", str(N_SMALL // 2), *SMALL,
               "--dump-outputs", str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["results_slot0.npy", "results_slot1.npy", "stats.npy"]
    ores, ost = small_oracle
    got = np.concatenate([np.load(tmp_path / f"results_slot{s}.npy") for s in range(2)])
    assert got.dtype == np.float64 and np.array_equal(got, ores)
    assert np.array_equal(np.load(tmp_path / "stats.npy"), ost)
    assert d["device_slots"] == 2


def test_host_fed_dump_is_in_packet_order(tmp_path, small_oracle):
    """--xdp-ring host-packed --dump-outputs: the words the library left in the rings' host arrays at the last step,
    put back into packet order, are the oracle's for the same packets (the CPU baseline checks the same array)."""
    from bench import stats_digest
    n = 1 << 16
    d = _bench("--gpus", "1", "--xdp-ring", "host-packed", "--from-frames", "128", "--steps", "2", "--batch", str(n),
               *SMALL, "--full", "--no-line-rates", "--dump-outputs", str(tmp_path))
    assert d["roofline"]["xdp_ring"]["results_equal_packer_path"] is True and d["roofline"]["xdp_ring"]["rings"] > 1
    assert d["cpu_baseline"]["gpu_results_bitexact_on_sample"] is True
    res = np.load(tmp_path / "results.npy")
    assert res.shape == (n,) and np.array_equal(res, small_oracle[0][:n])
    assert stats_digest(np.load(tmp_path / "stats.npy")) == d["config"]["stats_digest"]


def test_four_slot_context_from_imported_image():
    wl = W.Workload(W.CFG2_MIXED_1M, n_prefixes=20000, n_templates=128)
    src = infw.Classifier(flags=infw.F_HOST_ONLY, max_entries=wl.n_entries + 64)
    wl.load_into(src)
    src.commit()
    clf = infw.Classifier(devices=[0, 0, 0, 0], max_entries=wl.n_entries + 64)
    clf.import_image(src.export_image())
    info = clf.info()
    assert info["imported"] == 1 and info["n_device_slots"] == 4 and info["device_ms_max"] > 0
    m = oracle_for(wl)
    dev = torch.device("cuda", 0)
    n = 1 << 15
    batches = []
    for d in range(4):
        b = SoaBatch.empty(n, dev)
        wl.gen_device(b, d * n, 0)
        batches.append(b)
    keys = wl.keys_bytes().reshape(-1, 24)
    tmpl = wl.templates_bytes().reshape(-1, 1200)
    for epoch in range(3):
        for d in range(4):
            gres, _ = gpu_run(clf, batches[d], n, dev_index=d)
            hdr, cap, pl, ifx = wl.frames(d * n, n)
            ores, _, _, _ = m.classify_frames(hdr, cap, pl, ifx, nthreads=8)
            assert np.array_equal(gres, ores), (epoch, d)
        for i in range(epoch, keys.shape[0], 5):  # an incremental commit: deletes and rewrites
            kb = keys[i].tobytes()
            if i % 2:
                assert clf.delete_rc(infw.LpmIpKeySt.from_buffer_copy(kb)) == m.delete(kb)
            else:
                vb = tmpl[(i * 7 + epoch) % tmpl.shape[0]].tobytes()
                assert clf.update_rc(infw.LpmIpKeySt.from_buffer_copy(kb),
                                     infw.RulesValSt.from_buffer_copy(vb)) == m.update(kb, vb)
        clf.commit()
        assert clf.info()["commit_mode"] in (infw.COMMIT_INCREMENTAL, infw.COMMIT_REUPLOAD)
        assert clf.info()["n_device_slots"] == 4
