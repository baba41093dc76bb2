"""The decision lines' skewed cut codes (csrc/infw_tables.h infw_dt_cut; csrc/tables.cpp compile_rule_list) on the
CPU: hand-built rule lists whose classes must take a skewed code, stay uniform, or take one line (dt_skew_tables.py),
walked by infw_debug_walk -- the kernel's own lookup code over the committed host image -- at every cut edge and every
rule edge, against the oracle."""
import numpy as np
import pytest

import infw
import orc

import dt_skew_tables as T

HDR = 72  # image.cpp Header
# (name, kind, element size) of the compiled tables in image.cpp's order, as tests/test_image_cpu.py lists them
_TABLES = [("if_keys", "v", 4), ("if_slot", "v", 4), ("if_mult", "p", 4), ("if_shift", "p", 4), ("n_slots", "p", 4),
           ("l16", "v", 4), ("nodes", "v", 64), ("vpool", "v", 4), ("n_tbl8_groups", "p", 8), ("tbl24", "v", 8),
           ("tbl8", "v", 4), ("short_mode", "p", 4), ("ltab", "v", 32), ("btab", "v", 64),
           ("n_buckets", "p", 8), ("n_overflow_groups", "p", 8), ("wild", "v", 4), ("n_wild", "p", 4),
           ("levels", "v", 1), ("desc", "v", 8), ("rules", "v", 8), ("dte", "v", 64), ("dtl", "v", 64),
           ("dt_plog2", "p", 4), ("dt_pl", "v", 4)]


def sections(img: bytes):
    """{name: (offset, bytes)} of an image's fields up to dt_pl."""
    out, o = {}, HDR
    u64 = lambda at: int.from_bytes(img[at:at + 8], "little")
    for per in (1200, 48):  # the interned values, then the entries
        o += 8 + u64(o) * per
    for name, kind, sz in _TABLES:
        if kind == "p":
            out[name] = (o, sz)
            o += sz
        else:
            n = u64(o)
            out[name] = (o + 8, n * sz)
            o += 8 + n * sz
    return out


def dt_pl_of(c):
    """(dt_plog2, the per-list cut-code words) of a committed context's exported image."""
    img = c.export_image()
    s = sections(img)
    words = np.frombuffer(img, np.uint32, s["dt_pl"][1] // 4, s["dt_pl"][0])
    return int.from_bytes(img[s["dt_plog2"][0]:s["dt_plog2"][0] + 4], "little"), words


def codes(words, n_lists):
    """Sorted (TCP code, UDP code) of the first n_lists words."""
    return sorted((int(w) & 7, (int(w) >> 3) & 7) for w in words[:n_lists])


def ctx(names="abcd", flags=infw.F_HOST_ONLY, **options):
    c = infw.Classifier(flags=flags, options=options)
    for k, v in T.entries(names):
        c.update(infw.LpmIpKeySt.from_buffer_copy(k), infw.RulesValSt.from_buffer_copy(v))
    c.commit()
    return c


@pytest.fixture(scope="module")
def probes():
    hdr, cap, pl, ifx, tup = T.probe_frames()
    m = orc.OracleMap()
    for k, v in T.entries():
        assert m.update(k, v) == 0
    want, _, _, _ = m.classify_frames(hdr, cap, pl, ifx, nthreads=4)
    assert (want != 0).sum() >= 200  # the probes do hit the rules: each of the 100-odd rules in both families
    return tup, want


def test_codes_chosen_and_walk_matches_oracle(probes):
    tup, want = probes
    c = ctx()
    assert c.info()["dt_parts"] == 16
    plog2, words = dt_pl_of(c)
    assert plog2 == 4 and words.size == 4096 and not words[4:].any()
    assert codes(words, 4) == sorted(T.EXPECT.values())
    got = c.debug_walk(tup)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("adapt", [2, 0])
def test_uniform_only_options(probes, adapt):
    """dt_adapt = 2 keeps the per-list part counts without the skewed codes, 0 has no per-list word at all; both
    classify exactly like the default."""
    tup, want = probes
    c = ctx(dt_adapt=adapt)
    plog2, words = dt_pl_of(c)
    assert plog2 == 4
    if adapt == 0:
        assert words.size == 0
    else:
        assert codes(words, 4) == sorted(T.EXPECT_UNIFORM.values())
        assert all(((int(w) >> (3 * k)) & 7) <= 4 for w in words for k in range(7))
    assert np.array_equal(c.debug_walk(tup), want)


def test_image_codes_need_16_line_regions(probes):
    """import_image accepts the codes 5..7 exactly when dt_plog2 is 4."""
    import xxhash
    tup, want = probes
    img = bytearray(ctx().export_image())
    ok = infw.Classifier(flags=infw.F_HOST_ONLY)
    ok.import_image(bytes(img))
    assert np.array_equal(ok.debug_walk(tup), want)
    s = sections(img)
    off = s["dt_pl"][0]
    w0 = int.from_bytes(img[off:off + 4], "little")
    img[off:off + 4] = ((w0 & ~7) | 5).to_bytes(4, "little")                     # list 0's TCP class: code 5
    img[s["dt_plog2"][0]:s["dt_plog2"][0] + 4] = (3).to_bytes(4, "little")       # in 8-line regions
    img[64:72] = xxhash.xxh64(bytes(img[HDR:]), seed=0).intdigest().to_bytes(8, "little")
    c = infw.Classifier(flags=infw.F_HOST_ONLY)
    with pytest.raises(infw.InfwError) as e:
        c.import_image(bytes(img))
    assert e.value.errno == 22 and "part count" in infw._native.last_error()
    assert c.count() == 0


def test_incremental_append_uses_the_chooser(probes):
    """A commit that appends a shape-a list patches the image in place: the new list's word gets the skewed code and
    the image walks like a full compile's."""
    tup, want = probes
    inc = ctx("bcd", flags=infw.F_HOST_ONLY)
    for k, v in T.entries("a"):
        inc.update(infw.LpmIpKeySt.from_buffer_copy(k), infw.RulesValSt.from_buffer_copy(v))
    inc.commit()
    assert inc.info()["commit_mode"] == infw.COMMIT_INCREMENTAL
    _, words = dt_pl_of(inc)
    assert (int(words[3]) & 7, (int(words[3]) >> 3) & 7) == T.EXPECT["a"]      # appended: the last list
    assert codes(words, 4) == sorted(T.EXPECT.values())
    got = inc.debug_walk(tup)
    assert np.array_equal(got, ctx().debug_walk(tup)) and np.array_equal(got, want)
