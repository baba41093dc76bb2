"""infw_events_sort without a device: the symbol, and the argument errors a host-only context can answer."""
import ctypes as C

import pytest

import infw
from infw import _native as N

BUF = (C.c_uint64 * 8)()
A = C.addressof(BUF)


def test_symbol_bound():
    assert "infw_events_sort" in N.ABI_SYMBOLS and N.lib.infw_events_sort.argtypes[5] is C.c_uint64


@pytest.mark.parametrize("events,cap,count,want", [
    (A, 1, A + 48, -19),        # ENODEV: a well-formed call on a host-only context
    (None, 1, A + 48, -22),     # EINVAL: NULL events with cap != 0
    (A, 1, None, -22),          # NULL events_count
    (A + 4, 1, A + 48, -22),    # events not 8-byte aligned
    (A, 1 << 32, A + 48, -22),  # cap = 2^32
    (A, 0, A + 48, 0), (None, 0, None, 0),
])
def test_arguments_host_only(events, cap, count, want):
    c = infw.Classifier(flags=infw.F_HOST_ONLY)
    assert N.lib.infw_events_sort(c._ctx, 0, events, cap, count, 100, None) == want
