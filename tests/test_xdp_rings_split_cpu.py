"""infw_classify_xdp_rings_split without a device: bound with the header's argument types, its 16-B per-ring struct, and
a host-only context is -ENODEV."""
import ctypes as C

import infw
from infw import _native as N


def test_xdp_rings_split_bound_and_needs_a_device():
    f = N.lib.infw_classify_xdp_rings_split
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_void_p, C.c_int, C.POINTER(N.XdpRing), C.POINTER(N.XdpRingSplit), C.c_uint32,
                          C.c_void_p, C.c_void_p]
    assert "infw_classify_xdp_rings_split" in N.ABI_SYMBOLS and C.sizeof(N.XdpRingSplit) == 16
    c = infw.Classifier(flags=infw.F_HOST_ONLY)
    assert callable(c.classify_xdp_rings_split)
    ring = (N.XdpRing * 1)(N.XdpRing(16, 16, 1, 1, 0, None, None))
    assert f(c._ctx, 0, ring, (N.XdpRingSplit * 1)(N.XdpRingSplit(16, 16)), 1, 16, None) == -19  # ENODEV
