"""infw_classify_xdp_rings without a device: bound with the header's argument types; a host-only context is -ENODEV."""
import ctypes as C

import infw
from infw import _native as N


def test_xdp_rings_bound_and_needs_a_device():
    f = N.lib.infw_classify_xdp_rings
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_void_p, C.c_int, C.POINTER(N.XdpRing), C.c_uint32, C.c_void_p]
    assert "infw_classify_xdp_rings" in N.ABI_SYMBOLS and infw.XDP_RINGS_MAX == 1024
    c = infw.Classifier(flags=infw.F_HOST_ONLY)
    assert callable(c.classify_xdp_rings)
    assert f(c._ctx, 0, (N.XdpRing * 1)(N.XdpRing(16, 16, 1, 1, 0, None, None)), 1, None) == -19  # ENODEV
