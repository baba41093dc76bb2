"""infw_classify_xdp_mb without a device: a host-only context has no device tables to classify against."""
import infw
from infw import _native as N


def test_xdp_mb_needs_a_device():
    c = infw.Classifier(flags=infw.F_HOST_ONLY)
    assert N.lib.infw_classify_xdp_mb(c._ctx, 0, 16, 16, 1, 1, None, None, None) == -19  # ENODEV
