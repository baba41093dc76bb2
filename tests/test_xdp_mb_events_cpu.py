"""infw_classify_xdp_mb_ex / infw_events_capture_xdp without a device: a host-only context has nothing to run them on."""
import infw
from infw import _native as N


def test_xdp_mb_events_need_a_device():
    c = infw.Classifier(flags=infw.F_HOST_ONLY)
    assert N.lib.infw_classify_xdp_mb_ex(c._ctx, 0, 16, 16, 1, 1, None, None, None, None) == -19  # ENODEV
    assert N.lib.infw_events_capture_xdp(c._ctx, 0, 16, 16, 1, 16, 1, 16, 16, None) == -19
