"""The ICP_* switches icp_create reads, and a context created under a chosen set of them (test_gpu_moments.py, test_gpu_plane_f64.py)."""
import contextlib

SWITCHES = ("ICP_TRACE", "ICP_MAILBOX", "ICP_RESIDENT", "ICP_ARMED", "ICP_NN_ROW", "ICP_NN_WAVES128", "ICP_NN_HIER", "ICP_SORT", "ICP_F64_SPARSE",
            "ICP_HOST_ROWS_MAX", "ICP_FUSED_TAIL", "ICP_NN_SPARSE", "ICP_NN_SHARE", "ICP_NN_ORDER", "ICP_SHARE_RESIDENT_AFTER", "ICP_SHARE_AUTO")


@contextlib.contextmanager
def fresh_context(pkg, monkeypatch, env):
    """the ICP_* switches are read by icp_create"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pkg.Context(0) as c:
        yield c
