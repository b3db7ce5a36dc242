"""`iefvad_auc_ap_grouped` (csrc/metrics.h: per-class AUC / AP and the Ano-AUC of the evaluation tail in one pass) -- what can be
checked without a GPU: the two entries exist, the workspace size behaves, and every argument check runs before the first HIP call and
names the argument it refuses.  The pointers handed over here are never dereferenced: each call must fail in its checks."""
import ctypes as C

import pytest

from iefvad_amd import lib as L


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    return L.load_library()


def test_entries_exist_and_are_required(lib):
    for s in ("iefvad_auc_ap_grouped", "iefvad_auc_ap_grouped_workspace_bytes"):
        assert s in L.SYMBOLS and hasattr(lib, s)
    assert lib.iefvad_abi_version() == 8                  # entries were added, no struct changed


def test_workspace_size(lib):
    wb = lib.iefvad_auc_ap_grouped_workspace_bytes
    assert wb(0, 4) == 0
    assert wb(100, 0) == 0 and wb(100, 65) == 0
    sizes = [1, 63, 4095, 4096, 4097, 12289, 30000, 69500, 145000, 2097152]
    for g in (1, 3, 14, 64):
        got = [wb(n, g) for n in sizes]
        assert all(x > 0 and x % 256 == 0 for x in got)
        assert got == sorted(got), (g, got)
        assert got[0] >= lib.iefvad_auc_ap_workspace_bytes(1)
    for n in sizes:
        got = [wb(n, g) for g in range(1, 65)]
        assert got == sorted(got), n
    assert wb(2097152, 14) >= lib.iefvad_auc_ap_workspace_bytes(2097152)


def test_argument_checks_run_before_any_hip_call(lib):
    ok = C.c_void_p(0x10000)                              # 256-byte aligned, never read: every call below stops in its checks
    need = lib.iefvad_auc_ap_grouped_workspace_bytes(100, 4)

    def call(scores=ok, gt=ok, group=ok, n=100, repeat=16, ngroups=4, auc=ok, ap=ok, frames=ok, ws=ok, ws_bytes=need):
        rc = lib.iefvad_auc_ap_grouped(scores, gt, group, n, repeat, ngroups, auc, ap, frames, ws, ws_bytes, None)
        return rc, L.last_error()

    for kw, frag in [(dict(ngroups=0), "ngroups"), (dict(ngroups=65), "ngroups"), (dict(ngroups=-1), "ngroups"),
                     (dict(repeat=0), "repeat"), (dict(repeat=1 << 24), "repeat"),
                     (dict(n=1 << 29, ws_bytes=1 << 40), "n * repeat"), (dict(n=0), "n = 0"),
                     (dict(group=None), "group"), (dict(auc=None, ap=None), "auc and ap"),
                     (dict(scores=None), "scores"), (dict(gt=None), "gt_frames"), (dict(ws=None), "workspace"),
                     (dict(ws_bytes=need - 1), "workspace of"), (dict(ws_bytes=64), "workspace of"),
                     (dict(ws=C.c_void_p(0x10008)), "256-byte aligned")]:
        rc, msg = call(**kw)
        assert rc != 0, kw
        assert msg.startswith("iefvad_auc_ap_grouped:") and frag in msg, (kw, msg)


def test_grouped_wrapper_has_no_host_fallback():
    """Like device_auc_ap: scores in host memory are an error, not a quiet sklearn run."""
    import torch
    from iefvad_amd import harness
    with pytest.raises(RuntimeError, match="HIP device only"):
        harness.device_grouped_auc_ap(torch.rand(64), torch.zeros(64 * 16), torch.zeros(64, dtype=torch.uint8), 3)
