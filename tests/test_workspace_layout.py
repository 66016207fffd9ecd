"""CPU: the size of the handle's workspace (mmpc.hip WorkspaceLayout, reserved_layout) is what it was before the layout
became one struct.  mmpc_reserve_workspace writes *bytes before it looks for a device, so a handle that cannot reach one
reports it (with 256 compute units assumed) and allocates nothing; the return code is then MMPC_ERR_NO_DEVICE.  The
handles ask for a device index no machine has, so that the test is the same with and without a GPU.
tests/golden/workspace_bytes.json was recorded with the library of the commit before that change, never with the code
under test; equality is exact: a solve captured in a hipGraph relies on every reader of the layout agreeing to the byte."""
import ctypes as C
import json
import os

import pytest

from conftest import ROOT

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")))["rows"]
DIMS = {"two_link_arm": (4, 2), "exo_arm": (8, 4)}
NO_SUCH_DEVICE = 4096   # mmpc_create touches no device
# read from the earlier library independently of the golden file
ANCHORS = {("two_link_arm", 30, 4096): 232_587_520, ("two_link_arm", 1, 1): 1_678_416,
           ("exo_arm", 50, 65536): 10_185_867_520, ("exo_arm", 2, 5): 1_920_320}


def _reserve(s, B):
    n = C.c_uint64(12345)
    rc = s._L.mmpc_reserve_workspace(s._h, B, C.byref(n))   # not Solver.reserve_workspace: it raises on NO_DEVICE
    return rc, int(n.value)


def test_golden_covers_the_shapes():
    keys = {(r["model"], r["N"], r["B"]) for r in GOLDEN}
    assert keys == {(m, N, B) for m in DIMS for N in (1, 2, 17, 30, 50) for B in (1, 5, 4096, 65536)}
    for k, v in ANCHORS.items():
        assert [r["bytes"] for r in GOLDEN if (r["model"], r["N"], r["B"]) == k] == [v], k


@pytest.mark.parametrize("model", sorted(DIMS))
@pytest.mark.parametrize("N", [1, 2, 17, 30, 50])
def test_reserved_bytes_are_unchanged(model, N, mmpc_mod, tmp_path):
    nx, nu = DIMS[model]
    s = mmpc_mod.Solver(mmpc_mod.write_model_json(str(tmp_path / "m.json"), model, nx, nu, 2000, N, model=model),
                        device=NO_SUCH_DEVICE)
    for r in GOLDEN:
        if r["model"] == model and r["N"] == N:
            assert _reserve(s, r["B"]) == (-6, r["bytes"]), (model, N, r["B"])
    s.close()


def test_empty_batch_reserves_nothing(mmpc_mod, tmp_path):
    s = mmpc_mod.Solver(mmpc_mod.write_model_json(str(tmp_path / "m.json"), "two_link_arm", 4, 2, 2000, 30,
                                                  model="two_link_arm"), device=NO_SUCH_DEVICE)
    assert _reserve(s, 0) == (0, 0)
    s.close()
