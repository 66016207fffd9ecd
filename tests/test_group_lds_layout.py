"""CPU: the per-instance LDS layout of the 16-lane kernels (mahi-mpc_amd/csrc/sqp_group.h group_lds) through a small
host shim.  A group's block starts where the size says and its arrays lie where the offsets say; a disagreement is a
silent read of a neighbour's LDS, so the checks are exact.

tests/golden/group_lds_doubles.json was recorded from group_lds_doubles of the commit before group_lds existed, with
the same shim built against that tree -- never from the code under test.  The two byte counts in ANCHORS are typed in
from the comments of sqp_group.h, independently of the file.  (The grid is the issue's.  For the (10, 6, 5) shape
group_const_doubles is 0, nx + nu being 16, so its three (kc, kh) cases are (0, 0), (0, 0) and (0, head): the constant
block is exercised on three of the four shapes.)"""
import ctypes
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mahi-mpc_amd", "csrc")
_G = json.load(open(os.path.join(ROOT, "tests", "golden", "group_lds_doubles.json")))
GOLDEN = [dict(zip(_G["columns"], r)) for r in _G["rows"]]
FIELDS = ["U", "D", "DX", "DU", "F", "C", "Fq", "Fqd", "Fu", "R", "Hold", "Lin", "Kh", "Kc", "doubles"]
SHAPES = [(4, 2, 2), (8, 4, 4), (10, 6, 5), (3, 1, 1)]
HORIZONS = [1, 2, 3, 17, 26, 30, 50]

# no kernel is instantiated: the device side of the shim is empty
SRC = r"""
#include "sqp_group.h"
extern "C" void lds_layout(int nx, int nu, int nq, int N, int bounded, int linear, int kc, int kh, int* out) {
    const mmpc::GroupLds L = mmpc::group_lds(nx, nu, nq, N, bounded != 0, linear != 0, kc, kh);
    const int v[15] = {L.U, L.D, L.DX, L.DU, L.F, L.C, L.Fq, L.Fqd, L.Fu, L.R, L.Hold, L.Lin, L.Kh, L.Kc, L.doubles};
    for (int i = 0; i < 15; ++i) out[i] = v[i];
}
extern "C" int lds_stride(int nx, int nu, int nq, int N, int bounded, int linear, int kc, int kh) {
    return mmpc::group_lds_doubles(nx, nu, nq, N, bounded != 0, linear != 0, kc, kh);   // the kernels' group stride
}
extern "C" int const_doubles(int nx, int nu) { return mmpc::group_const_doubles(nx, nu); }
extern "C" int head_doubles(int nx, int nu) { return mmpc::group_head_doubles(nx, nu); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("group_lds")
    src, so = d / "lds.hip", d / "lds.so"
    src.write_text(SRC)
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-shared", "-fPIC", "-w",
                    "-I", CSRC, str(src), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def _layout(shim, nx, nu, nq, N, bounded, linear, kc, kh):
    out = (ctypes.c_int * 15)()
    shim.lds_layout(nx, nu, nq, N, int(bounded), int(linear), kc, kh, out)
    return dict(zip(FIELDS, out))


def _grid(shim):
    for nx, nu, nq in SHAPES:
        c, hd = shim.const_doubles(nx, nu), shim.head_doubles(nx, nu)
        for N in HORIZONS:
            for bounded in (0, 1):
                for linear in (0, 1):
                    for kc, kh in ((0, 0), (c, 0), (c, hd)):
                        yield nx, nu, nq, N, bounded, linear, kc, kh


def test_sizes_are_the_earlier_formula(shim):
    keys = [(r["nx"], r["nu"], r["nq"], r["N"], r["bounded"], r["linear"], r["kc"], r["kh"]) for r in GOLDEN]
    assert keys == list(_grid(shim)) and len(keys) == 4 * 7 * 2 * 2 * 3
    for r, k in zip(GOLDEN, keys):
        assert _layout(shim, *k)["doubles"] == r["doubles"], k
        assert shim.lds_stride(*k) == r["doubles"], k


def test_cfg2_workgroups(shim):
    """cfg#2 (2-link arm, N = 30, nonlinear), four instances per workgroup: 40,384 B unbounded (constant block 8, head
    block 42 doubles) and 40,960 B control-bounded (constant block alone)"""
    assert (shim.const_doubles(4, 2), shim.head_doubles(4, 2)) == (8, 42)
    assert 4 * 8 * _layout(shim, 4, 2, 2, 30, False, False, 8, 42)["doubles"] == 40_384
    assert 4 * 8 * _layout(shim, 4, 2, 2, 30, True, False, 8, 0)["doubles"] == 40_960


def test_offsets_are_ordered_and_the_pad_rule(shim):
    padded = set()
    for k in _grid(shim):
        nx, nu, nq, N, bounded, linear, kc, kh = k
        L = _layout(shim, *k)
        na = nx - nq
        off = [0] + [L[f] for f in FIELDS]
        over = 2 * na * na   # the d recursion's over-read behind sFqd
        want_pad = over if N * (na * nu + nx) < over else 0
        # strictly ordered, except across an array the variant does not have (a field is where the array in front of it
        # ends): the hold targets (unbounded), the linear-mode block with the pad, the head block, the constant block
        empty = {"Lin"} if not bounded else set()
        empty |= {"Kh"} if not linear and not want_pad else set()
        empty |= {"Kc"} if kh == 0 else set()
        empty |= {"doubles"} if kc == 0 else set()
        for f, a, b in zip(FIELDS, off, off[1:]):
            assert (a == b) if f in empty else (a < b), (k, f, L)
        assert L["Kc"] + kc == L["doubles"] and L["Kh"] + kh == L["Kc"], (k, L)
        pad = L["Kh"] - (L["Lin"] + (na * (nq + na + nu) + nx if linear else 0))
        assert pad == want_pad, (k, L)
        if pad:
            padded.add((nx, nu, nq, N))
    assert (8, 4, 4, 1) in padded and (4, 2, 2, 30) not in padded, padded
