"""CPU: the width-generic model functions of mahi-mpc_amd/csrc/two_link_fast.h and fast_trig.h compiled for the host.

TwoLinkFast::eval, eval_acc_jac and eval_hess instantiated with dpack<2> / dpack<3> values (W points at once, the
operations of the W chains in turn -- what the 16-lane kernel's paired stages run) must give, element by element, the
bytes of the double instantiation at that element's point: every operation keeps its operands and its order.  Built
with the device's trig path (sincos_fast_w, no libm branch) and with contraction off and on: a compiler that contracts
must contract both instantiations alike for the solver's outputs to stay what they were."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mahi-mpc_amd", "csrc")

SRC = r"""
#include <math.h>
#define MMPC_HD
#include "two_link_fast.h"
using namespace mmpc;
// in: n points of (x[4], u[2], lam[2]); out: per point acc[2] Fq[4] Fqd[4] Fu[4] xd[4] W[36] = 54 doubles
template <int W>
static void run(const double* in, double* out, long n) {
    for (long i = 0; i + W <= n; i += W) {
        dpack<W> x[4], u[2], l[2], acc[2], Fq[4], Fqd[4], Fu[4], xd[4], H[36];
        for (int e = 0; e < W; ++e) {
            const double* p = in + (i + e) * 8;
            for (int j = 0; j < 4; ++j) x[j].v[e] = p[j];
            for (int j = 0; j < 2; ++j) u[j].v[e] = p[4 + j], l[j].v[e] = p[6 + j];
        }
        TwoLinkFast::eval_acc_jac(x, u, acc, Fq, Fqd, Fu);
        TwoLinkFast::eval(x, u, xd);
        TwoLinkFast::eval_hess(x, u, l, H);
        for (int e = 0; e < W; ++e) {
            double* o = out + (i + e) * 54;
            for (int j = 0; j < 2; ++j) o[j] = acc[j].v[e];
            for (int j = 0; j < 4; ++j) o[2 + j] = Fq[j].v[e], o[6 + j] = Fqd[j].v[e], o[10 + j] = Fu[j].v[e], o[14 + j] = xd[j].v[e];
            for (int j = 0; j < 36; ++j) o[18 + j] = H[j].v[e];
        }
    }
}
extern "C" void pack_eval(int w, const double* in, double* out, long n) {
    if (w == 2) run<2>(in, out, n);
    else if (w == 3) run<3>(in, out, n);
    else
        for (long i = 0; i < n; ++i) {
            const double* p = in + i * 8;
            double* o = out + i * 54;
            TwoLinkFast::eval_acc_jac(p, p + 4, o, o + 2, o + 6, o + 10);
            TwoLinkFast::eval(p, p + 4, o + 14);
            TwoLinkFast::eval_hess(p, p + 4, p + 6, o + 18);
        }
}
"""


@pytest.fixture(scope="module", params=["off", "fast"])
def lib(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("two_link_pack_" + request.param)
    src = d / "tp.cpp"
    src.write_text(SRC)
    so = d / "tp.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-ffp-contract=" + request.param,
                    "-DMMPC_TRIG_DEVICE_PATH_ON_HOST", "-I", CSRC, str(src), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def _run(lib, w, pts):
    out = np.full((len(pts), 54), np.nan)
    P = ctypes.POINTER(ctypes.c_double)
    lib.pack_eval(ctypes.c_int(w), pts.ctypes.data_as(P), out.ctypes.data_as(P), ctypes.c_long(len(pts)))
    return out


@pytest.mark.parametrize("w", [2, 3])
def test_pack_elements_are_the_scalar_bytes(lib, w):
    rng = np.random.default_rng(21)
    n = 6000
    pts = np.empty((n, 8))
    pts[:, :2] = rng.uniform(-40.0, 40.0, (n, 2))      # angles over many quadrants
    pts[:, 2:4] = rng.uniform(-6.0, 6.0, (n, 2))
    pts[:, 4:6] = rng.uniform(-20.0, 20.0, (n, 2))
    pts[:, 6:] = rng.standard_normal((n, 2))
    pts[:6, :2] = [[0.0, 0.0], [np.pi / 2, -np.pi / 2], [1e5, -1e5], [2.0e6, 0.3], [np.nan, 0.1], [0.2, np.inf]]
    ref = _run(lib, 1, pts)
    got = _run(lib, w, pts)
    assert np.isfinite(ref[6:]).all() and np.isnan(ref[3:6, 18:]).any(1).all()   # beyond the trig domain: NaN, as the device
    assert got.tobytes() == ref.tobytes()
