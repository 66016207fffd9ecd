"""Python binding of the mmpc C-ABI (include/mmpc.h) -- MI355X batched nonlinear MPC.

This is a thin ctypes layer over ``lib/libmmpc.so``; every compute call runs the HIP
kernels on the GPU.  There is no CPU fallback: if the library or a GPU is missing the
calls raise ``MmpcError``.

Reference mapping (mahi-mpc):
  Solver(...)            ~ ModelControl::load_model      (src/Mahi/Mpc/ModelControl.cpp:21-73)
  Solver.solve_batch*    ~ m_solver(m_solver_args)       (src/Mahi/Mpc/ModelControl.cpp:159), batched
  Solver.linearize*      ~ <name>_get_A/_get_B/_get_x_dot_init externals (ModelGenerator.cpp:51-53)
  write_model_json       ~ ModelGenerator::save_param_file (ModelGenerator.cpp:261-270)
"""
from __future__ import annotations

import ctypes as C
import json
import os
import re

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)                      # mahi-mpc_amd/
REPO = os.path.dirname(ROOT)
LIB_PATH = os.environ.get("MMPC_LIB_PATH") or os.path.join(ROOT, "lib", "libmmpc.so")
HEADER_PATH = os.path.join(REPO, "include", "mmpc.h")

OK = 0
STATUS = {0: "converged", 1: "max_iter", 2: "linesearch_failed", 3: "nonfinite",
          4: "factorization_failed", 5: "bounds_violated"}
STATUS_CONVERGED, STATUS_MAX_ITER, STATUS_LINESEARCH_FAILED = 0, 1, 2
STATUS_NONFINITE, STATUS_FACTORIZATION_FAILED, STATUS_BOUNDS_VIOLATED = 3, 4, 5
ERR = {-1: "invalid_arg", -2: "io", -3: "parse", -4: "unsupported", -5: "hip", -6: "no_device"}


class MmpcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mmpc error {code} ({ERR.get(code, '?')}): {msg}")
        self.code = code


KKT_AUTO, KKT_CONDENSED, KKT_RICCATI, KKT_RICCATI_GROUP = 0, 1, 2, 3
INIT_AS_GIVEN, INIT_HOLD_X0, INIT_ZERO = 0, 1, 2
HESSIAN_AUTO, HESSIAN_GAUSS_NEWTON, HESSIAN_EXACT = 0, 1, 2
# barrier rule of state-bounded solves (enum mmpc_barrier_rule): IPOPT's monotone rule, or Mehrotra's
# predictor-corrector (16-lane solver, nonlinear mode; include/mmpc.h)
BARRIER_MONOTONE, BARRIER_MEHROTRA = 0, 1
# kernel of the feedback-gain sweep (enum mmpc_gain_kernel) and its per-instance status
GAIN_KERNEL_AUTO, GAIN_KERNEL_LANE, GAIN_KERNEL_GROUP = 0, 1, 2
GAIN_OK, GAIN_GAUSS_NEWTON_FALLBACK, GAIN_FAILED = 0, 1, 2
# per-instance status of the solve VJP (mmpc_solve_vjp_batch): the same three values
VJP_OK, VJP_GAUSS_NEWTON_FALLBACK, VJP_FAILED = 0, 1, 2
# and of the solve JVP (mmpc_solve_jvp_batch)
JVP_OK, JVP_GAUSS_NEWTON_FALLBACK, JVP_FAILED = 0, 1, 2
# and of the real-time iteration calls (mmpc_rti_prepare_batch / mmpc_rti_feedback_batch)
RTI_OK, RTI_GAUSS_NEWTON_FALLBACK, RTI_FAILED = 0, 1, 2
MODEL_TWO_LINK_ARM, MODEL_EXO_ARM, MODEL_USER = 0, 1, 2
USER_LIB_DIR = os.path.join(ROOT, "lib", "user")
BUILTIN_MODELS = ("two_link_arm", "double_pendulum", "exo_arm", "exo")  # "mmpc_model" names libmmpc.so serves   # models generated from SX by ModelGenerator (make -C host user)


class Opts(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("device", C.c_int32), ("tol_grad", C.c_double),
                ("tol_defect", C.c_double), ("kkt_solver", C.c_int32), ("factor_fp32", C.c_int32),
                ("init_states", C.c_int32), ("hessian", C.c_int32), ("tail_cap", C.c_int32),
                ("tail_wave_max", C.c_int32), ("tail_rounds", C.c_int32)]


class ModelInfo(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("model_id", C.c_int32), ("num_x", C.c_int32), ("num_u", C.c_int32),
                ("num_shooting_nodes", C.c_int32), ("num_v", C.c_int32), ("num_g", C.c_int32),
                ("is_linear", C.c_int32), ("step_size", C.c_double), ("timespan_us", C.c_int64),
                ("step_size_us", C.c_int64), ("u_min", C.c_double * 16), ("u_max", C.c_double * 16),
                ("x_min", C.c_double * 16), ("x_max", C.c_double * 16)]


_libs = {}
_vp = C.c_void_p


def build(force: bool = False) -> str:
    """Compile lib/libmmpc.so for gfx950 with hipcc (make -C mahi-mpc_amd)."""
    import subprocess
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT], check=True)
    return LIB_PATH


def header_functions(path: str = HEADER_PATH):
    """Names of every function declared in include/mmpc.h."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mmpc_\w+)\s*\(", text)))


def lib(path: str | None = None):
    """The C-ABI library: libmmpc.so (built-in models) or a model's generated <name>.so (same ABI)."""
    path = os.path.abspath(path or LIB_PATH)
    if path not in _libs:
        if not os.path.exists(path):
            raise MmpcError(-2, f"{path} not built (run make -C mahi-mpc_amd)")
        # PyTorch-ROCm ships its own HIP runtime: if libmmpc's initialises first, torch later sees no GPU
        # (observed on the MI355X box), so torch -- when present -- initialises before the library is loaded
        try:
            import torch
            torch.cuda.is_available()
        except ImportError:
            pass
        L = C.CDLL(path)  # RTLD_LOCAL: each model library keeps its own kernels (linked with -Bsymbolic)
        L.mmpc_abi_version.restype = C.c_int
        L.mmpc_default_opts.argtypes = [C.POINTER(Opts)]
        L.mmpc_create.argtypes = [C.c_char_p, C.POINTER(Opts), C.POINTER(_vp)]
        L.mmpc_create_from_json.argtypes = [C.c_char_p, C.POINTER(Opts), C.POINTER(_vp)]
        L.mmpc_destroy.argtypes = [_vp]
        L.mmpc_get_model_info.argtypes = [_vp, C.POINTER(ModelInfo)]
        L.mmpc_set_opts.argtypes = [_vp, C.POINTER(Opts)]
        L.mmpc_reserve_workspace.argtypes = [_vp, C.c_int64, C.POINTER(C.c_uint64)]
        L.mmpc_solve_batch.argtypes = [_vp, C.c_int64] + [_vp] * 4 + [C.c_int64] + [_vp] * 7
        L.mmpc_solve_batch_host.argtypes = [_vp, C.c_int64] + [_vp] * 4 + [C.c_int64] + [_vp] * 6
        L.mmpc_solve_batch_u0.argtypes = [_vp, C.c_int64] + [_vp] * 4 + [C.c_int64] + [_vp] * 8
        # per-instance control bounds: the signatures above plus bounds_stride after u_ub
        L.mmpc_solve_batch_bounds.argtypes = [_vp, C.c_int64] + [_vp] * 4 + [C.c_int64, _vp, _vp, C.c_int64] + [_vp] * 6
        L.mmpc_solve_batch_host_bounds.argtypes = ([_vp, C.c_int64] + [_vp] * 4 + [C.c_int64, _vp, _vp, C.c_int64]
                                                   + [_vp] * 4)
        L.mmpc_multi_solve_batch_host_bounds.argtypes = L.mmpc_solve_batch_host_bounds.argtypes
        L.mmpc_multi_solve_batch_rccl_bounds.argtypes = ([_vp, C.c_int64] + [_vp] * 4 + [C.c_int64, _vp, _vp, C.c_int64]
                                                         + [_vp] * 5)
        # committed controls: the *_bounds signatures plus (u_pin, n_pin) after bounds_stride
        _pin = [_vp, C.c_int64] + [_vp] * 4 + [C.c_int64, _vp, _vp, C.c_int64, _vp, C.c_int32]
        L.mmpc_solve_batch_pinned.argtypes = _pin + [_vp] * 6
        L.mmpc_solve_batch_host_pinned.argtypes = _pin + [_vp] * 4
        L.mmpc_multi_solve_batch_host_pinned.argtypes = _pin + [_vp] * 4
        # feedback gains: (V, u_prev, traj, weights), weights_stride, (u_lb, u_ub), bounds_stride, n_pin, n_gain,
        # hessian, kernel, (G_out, gain_status[, stream])
        _gain = ([_vp, C.c_int64] + [_vp] * 4 + [C.c_int64, _vp, _vp, C.c_int64] + [C.c_int32] * 4)
        L.mmpc_feedback_gains_batch.argtypes = _gain + [_vp] * 3
        L.mmpc_feedback_gains_batch_host.argtypes = _gain + [_vp] * 2
        # solve VJP: (V, u_prev, traj, weights), weights_stride, (u_lb, u_ub), bounds_stride, n_pin, V_bar, hessian,
        # (x0_bar, u_prev_bar, traj_bar, weights_bar, adj_V, vjp_status[, workspace, workspace_bytes, stream])
        _vjp = ([_vp, C.c_int64] + [_vp] * 4 + [C.c_int64, _vp, _vp, C.c_int64, C.c_int32, _vp, C.c_int32] + [_vp] * 6)
        L.mmpc_solve_vjp_batch.argtypes = _vjp + [_vp, C.c_uint64, _vp]
        L.mmpc_solve_vjp_batch_host.argtypes = _vjp
        L.mmpc_solve_vjp_workspace_bytes.argtypes = [_vp, C.c_int64, C.POINTER(C.c_uint64)]
        # solve JVP: (V, u_prev, traj, weights), weights_stride, (u_lb, u_ub), bounds_stride, n_pin, (dx0, du_prev,
        # dtraj, dweights), hessian, (dV, du0, jvp_status[, workspace, workspace_bytes, stream])
        _jvp = ([_vp, C.c_int64] + [_vp] * 4 + [C.c_int64, _vp, _vp, C.c_int64, C.c_int32] + [_vp] * 4 + [C.c_int32]
                + [_vp] * 3)
        L.mmpc_solve_jvp_batch.argtypes = _jvp + [_vp, C.c_uint64, _vp]
        L.mmpc_solve_jvp_batch_host.argtypes = _jvp
        L.mmpc_solve_jvp_workspace_bytes.argtypes = [_vp, C.c_int64, C.POINTER(C.c_uint64)]
        # real-time iteration.  prepare: (V, u_prev, traj, weights), weights_stride, (u_lb, u_ub), bounds_stride, n_pin,
        # hessian, prep_status, workspace, workspace_bytes, stream;  feedback: x0_meas, (u_lb, u_ub), bounds_stride,
        # (V_inout, u0_out, step_inf, status), workspace, workspace_bytes, stream;  host: V_inout, x0_meas, (u_prev, traj,
        # weights), weights_stride, (u_lb, u_ub), bounds_stride, n_pin, hessian, (u0_out, step_inf, status)
        L.mmpc_rti_workspace_bytes.argtypes = [_vp, C.c_int64, C.POINTER(C.c_uint64)]
        L.mmpc_rti_prepare_batch.argtypes = ([_vp, C.c_int64] + [_vp] * 4 + [C.c_int64, _vp, _vp, C.c_int64, C.c_int32,
                                                                             C.c_int32, _vp, _vp, C.c_uint64, _vp])
        L.mmpc_rti_feedback_batch.argtypes = [_vp, C.c_int64, _vp, _vp, _vp, C.c_int64] + [_vp] * 5 + [C.c_uint64, _vp]
        L.mmpc_rti_step_batch_host.argtypes = ([_vp, C.c_int64] + [_vp] * 5 + [C.c_int64, _vp, _vp, C.c_int64, C.c_int32,
                                                                               C.c_int32] + [_vp] * 3)
        # the shift between two ticks: V_in, n_shift, V_out, u_prev_out, stream
        L.mmpc_rti_shift_batch.argtypes = [_vp, C.c_int64, _vp, C.c_int32, _vp, _vp, _vp]
        L.mmpc_host_alloc.argtypes = [C.c_uint64, C.POINTER(_vp)]
        L.mmpc_host_free.argtypes = [_vp]
        L.mmpc_linearize_batch.argtypes = [_vp, C.c_int64] + [_vp] * 6
        L.mmpc_linearize_batch_host.argtypes = [_vp, C.c_int64] + [_vp] * 5
        L.mmpc_nlp_eval_batch.argtypes = [_vp, C.c_int64] + [_vp] * 4 + [C.c_int64] + [_vp] * 3
        L.mmpc_synth_batch.argtypes = [_vp, C.c_uint64, C.c_int64, C.c_int64] + [_vp] * 4
        L.mmpc_nlp_derivs_batch.argtypes = [_vp, C.c_int64] + [_vp] * 4 + [C.c_int64] + [_vp] * 4
        L.mmpc_nlp_hess_batch.argtypes = [_vp, C.c_int64] + [_vp] * 4 + [C.c_int64, C.c_double, _vp, _vp, _vp]
        L.mmpc_shard.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.mmpc_multi_create.argtypes = [C.c_char_p, C.POINTER(Opts), C.POINTER(C.c_int32), C.c_int32, C.POINTER(_vp)]
        L.mmpc_multi_destroy.argtypes = [_vp]
        L.mmpc_multi_num_devices.argtypes = [_vp, C.POINTER(C.c_int32)]
        L.mmpc_multi_handle.argtypes = [_vp, C.c_int32, C.POINTER(_vp)]
        L.mmpc_multi_solve_batch_host.argtypes = [_vp, C.c_int64] + [_vp] * 4 + [C.c_int64] + [_vp] * 6
        L.mmpc_multi_solve_batch_rccl.argtypes = [_vp, C.c_int64] + [_vp] * 4 + [C.c_int64] + [_vp] * 7
        L.mmpc_rccl_version.argtypes = [C.POINTER(C.c_int32)]
        L.mmpc_resolve_kkt_solver.argtypes = [_vp, C.c_int64, C.POINTER(C.c_int32)]
        L.mmpc_resolve_hessian.argtypes = [_vp, C.c_int64, C.c_int32, C.POINTER(C.c_int32)]
        L.mmpc_set_state_bounds.argtypes = [_vp, _vp, _vp]
        L.mmpc_get_state_bounds.argtypes = [_vp, _vp, _vp]
        L.mmpc_set_barrier_rule.argtypes = [_vp, C.c_int32]
        L.mmpc_get_barrier_rule.argtypes = [_vp, C.POINTER(C.c_int32)]
        _pd = C.POINTER(C.c_double)
        L.mmpc_sensitivity_barrier_default.argtypes = [_pd, _pd]
        L.mmpc_set_sensitivity_barrier.argtypes = [_vp, C.c_double, C.c_double]
        L.mmpc_get_sensitivity_barrier.argtypes = [_vp, _pd, _pd]
        L.mmpc_status_string.argtypes = [C.c_int32]
        L.mmpc_status_string.restype = C.c_char_p
        L.mmpc_last_error.restype = C.c_char_p
        _libs[path] = L
    return _libs[path]


def model_library(model_json: str) -> str:
    """Library serving the model of <name>.json: for a model generated from SX expressions ("mmpc_model" naming
    no built-in model) its dll_filepath, resolved against the JSON's directory as ModelControl does; else
    libmmpc.so (built-in models, and reference-written JSONs whose dll_filepath is a CasADi NLP library)."""
    try:
        with open(model_json) as fh:
            m = json.load(fh)
    except (OSError, ValueError):
        return LIB_PATH  # mmpc_create reports the I/O or parse error
    m = m.get("model", m) if isinstance(m, dict) else {}
    dll = m.get("dll_filepath") or ""
    if m.get("mmpc_model") in (None, *BUILTIN_MODELS) or not dll or os.path.basename(dll) == "libmmpc.so":
        return LIB_PATH
    cands = [dll] if os.path.isabs(dll) else [os.path.join(os.path.dirname(os.path.abspath(model_json)), dll), dll]
    for c in cands:
        if os.path.exists(c):
            return os.path.abspath(c)
    raise MmpcError(-2, f"model library {dll} of {model_json} not found")


def _check(rc, L=None):
    if rc != OK:
        raise MmpcError(rc, (L or lib()).mmpc_last_error().decode())


def default_opts() -> Opts:
    o = Opts()
    lib().mmpc_default_opts(C.byref(o))
    return o


def write_model_json(path, name, num_x, num_u, step_size_us, num_shooting_nodes, is_linear=False,
                     u_min=None, u_max=None, x_min=None, x_max=None, dll_filepath="", extra=None, model=None):
    """Write <name>.json exactly as ModelGenerator::save_param_file does (ModelParameters.cpp:37-50),
    including the +-10e30 defaults of the ModelParameters constructor (ModelParameters.cpp:14-24).
    ``model`` ("two_link_arm" / "exo_arm") adds the "mmpc_model" key naming the built-in dynamics."""
    def dflt(v, n, s):
        return list(v) if v is not None else [s * 10e30] * n
    m = {"name": name, "timespan": int(step_size_us) * int(num_shooting_nodes), "step_size": int(step_size_us),
         "num_x": num_x, "num_u": num_u, "num_shooting_nodes": num_shooting_nodes,
         "x_min": dflt(x_min, num_x, -1), "u_min": dflt(u_min, num_u, -1),
         "x_max": dflt(x_max, num_x, 1), "u_max": dflt(u_max, num_u, 1),
         "dll_filepath": dll_filepath, "is_linear": bool(is_linear)}
    if model:
        m["mmpc_model"] = model
    if extra:
        m.update(extra)
    with open(path, "w") as fh:
        json.dump({"model": m}, fh)
    return path


def _ptr(a):
    """device/host pointer of a torch tensor, numpy array, int address or None."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    if isinstance(a, np.ndarray):
        assert a.flags.c_contiguous
        return a.ctypes.data
    raise TypeError(type(a))


class HostBuffer:
    """Pinned host memory mapped into the devices' address space (mmpc_host_alloc): a solve kernel stores its
    per-tick results (u_0*, status, iters) straight into it -- on the host once the stream has completed.
    ``view(offset, dtype, count)`` gives numpy views; pass them (or their addresses) as solve outputs."""

    def __init__(self, nbytes: int, path: str | None = None):
        self._L = lib(path)
        p = _vp()
        rc = self._L.mmpc_host_alloc(int(nbytes), C.byref(p))
        if rc != 0:
            raise MmpcError(rc, self._L.mmpc_last_error().decode())
        self.ptr = p.value or 0
        self.nbytes = int(nbytes)
        self._buf = (C.c_char * self.nbytes).from_address(self.ptr) if self.nbytes else None
        if self.nbytes:   # hipHostMalloc does not zero: rows a ragged shard never writes must compare equal
            C.memset(self.ptr, 0, self.nbytes)

    def view(self, offset: int, dtype, count: int) -> np.ndarray:
        dt = np.dtype(dtype)
        assert offset % dt.itemsize == 0 and offset + count * dt.itemsize <= self.nbytes
        return np.frombuffer(self._buf, dtype=dt, count=count, offset=offset)

    def close(self):
        if self.ptr:
            self._buf = None
            self._L.mmpc_host_free(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _host_bounds(u_lb, u_ub, B, nu):
    """(lb, ub, bounds_stride) of host control bounds: [nu] rows are shared (stride 0), [B, nu] arrays are per
    instance (stride nu); when only one of the two is 2-D the other is repeated, since one stride serves both."""
    lb = None if u_lb is None else _f64(u_lb)
    ub = None if u_ub is None else _f64(u_ub)
    if not any(a is not None and a.ndim == 2 for a in (lb, ub)):
        return lb, ub, 0
    def rows(a):
        if a is None:
            return None
        if a.ndim == 1:
            a = np.broadcast_to(a.reshape(1, nu), (B, nu))
        if a.shape != (B, nu):
            raise ValueError(f"control bounds of shape {a.shape}: expected ({nu},) or ({B}, {nu})")
        return np.ascontiguousarray(a)
    return rows(lb), rows(ub), nu


def _host_pins(u_pin, B, nu, N):
    """(pins, n_pin) of host committed controls: None pins nothing; otherwise a [B, m, nu] array, m from its shape
    (0 <= m <= N - 1).  A wrong shape raises ValueError before the library is called."""
    if u_pin is None:
        return None, 0
    a = np.asarray(u_pin, dtype=np.float64)
    if a.ndim != 3 or a.shape[0] != B or a.shape[2] != nu:
        raise ValueError(f"u_pin of shape {a.shape}: expected ({B}, m, {nu})")
    m = a.shape[1]
    if m > N - 1:
        raise ValueError(f"u_pin pins {m} controls: at most N - 1 = {N - 1}")
    return (np.ascontiguousarray(a), m) if m else (None, 0)


class Solver:
    """One loaded model (the reference's ModelControl without the thread/bookkeeping)."""

    def __init__(self, model_json=None, json_text=None, max_iter=None, tol_grad=None, tol_defect=None,
                 device=None, kkt_solver=None, factor_fp32=None, library=None, init_states=None, hessian=None,
                 tail_cap=None, tail_wave_max=None, tail_rounds=None, barrier_rule=None, sensitivity_barrier=None):
        self._L = L = lib(library or (model_library(model_json) if model_json is not None else None))
        o = Opts()
        L.mmpc_default_opts(C.byref(o))
        if kkt_solver is not None:
            o.kkt_solver = kkt_solver
        if factor_fp32 is not None:
            o.factor_fp32 = int(factor_fp32)
        if init_states is not None:
            o.init_states = int(init_states)
        if hessian is not None:
            o.hessian = int(hessian)
        if tail_cap is not None:      # the lane solver's iteration-tail hand-over (ABI 6; -1 = default, 0 = off)
            o.tail_cap = int(tail_cap)
        if tail_wave_max is not None:
            o.tail_wave_max = int(tail_wave_max)
        if tail_rounds is not None:
            o.tail_rounds = int(tail_rounds)
        if max_iter is not None:
            o.max_iter = max_iter
        if tol_grad is not None:
            o.tol_grad = tol_grad
        if tol_defect is not None:
            o.tol_defect = tol_defect
        if device is not None:
            o.device = device
        h = _vp()
        if json_text is not None:
            self._check(L.mmpc_create_from_json(json_text.encode(), C.byref(o), C.byref(h)))
        else:
            self._check(L.mmpc_create(os.fsencode(model_json), C.byref(o), C.byref(h)))
        self._h = h
        info = ModelInfo()
        self._check(L.mmpc_get_model_info(h, C.byref(info)))
        self.info = info
        self.nx, self.nu, self.N = info.num_x, info.num_u, info.num_shooting_nodes
        self.NV = info.num_v
        self.h = info.step_size
        if barrier_rule is not None:
            self.set_barrier_rule(barrier_rule)
        if sensitivity_barrier is not None:   # True: the library's defaults; a number: mu; a pair: (mu, sigma_cap)
            if sensitivity_barrier is True:
                self.set_sensitivity_barrier()
            elif sensitivity_barrier is False:
                self.set_sensitivity_barrier(mu=0)
            elif np.ndim(sensitivity_barrier) == 0:
                self.set_sensitivity_barrier(mu=sensitivity_barrier)
            else:
                self.set_sensitivity_barrier(*sensitivity_barrier)

    def _check(self, rc):
        _check(rc, self._L)

    def reserve_workspace(self, B) -> int:
        """Pre-allocate the Riccati solver workspace for up to B instances; returns its size in bytes."""
        n = C.c_uint64(0)
        self._check(self._L.mmpc_reserve_workspace(self._h, B, C.byref(n)))
        return int(n.value)

    def close(self):
        if getattr(self, "_h", None):
            self._L.mmpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- device-pointer API (torch tensors on the GPU or raw addresses) ----
    def solve_batch(self, B, x0, u_prev, traj, weights, V, status=None, iters=None, kkt=None,
                    weights_stride=0, u_lb=None, u_ub=None, stream=None, u0=None, bounds_stride=0, u_pin=None,
                    n_pin=0):
        """Device-pointer solve (stream-ordered).  u0: optional [B][nu] output of u_0* (mmpc_solve_batch_u0);
        u0 / status / iters may be HostBuffer views (results stored by the kernel straight into host memory).
        bounds_stride: 0 = u_lb / u_ub are [nu], shared; >= nu = instance b's row starts at b * bounds_stride
        (mmpc_solve_batch_bounds).  u_pin, n_pin: committed controls, device [B][n_pin][nu] -- the first n_pin
        controls of every instance are fixed to them (mmpc_solve_batch_pinned; n_pin = 0 pins nothing)."""
        if n_pin:
            self._check(self._L.mmpc_solve_batch_pinned(self._h, B, _ptr(x0), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                                        weights_stride, _ptr(u_lb), _ptr(u_ub), int(bounds_stride),
                                                        _ptr(u_pin), int(n_pin), _ptr(V), _ptr(status), _ptr(iters),
                                                        _ptr(kkt), _ptr(u0), stream))
        elif bounds_stride:
            self._check(self._L.mmpc_solve_batch_bounds(self._h, B, _ptr(x0), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                                        weights_stride, _ptr(u_lb), _ptr(u_ub), int(bounds_stride),
                                                        _ptr(V), _ptr(status), _ptr(iters), _ptr(kkt), _ptr(u0),
                                                        stream))
        elif u0 is None:
            self._check(self._L.mmpc_solve_batch(self._h, B, _ptr(x0), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                                 weights_stride, _ptr(u_lb), _ptr(u_ub), _ptr(V), _ptr(status),
                                                 _ptr(iters), _ptr(kkt), stream))
        else:
            self._check(self._L.mmpc_solve_batch_u0(self._h, B, _ptr(x0), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                                    weights_stride, _ptr(u_lb), _ptr(u_ub), _ptr(V), _ptr(status),
                                                    _ptr(iters), _ptr(kkt), _ptr(u0), stream))

    def synth(self, seed, first_index, B, x0, u_prev, traj, stream=None):
        self._check(self._L.mmpc_synth_batch(self._h, seed, first_index, B, _ptr(x0), _ptr(u_prev), _ptr(traj), stream))

    def nlp_eval(self, B, V, u_prev, traj, weights, J, defect_inf, weights_stride=0, stream=None):
        self._check(self._L.mmpc_nlp_eval_batch(self._h, B, _ptr(V), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                         weights_stride, _ptr(J), _ptr(defect_inf), stream))

    def nlp_derivs(self, B, V, u_prev, traj, weights, J=None, grad=None, jac_blocks=None, weights_stride=0,
                   stream=None):
        """J, dJ/dV and the defect-Jacobian stage blocks at V (device pointers; nlp_grad_f / nlp_jac_g)."""
        self._check(self._L.mmpc_nlp_derivs_batch(self._h, B, _ptr(V), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                                  weights_stride, _ptr(J), _ptr(grad), _ptr(jac_blocks), stream))

    def nlp_hess(self, B, V, u_prev, traj, weights, lam_f, lam_g, blocks, weights_stride=0, stream=None):
        """nlp_hess_l stage blocks [B][N][K][K] of lam_f J + lam_g^T g at V (device pointers)."""
        self._check(self._L.mmpc_nlp_hess_batch(self._h, B, _ptr(V), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                                weights_stride, float(lam_f), _ptr(lam_g), _ptr(blocks), stream))

    def linearize(self, B, x, u, A, Bm, xdot, stream=None):
        self._check(self._L.mmpc_linearize_batch(self._h, B, _ptr(x), _ptr(u), _ptr(A), _ptr(Bm), _ptr(xdot), stream))

    # ---- host (numpy) API, synchronous ----
    def solve_batch_host(self, x0, u_prev, traj, weights, V=None, u_lb=None, u_ub=None, u_pin=None):
        """u_pin: committed controls [B, m, nu] (m from the shape): the first m controls of every instance are
        fixed to them (mmpc_solve_batch_host_pinned); None pins nothing."""
        nx, nu, N, NV = self.nx, self.nu, self.N, self.NV
        x0 = _f64(x0, (-1, nx))
        B = x0.shape[0]
        pin, m = _host_pins(u_pin, B, nu, N)
        u_prev = _f64(u_prev, (B, nu))
        traj = _f64(traj, (B, N, nx))
        weights = _f64(weights)
        ws = 0 if weights.ndim == 1 else weights.shape[-1]
        V = np.zeros((B, NV)) if V is None else _f64(V, (B, NV)).copy()
        st = np.zeros(B, np.int32)
        it = np.zeros(B, np.int32)
        kkt = np.zeros(B)
        lb, ub, bs = _host_bounds(u_lb, u_ub, B, nu)   # [nu] shared, or [B, nu] per instance
        if m:
            self._check(self._L.mmpc_solve_batch_host_pinned(self._h, B, _ptr(x0), _ptr(u_prev), _ptr(traj),
                                                             _ptr(weights), ws, _ptr(lb), _ptr(ub), bs, _ptr(pin), m,
                                                             _ptr(V), _ptr(st), _ptr(it), _ptr(kkt)))
            return dict(V=V, status=st, iters=it, kkt=kkt)
        self._check(self._L.mmpc_solve_batch_host_bounds(self._h, B, _ptr(x0), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                                         ws, _ptr(lb), _ptr(ub), bs, _ptr(V), _ptr(st), _ptr(it),
                                                         _ptr(kkt)))
        return dict(V=V, status=st, iters=it, kkt=kkt)

    def feedback_gains(self, B, V, u_prev, traj, weights, G=None, gain_status=None, weights_stride=0, u_lb=None,
                       u_ub=None, bounds_stride=0, n_pin=0, n_gain=None, hessian=HESSIAN_AUTO, kernel=GAIN_KERNEL_AUTO,
                       stream=None):
        """Feedback gains G_k = d u_k* / d(x_k, u_{k-1}) along the plan V (mmpc_feedback_gains_batch; device
        pointers, stream-ordered, no allocation by the library).  Returns (G, gain_status): G [B, n_gain, nu, nx + nu]
        (n_gain defaults to N), gain_status [B] int32 (0 as asked, 1 Gauss-Newton fallback, 2 failed: gains 0).  G and
        gain_status are torch tensors on V's device unless given (tensors or raw addresses, returned as given)."""
        n_gain = self.N if n_gain is None else int(n_gain)
        if G is None or gain_status is None:
            import torch
            if G is None:
                G = torch.empty((B, n_gain, self.nu, self.nx + self.nu), dtype=torch.float64, device=V.device)
            if gain_status is None:
                gain_status = torch.empty((B,), dtype=torch.int32, device=V.device)
        self._check(self._L.mmpc_feedback_gains_batch(self._h, B, _ptr(V), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                                      weights_stride, _ptr(u_lb), _ptr(u_ub), int(bounds_stride),
                                                      int(n_pin), n_gain, int(hessian), int(kernel), _ptr(G),
                                                      _ptr(gain_status), stream))
        return G, gain_status

    def feedback_gains_host(self, V, u_prev, traj, weights, u_lb=None, u_ub=None, n_pin=0, n_gain=None,
                            hessian=HESSIAN_AUTO, kernel=GAIN_KERNEL_AUTO):
        """feedback_gains for numpy arrays, synchronous (mmpc_feedback_gains_batch_host); u_lb / u_ub [nu] shared or
        [B, nu] per instance.  Returns (G [B, n_gain, nu, nx + nu], gain_status [B])."""
        nx, nu, N, NV = self.nx, self.nu, self.N, self.NV
        V = _f64(V, (-1, NV))
        B = V.shape[0]
        u_prev, traj, weights = _f64(u_prev, (B, nu)), _f64(traj, (B, N, nx)), _f64(weights)
        ws = 0 if weights.ndim == 1 else weights.shape[-1]
        n_gain = N if n_gain is None else int(n_gain)
        lb, ub, bs = _host_bounds(u_lb, u_ub, B, nu)
        G = np.zeros((B, max(n_gain, 0), nu, nx + nu))
        st = np.full(B, -1, np.int32)
        self._check(self._L.mmpc_feedback_gains_batch_host(self._h, B, _ptr(V), _ptr(u_prev), _ptr(traj),
                                                           _ptr(weights), ws, _ptr(lb), _ptr(ub), bs, int(n_pin),
                                                           n_gain, int(hessian), int(kernel), _ptr(G), _ptr(st)))
        return G, st

    def solve_vjp_workspace_bytes(self, B) -> int:
        """Bytes of the record workspace a full solve_vjp of B instances needs (mmpc_solve_vjp_workspace_bytes)."""
        n = C.c_uint64(0)
        self._check(self._L.mmpc_solve_vjp_workspace_bytes(self._h, B, C.byref(n)))
        return int(n.value)

    def solve_vjp(self, B, V, u_prev, traj, weights, V_bar, x0_bar=None, u_prev_bar=None, traj_bar=None,
                  weights_bar=None, adj_V=None, vjp_status=None, workspace=None, workspace_bytes=None,
                  weights_stride=0, u_lb=None, u_ub=None, bounds_stride=0, n_pin=0, hessian=HESSIAN_AUTO,
                  backward_only=False, stream=None):
        """Reverse-mode product of the solve at V (mmpc_solve_vjp_batch; device tensors, one stream-ordered launch):
        theta_bar = (d V* / d theta)^T V_bar for theta = x0, u_prev, traj and the weights.  Returns a dict with x0_bar
        [B, nx], u_prev_bar [B, nu], traj_bar [B, N, nx], weights_bar [B, nx + 2 nu] (per instance: sum the rows for
        shared weights), adj_V [B, NV] and vjp_status [B] int32 (0 as asked, 1 Gauss-Newton fallback, 2 failed: rows
        0).  Outputs and the workspace are torch tensors on V's device unless given (tensors or raw addresses, used as
        given; a raw workspace address needs workspace_bytes).  backward_only: only x0_bar, u_prev_bar and vjp_status
        -- no forward sweep, no workspace; traj_bar, weights_bar and adj_V are then None."""
        nx, nu, N, NV = self.nx, self.nu, self.N, self.NV
        out = dict(x0_bar=x0_bar, u_prev_bar=u_prev_bar, traj_bar=traj_bar, weights_bar=weights_bar, adj_V=adj_V,
                   vjp_status=vjp_status)
        shapes = dict(x0_bar=(B, nx), u_prev_bar=(B, nu), traj_bar=(B, N, nx), weights_bar=(B, nx + 2 * nu),
                      adj_V=(B, NV), vjp_status=(B,))
        fwd = ("traj_bar", "weights_bar", "adj_V")
        if backward_only and any(out[k] is not None for k in fwd):
            raise ValueError("backward_only takes no traj_bar, weights_bar or adj_V")
        want = [k for k in out if out[k] is None and not (backward_only and k in fwd)]
        if want or (workspace is None and not backward_only):
            import torch
            for k in want:
                out[k] = torch.empty(shapes[k], dtype=torch.int32 if k == "vjp_status" else torch.float64,
                                     device=V.device)
            if workspace is None and not backward_only:
                workspace = torch.empty((max(self.solve_vjp_workspace_bytes(B), 8) // 8,), dtype=torch.float64,
                                        device=V.device)
        if workspace_bytes is None:
            workspace_bytes = workspace.numel() * workspace.element_size() if hasattr(workspace, "numel") else 0
        self._check(self._L.mmpc_solve_vjp_batch(self._h, B, _ptr(V), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                                 weights_stride, _ptr(u_lb), _ptr(u_ub), int(bounds_stride),
                                                 int(n_pin), _ptr(V_bar), int(hessian), _ptr(out["x0_bar"]),
                                                 _ptr(out["u_prev_bar"]), _ptr(out["traj_bar"]),
                                                 _ptr(out["weights_bar"]), _ptr(out["adj_V"]),
                                                 _ptr(out["vjp_status"]), _ptr(workspace), int(workspace_bytes),
                                                 stream))
        return out

    def solve_vjp_host(self, V, u_prev, traj, weights, V_bar, u_lb=None, u_ub=None, n_pin=0, hessian=HESSIAN_AUTO,
                       backward_only=False):
        """solve_vjp for numpy arrays, synchronous (mmpc_solve_vjp_batch_host; the library brings the workspace);
        u_lb / u_ub [nu] shared or [B, nu] per instance.  Returns a dict of numpy arrays with solve_vjp's keys."""
        nx, nu, N, NV = self.nx, self.nu, self.N, self.NV
        V = _f64(V, (-1, NV))
        B = V.shape[0]
        u_prev, traj, weights, V_bar = _f64(u_prev, (B, nu)), _f64(traj, (B, N, nx)), _f64(weights), _f64(V_bar, (B, NV))
        ws = 0 if weights.ndim == 1 else weights.shape[-1]
        lb, ub, bs = _host_bounds(u_lb, u_ub, B, nu)
        out = dict(x0_bar=np.zeros((B, nx)), u_prev_bar=np.zeros((B, nu)),
                   traj_bar=None if backward_only else np.zeros((B, N, nx)),
                   weights_bar=None if backward_only else np.zeros((B, nx + 2 * nu)),
                   adj_V=None if backward_only else np.zeros((B, NV)), vjp_status=np.full(B, -1, np.int32))
        self._check(self._L.mmpc_solve_vjp_batch_host(self._h, B, _ptr(V), _ptr(u_prev), _ptr(traj), _ptr(weights), ws,
                                                      _ptr(lb), _ptr(ub), bs, int(n_pin), _ptr(V_bar), int(hessian),
                                                      _ptr(out["x0_bar"]), _ptr(out["u_prev_bar"]),
                                                      _ptr(out["traj_bar"]), _ptr(out["weights_bar"]),
                                                      _ptr(out["adj_V"]), _ptr(out["vjp_status"])))
        return out

    def solve_jvp_workspace_bytes(self, B) -> int:
        """Bytes of the record workspace a full solve_jvp of B instances needs (mmpc_solve_jvp_workspace_bytes)."""
        n = C.c_uint64(0)
        self._check(self._L.mmpc_solve_jvp_workspace_bytes(self._h, B, C.byref(n)))
        return int(n.value)

    def solve_jvp(self, B, V, u_prev, traj, weights, dx0=None, du_prev=None, dtraj=None, dweights=None, dV=None,
                  du0=None, jvp_status=None, workspace=None, workspace_bytes=None, weights_stride=0, u_lb=None,
                  u_ub=None, bounds_stride=0, n_pin=0, hessian=HESSIAN_AUTO, forward_free=False, stream=None):
        """Forward-mode product of the solve at V (mmpc_solve_jvp_batch; device tensors, one stream-ordered launch):
        dV = (d V* / d theta) d theta for the tangents dx0 [B, nx], du_prev [B, nu], dtraj [B, N, nx] and dweights
        [B, nx + 2 nu] (None: zero; at least one is needed) -- V + dV is the plan updated to first order.  Returns a
        dict with dV [B, NV], du0 [B, nu] (the u_0 entries of dV) and jvp_status [B] int32 (0 as asked, 1 Gauss-Newton
        fallback, 2 failed: rows 0).  Outputs and the workspace are torch tensors on V's device unless given (tensors
        or raw addresses, used as given; a raw workspace address needs workspace_bytes).  forward_free: only du0 and
        jvp_status -- no forward sweep, no workspace; dV is then None."""
        nx, nu, NV = self.nx, self.nu, self.NV
        if forward_free and dV is not None:
            raise ValueError("forward_free takes no dV")
        out = dict(dV=dV, du0=du0, jvp_status=jvp_status)
        shapes = dict(dV=(B, NV), du0=(B, nu), jvp_status=(B,))
        want = [k for k in out if out[k] is None and not (forward_free and k == "dV")]
        if want or (workspace is None and not forward_free):
            import torch
            for k in want:
                out[k] = torch.empty(shapes[k], dtype=torch.int32 if k == "jvp_status" else torch.float64,
                                     device=V.device)
            if workspace is None and not forward_free:
                workspace = torch.empty((max(self.solve_jvp_workspace_bytes(B), 8) // 8,), dtype=torch.float64,
                                        device=V.device)
        if workspace_bytes is None:
            workspace_bytes = workspace.numel() * workspace.element_size() if hasattr(workspace, "numel") else 0
        self._check(self._L.mmpc_solve_jvp_batch(self._h, B, _ptr(V), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                                 weights_stride, _ptr(u_lb), _ptr(u_ub), int(bounds_stride),
                                                 int(n_pin), _ptr(dx0), _ptr(du_prev), _ptr(dtraj), _ptr(dweights),
                                                 int(hessian), _ptr(out["dV"]), _ptr(out["du0"]),
                                                 _ptr(out["jvp_status"]), _ptr(workspace), int(workspace_bytes),
                                                 stream))
        return out

    def solve_jvp_host(self, V, u_prev, traj, weights, dx0=None, du_prev=None, dtraj=None, dweights=None, u_lb=None,
                       u_ub=None, n_pin=0, hessian=HESSIAN_AUTO, forward_free=False):
        """solve_jvp for numpy arrays, synchronous (mmpc_solve_jvp_batch_host; the library brings the workspace);
        u_lb / u_ub [nu] shared or [B, nu] per instance.  Returns a dict of numpy arrays with solve_jvp's keys."""
        nx, nu, N, NV = self.nx, self.nu, self.N, self.NV
        V = _f64(V, (-1, NV))
        B = V.shape[0]
        u_prev, traj, weights = _f64(u_prev, (B, nu)), _f64(traj, (B, N, nx)), _f64(weights)
        opt = lambda t, shape: None if t is None else _f64(t, shape)  # noqa: E731
        dx0, du_prev, dtraj = opt(dx0, (B, nx)), opt(du_prev, (B, nu)), opt(dtraj, (B, N, nx))
        dweights = opt(dweights, (B, nx + 2 * nu))
        ws = 0 if weights.ndim == 1 else weights.shape[-1]
        lb, ub, bs = _host_bounds(u_lb, u_ub, B, nu)
        out = dict(dV=None if forward_free else np.zeros((B, NV)), du0=np.zeros((B, nu)),
                   jvp_status=np.full(B, -1, np.int32))
        self._check(self._L.mmpc_solve_jvp_batch_host(self._h, B, _ptr(V), _ptr(u_prev), _ptr(traj), _ptr(weights), ws,
                                                      _ptr(lb), _ptr(ub), bs, int(n_pin), _ptr(dx0), _ptr(du_prev),
                                                      _ptr(dtraj), _ptr(dweights), int(hessian), _ptr(out["dV"]),
                                                      _ptr(out["du0"]), _ptr(out["jvp_status"])))
        return out

    def rti_workspace_bytes(self, B) -> int:
        """Bytes of the workspace rti_prepare / rti_feedback of B instances need (mmpc_rti_workspace_bytes):
        ceil(B / 64) * 64 * ((N K (K + 1) + NV) * 8 + 4), K = nx + nu."""
        n = C.c_uint64(0)
        self._check(self._L.mmpc_rti_workspace_bytes(self._h, B, C.byref(n)))
        return int(n.value)

    def rti_prepare(self, B, V, u_prev, traj, weights, workspace=None, workspace_bytes=None, prep_status=None,
                    weights_stride=0, u_lb=None, u_ub=None, bounds_stride=0, n_pin=0, hessian=HESSIAN_AUTO,
                    stream=None):
        """Preparation of a real-time iteration at the plan V, which need not be a solution (mmpc_rti_prepare_batch;
        device tensors, one stream-ordered launch): linearisation, gradient, defects and the backward Riccati sweep,
        stored in the workspace for rti_feedback.  Returns a dict with workspace (a float64 torch tensor on V's device
        unless given; a raw address needs workspace_bytes) and prep_status [B] int32 (0 as asked, 1 Gauss-Newton
        fallback, 2 failed)."""
        if workspace is None or prep_status is None:
            import torch
            if workspace is None:
                workspace = torch.empty((max(self.rti_workspace_bytes(B), 8) // 8,), dtype=torch.float64,
                                        device=V.device)
            if prep_status is None:
                prep_status = torch.empty((B,), dtype=torch.int32, device=V.device)
        if workspace_bytes is None:
            workspace_bytes = workspace.numel() * workspace.element_size() if hasattr(workspace, "numel") else 0
        self._check(self._L.mmpc_rti_prepare_batch(self._h, B, _ptr(V), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                                   weights_stride, _ptr(u_lb), _ptr(u_ub), int(bounds_stride),
                                                   int(n_pin), int(hessian), _ptr(prep_status), _ptr(workspace),
                                                   int(workspace_bytes), stream))
        return dict(workspace=workspace, prep_status=prep_status)

    def rti_feedback(self, B, x0_meas, V, workspace, workspace_bytes=None, u0=None, step_inf=None, status=None,
                     u_lb=None, u_ub=None, bounds_stride=0, stream=None):
        """Feedback of a real-time iteration (mmpc_rti_feedback_batch; device tensors, one stream-ordered launch, no
        model inside): V, the plan rti_prepare was given, becomes V + dV in place with V[:, :nx] = x0_meas; u_lb / u_ub
        clamp the controls.  Returns a dict with V, u0 [B, nu] (the control to apply), step_inf [B] (max |dV|) and
        status [B] int32 (0 as asked, 1 Gauss-Newton fallback, 2 failed: V unchanged, u0 the plan's own, step_inf
        inf).  Outputs are torch tensors on V's device unless given (tensors or raw addresses, e.g. of HostBuffer
        memory, used as given)."""
        out = dict(u0=u0, step_inf=step_inf, status=status)
        shapes = dict(u0=(B, self.nu), step_inf=(B,), status=(B,))
        want = [k for k in out if out[k] is None]
        if want:
            import torch
            for k in want:
                out[k] = torch.empty(shapes[k], dtype=torch.int32 if k == "status" else torch.float64, device=V.device)
        if workspace_bytes is None:
            workspace_bytes = workspace.numel() * workspace.element_size() if hasattr(workspace, "numel") else 0
        self._check(self._L.mmpc_rti_feedback_batch(self._h, B, _ptr(x0_meas), _ptr(u_lb), _ptr(u_ub),
                                                    int(bounds_stride), _ptr(V), _ptr(out["u0"]),
                                                    _ptr(out["step_inf"]), _ptr(out["status"]), _ptr(workspace),
                                                    int(workspace_bytes), stream))
        out["V"] = V
        return out

    def rti_shift(self, B, V_in, n_shift=1, V_out=None, u_prev_out=None, stream=None):
        """The plans V_in [B, NV] moved n_shift stages earlier (mmpc_rti_shift_batch; device tensors, one stream-ordered
        launch, no workspace): the tail repeats the old u_{N-1} and rolls the states out with the model's Euler step.
        V_out may not be V_in.  Returns a dict with V and u_prev [B, nu] (the old u_{n_shift-1}; not written for
        n_shift = 0): torch tensors on V_in's device unless given (tensors or raw addresses, used as given)."""
        if V_out is None or u_prev_out is None:
            import torch
            if V_out is None:
                V_out = torch.empty((B, self.NV), dtype=torch.float64, device=V_in.device)
            if u_prev_out is None:
                u_prev_out = torch.zeros((B, self.nu), dtype=torch.float64, device=V_in.device)
        self._check(self._L.mmpc_rti_shift_batch(self._h, B, _ptr(V_in), int(n_shift), _ptr(V_out), _ptr(u_prev_out),
                                                 stream))
        return dict(V=V_out, u_prev=u_prev_out)

    def rti_step_host(self, V, x0_meas, u_prev, traj, weights, u_lb=None, u_ub=None, n_pin=0, hessian=HESSIAN_AUTO):
        """rti_prepare + rti_feedback for numpy arrays, synchronous (mmpc_rti_step_batch_host; the library brings the
        workspace); u_lb / u_ub [nu] shared or [B, nu] per instance.  V is not modified; returns a dict of numpy
        arrays with rti_feedback's keys."""
        nx, nu, N, NV = self.nx, self.nu, self.N, self.NV
        V = _f64(V, (-1, NV)).copy()
        B = V.shape[0]
        x0_meas, u_prev = _f64(x0_meas, (B, nx)), _f64(u_prev, (B, nu))
        traj, weights = _f64(traj, (B, N, nx)), _f64(weights)
        ws = 0 if weights.ndim == 1 else weights.shape[-1]
        lb, ub, bs = _host_bounds(u_lb, u_ub, B, nu)
        out = dict(V=V, u0=np.zeros((B, nu)), step_inf=np.zeros(B), status=np.full(B, -1, np.int32))
        self._check(self._L.mmpc_rti_step_batch_host(self._h, B, _ptr(V), _ptr(x0_meas), _ptr(u_prev), _ptr(traj),
                                                     _ptr(weights), ws, _ptr(lb), _ptr(ub), bs, int(n_pin),
                                                     int(hessian), _ptr(out["u0"]), _ptr(out["step_inf"]),
                                                     _ptr(out["status"])))
        return out

    def set_state_bounds(self, x_lb=None, x_ub=None):
        """x_lb <= x_k <= x_ub for k = 1..N (None = unbounded); finite bounds select the interior-point variant."""
        lb = None if x_lb is None else _f64(x_lb, (self.nx,))
        ub = None if x_ub is None else _f64(x_ub, (self.nx,))
        self._check(self._L.mmpc_set_state_bounds(self._h, _ptr(lb), _ptr(ub)))

    def state_bounds(self):
        lb, ub = np.zeros(self.nx), np.zeros(self.nx)
        self._check(self._L.mmpc_get_state_bounds(self._h, _ptr(lb), _ptr(ub)))
        return lb, ub

    def set_barrier_rule(self, rule: int):
        """BARRIER_MONOTONE (default) or BARRIER_MEHROTRA for the solves with finite state bounds (mmpc_set_barrier_rule:
        MEHROTRA runs on the 16-lane solver in nonlinear mode, other state-bounded solves then raise MmpcError -4)."""
        self._check(self._L.mmpc_set_barrier_rule(self._h, int(rule)))

    def barrier_rule(self) -> int:
        r = C.c_int32(-1)
        self._check(self._L.mmpc_get_barrier_rule(self._h, C.byref(r)))
        return int(r.value)

    def set_sensitivity_barrier(self, mu=None, sigma_cap=None):
        """Barrier of the feedback gains and the solve VJP on a state-bounded solver (mmpc_set_sensitivity_barrier):
        None is the library's default (the barrier value a monotone-rule solve ends at, cap 1e12), mu=0 switches it
        off -- the state of a new solver, in which those calls refuse a state-bounded solver."""
        dm, dc = C.c_double(), C.c_double()
        self._check(self._L.mmpc_sensitivity_barrier_default(C.byref(dm), C.byref(dc)))
        self._check(self._L.mmpc_set_sensitivity_barrier(self._h, dm.value if mu is None else float(mu),
                                                         dc.value if sigma_cap is None else float(sigma_cap)))

    @property
    def sensitivity_barrier(self):
        """(mu, sigma_cap) of set_sensitivity_barrier; mu = 0: off"""
        mu, cap = C.c_double(), C.c_double()
        self._check(self._L.mmpc_get_sensitivity_barrier(self._h, C.byref(mu), C.byref(cap)))
        return mu.value, cap.value

    def kkt_solver_for(self, B: int) -> int:
        """KKT_* solver a solve of B instances runs (the AUTO choice resolved)."""
        v = C.c_int32()
        self._check(self._L.mmpc_resolve_kkt_solver(self._h, B, C.byref(v)))
        return v.value

    def hessian_for(self, B: int, u_bounded: bool = False) -> int:
        """HESSIAN_GAUSS_NEWTON or HESSIAN_EXACT: what a solve of B instances runs (the AUTO choice resolved)."""
        v = C.c_int32()
        self._check(self._L.mmpc_resolve_hessian(self._h, B, int(bool(u_bounded)), C.byref(v)))
        return v.value

    def linearize_host(self, x, u):
        nx, nu = self.nx, self.nu
        x = _f64(x, (-1, nx))
        B = x.shape[0]
        u = _f64(u, (B, nu))
        A = np.zeros((B, nx * nx)); Bm = np.zeros((B, nx * nu)); xd = np.zeros((B, nx))
        self._check(self._L.mmpc_linearize_batch_host(self._h, B, _ptr(x), _ptr(u), _ptr(A), _ptr(Bm), _ptr(xd)))
        # column-major per instance (CasADi DM order) -> (B, nx, nx) row-major views
        return (A.reshape(B, nx, nx).transpose(0, 2, 1), Bm.reshape(B, nu, nx).transpose(0, 2, 1), xd)


def shard(B: int, n: int, i: int) -> tuple:
    """(first, count) of shard i of B instances over n shards (mmpc_shard; the C-ABI's partition)."""
    f, c = C.c_int64(), C.c_int64()
    _check(lib().mmpc_shard(B, n, i, C.byref(f), C.byref(c)))
    return f.value, c.value


class MultiSolver:
    """One process over several devices (mmpc_multi_*): contiguous shards, one handle and stream per device."""

    def __init__(self, model_json, devices, **opts):
        self._L = L = lib(model_library(model_json))
        o = Opts()
        L.mmpc_default_opts(C.byref(o))
        for k, v in opts.items():
            setattr(o, k, v)
        devs = (C.c_int32 * len(devices))(*devices)
        m = _vp()
        _check(L.mmpc_multi_create(os.fsencode(model_json), C.byref(o), devs, len(devices), C.byref(m)), L)
        self._m = m
        info = ModelInfo()
        h = _vp()
        _check(L.mmpc_multi_handle(m, 0, C.byref(h)), L)
        _check(L.mmpc_get_model_info(h, C.byref(info)), L)
        self.nx, self.nu, self.N, self.NV = info.num_x, info.num_u, info.num_shooting_nodes, info.num_v

    def num_devices(self) -> int:
        n = C.c_int32()
        _check(self._L.mmpc_multi_num_devices(self._m, C.byref(n)), self._L)
        return n.value

    def solve_batch_host(self, x0, u_prev, traj, weights, V=None, u_lb=None, u_ub=None, u_pin=None):
        """u_pin: committed controls [B, m, nu], sharded with the instances (mmpc_multi_solve_batch_host_pinned)"""
        nx, nu, N, NV = self.nx, self.nu, self.N, self.NV
        x0 = _f64(x0, (-1, nx))
        B = x0.shape[0]
        pin, m = _host_pins(u_pin, B, nu, N)
        u_prev, traj, weights = _f64(u_prev, (B, nu)), _f64(traj, (B, N, nx)), _f64(weights)
        ws = 0 if weights.ndim == 1 else weights.shape[-1]
        V = np.zeros((B, NV)) if V is None else _f64(V, (B, NV)).copy()
        st, it, kkt = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B)
        lb, ub, bs = _host_bounds(u_lb, u_ub, B, nu)   # [nu] shared, or [B, nu] per instance
        if m:
            _check(self._L.mmpc_multi_solve_batch_host_pinned(self._m, B, _ptr(x0), _ptr(u_prev), _ptr(traj),
                                                              _ptr(weights), ws, _ptr(lb), _ptr(ub), bs, _ptr(pin), m,
                                                              _ptr(V), _ptr(st), _ptr(it), _ptr(kkt)), self._L)
            return dict(V=V, status=st, iters=it, kkt=kkt)
        _check(self._L.mmpc_multi_solve_batch_host_bounds(self._m, B, _ptr(x0), _ptr(u_prev), _ptr(traj), _ptr(weights),
                                                          ws, _ptr(lb), _ptr(ub), bs, _ptr(V), _ptr(st), _ptr(it),
                                                          _ptr(kkt)), self._L)
        return dict(V=V, status=st, iters=it, kkt=kkt)

    def solve_batch_rccl(self, x0, u_prev, traj, weights, V, status=None, iters=None, kkt=None, u_lb=None,
                         u_ub=None, weights_stride=None, stream=None, bounds_stride=None):
        """mmpc_multi_solve_batch_rccl_bounds: torch tensors on the FIRST device of the handle (fp64, contiguous;
        weights [nx+2nu] shared or [B][nx+2nu], or a flat buffer with an explicit weights_stride; u_lb / u_ub [nu]
        shared or [B][nu], or flat buffers with an explicit bounds_stride); V is updated in place, status / iters
        (int32) / kkt filled if given.  stream: the hipStream_t (int) the inputs were produced on -- default torch's
        current stream of x0's device."""
        B = x0.shape[0]
        ws = (0 if weights.dim() == 1 else weights.shape[-1]) if weights_stride is None else int(weights_stride)
        if bounds_stride is None:
            two_d = [t for t in (u_lb, u_ub) if t is not None and t.dim() == 2]
            if two_d and any(t is not None and t.dim() != 2 for t in (u_lb, u_ub)):
                raise ValueError("u_lb and u_ub: both [nu] or both [B, nu] (one stride serves both)")
            bs = two_d[0].shape[-1] if two_d else 0
        else:
            bs = int(bounds_stride)
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(x0.device).cuda_stream
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        _check(self._L.mmpc_multi_solve_batch_rccl_bounds(self._m, B, p(x0), p(u_prev), p(traj), p(weights), ws,
                                                          p(u_lb), p(u_ub), bs, p(V), p(status), p(iters), p(kkt),
                                                          C.c_void_p(stream) if stream else None), self._L)

    def close(self):
        if getattr(self, "_m", None):
            self._L.mmpc_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rccl_version() -> int:
    """ncclGetVersion of the RCCL the multi-device RCCL path loads (mmpc_rccl_version), e.g. 22606; 0 if none"""
    v = C.c_int32()
    return v.value if lib().mmpc_rccl_version(C.byref(v)) == OK else 0


def flops_per_iteration(N: int, nx: int = 4, nu: int = 2) -> dict:
    """Algorithmic flop count of ONE SQP iteration of the HIP kernel (mul+add = 2), counted from
    sqp_wave.h phase by phase (structure-exploiting: no flop on structural zeros).  See DESIGN.md."""
    M = N * nu
    f = {}
    f["defect_recursion"] = N * (2 * nx * nx + 2 * nx)          # d_{k+1} = A d + c ; e
    f["adjoint"] = (N - 1) * (2 * nx * nx + 2 * nx)             # lam recursion
    f["gradient"] = M * (2 * nx + 8)
    f["lyapunov"] = N * (4 * nx ** 3 + 2 * nu * nx * nx)        # P A, A^T (PA), Z = B^T P
    # H rows: lower part sum over rows of (i+1) steps, upper part (N-1-i) steps; each step = vector x A
    # (2 nx^2) plus nu outputs (2 nx each)
    steps = sum((i + 1) + (N - 1 - i) for i in range(N)) * nu
    f["hessian"] = steps * (2 * nx * nx + 2 * nu * nx)
    f["gauss_jordan"] = sum(2 * (M - 1) * (M - k) for k in range(M)) + M  # rows x remaining cols, + rhs
    f["dx_recursion"] = N * (2 * nx * nx + 2 * nu * nx + nx)
    f["merit"] = N * (2 * nx * (nx + nu) + 12)
    f["total"] = sum(f.values())
    return f


def riccati_flops_per_iteration(N: int, nx: int = 8, nu: int = 4, exact: bool = False) -> dict:
    """Algorithmic flop count (mul+add = 2) of ONE SQP iteration of the lane-per-instance Riccati kernel
    (sqp_lane.h), structure-exploiting for second-order models (A = [[I, hI],[hFq, I+hFqd]],
    B = [[0],[hFu]], nq = nx/2).  Model evaluations are excluded (SURVEY.md 8d counts them separately)."""
    nq, ns = nx // 2, nx + nu
    at_mul = 2 * nq * nx + 2 * nx            # A^T v or A v with the block structure
    f = {}
    f["defect_recursion"] = N * (at_mul + nx)
    f["adjoint_gradient"] = N * (at_mul + 2 * nq * nu + 6 * nu)
    st = 0
    st += nx * nu * 2 * nq                    # G = P_xx B + P_xu
    st += 2 * nx * nx                         # mv = P_xx c + p_x
    st += nu * (nu + 1) // 2 * 4 * nq         # H_ww
    st += nu * (2 * nq + 2 * nx + 4)          # h_w
    st += nu * at_mul                         # H_wx = (A^T G)^T
    st += nx * (nx * (2 * nq + 2) + at_mul)   # A^T P_xx A by columns
    st += at_mul + 2 * nx                     # p_x
    st += nu ** 3 // 3 + nu * nu * (ns + 1)   # Cholesky + forward solve
    st += nu * nu * (ns + 1)                  # back solve (K)
    st += ns * (ns + 1) // 2 * 2 * nu + ns * 2 * nu  # P~ = ... - Y^T Y, p~
    f["riccati"] = N * st
    if exact:   # the stage Hessian W_k enters P~_xx, H_ww and H_wx (its evaluation is a model evaluation: excluded)
        f["riccati"] += N * (nx * nx + nu * nu + nx * nu)
    f["step_recursion"] = N * (2 * nu * ns + at_mul + 2 * nq * nu + nx)
    f["merit"] = N * (4 * nx + 8 * nu)
    f["total"] = sum(f.values())
    return f


def survey_flops_per_iteration(N: int, nx: int = 4, nu: int = 2) -> int:
    """SURVEY.md 8(d) reference count (explicit Gamma + block-triangular G^T Q G + Cholesky)."""
    M, S = N * nu, N * nx
    return int(N * (N - 1) / 2 * 2 * nx * nx * nu + N * (N + 1) * (N + 2) / 6 * 2 * nu * nu * nx
               + M ** 3 / 3 + 4 * M * M + 2 * S * M + N * (nx * nx + nx * nu))
