"""Host-side mirror of the reference's evaluate/solve surface, above the C ABI.

Same names, argument meaning and return shapes as the reference (Julia) so that a caller of
    tv_op_learning_function(x, data, D; Dt=1e-6, kwargs...) -> (u, cost, grad)
    denoise(data, x, op; kwargs...)                          -> u
    TVDenoise(data, parameter)                               -> u
(/root/reference/src/TVLearningFunctionVec.jl:14-27, :45-70; /root/reference/src/BPLDenoising.jl:41-82)
can switch to this module; every call goes through libbpltv (HIP, gfx950) -- no CPU path.

Array convention: a Julia `Array{Float64,3}` of size (M, N, O) (column major) is a C-contiguous
numpy array of shape (O, N, M).  A Julia m x n parameter matrix is a numpy array of shape (n, m).
"""
import ctypes as C
import functools
import math
import re
import numpy as np

from . import _lib

_dp = C.POINTER(C.c_double)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def _alpha_arg(x):
    a = np.asarray(x, dtype=np.float64)
    if a.ndim == 0:
        return np.ascontiguousarray(a.reshape(1)), 1, 1, True
    if a.ndim == 1:
        a = a.reshape(1, -1)  # Julia vector of length m == m x 1 matrix
    if a.ndim != 2:
        raise ValueError("parameter must be a scalar or a matrix, got ndim=%d" % a.ndim)
    a = np.ascontiguousarray(a)
    an, am = a.shape
    return a, am, an, False


def _sr_alpha_arg(x):
    """Sum-of-regularisers parameter: Julia Vector [a1; a2; a3] == numpy (3,); Julia m x n x 3 == numpy (3, n, m)."""
    a = np.ascontiguousarray(x, dtype=np.float64)
    if a.ndim == 1 and a.shape[0] == 3:
        return a, 1, 1, True
    if a.ndim == 3 and a.shape[0] == 3:
        return a, a.shape[2], a.shape[1], False
    raise ValueError("sum-of-regularisers parameter must have shape (3,) or (3, n, m), got %s" % (a.shape,))


class FwdGradientOp:
    """Marker for the forward-difference gradient operator (Neumann boundary), the only operator
    the reference passes on this path (/root/reference/src/TVLearningFunctionVec.jl:17)."""

    def __repr__(self):
        return "FwdGradientOp()"


# reference NamedTuple names -> bpltv_params fields
_PARAM_ALIASES = {
    "ρ": "rho", "rho": "rho", "τ₀": "tau0", "tau0": "tau0", "σ₀": "sigma0", "sigma0": "sigma0",
    "accel": "accel", "maxiter": "maxiter", "Δt": "delta_t", "delta_t": "delta_t",
    "check_every": "check_every", "gap_tol": "gap_tol", "tile_iters": "tile_iters",
    "use_graph": "use_graph", "kappa_cap": "kappa_cap", "refine": "refine", "deterministic": "deterministic",
    "init": "init", "order": "order", "opnorm": "opnorm",
}
_IGNORED = {"verbose_iter", "save_results", "save_iterations", "op", "α", "alpha"}
# ^ reference keys with no numerical meaning on this path (TVLearningFunctionVec.jl:39-42)


def _restores_full_tape(method):
    """A taped method of TVSolver: the tape_checkpoint option its checkpoint_every= set is back at 0 when it returns or raises."""
    @functools.wraps(method)
    def call(self, *args, **kw):
        try:
            return method(self, *args, **kw)
        finally:
            if getattr(self, "_spacing_set", False) and self._h:
                self._spacing_set = False
                self._lib.bpltv_set_option(self._h, b"tape_checkpoint", 0.0)
    return call


class TVSolver:
    """One libbpltv handle: O images of size M x N resident on one GPU (`device`), or -- `ngpus` / `devices`
    -- block-sharded over several GPUs behind the same handle (bpltv_create_multi / bpltv_create_sharded:
    one worker thread per device inside the library, one RCCL collective per evaluation)."""

    def __init__(self, M, N, O, device=-1, ngpus=None, devices=None, dtype=64):
        """dtype: 64 = the reference's Float64 (default); 32 = opt-in single-precision PDHG iteration (include/bpltv.h,
        bpltv_create) -- narrower than the reference, every array in and out stays float64."""
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.M, self.N, self.O = int(M), int(N), int(O)
        self.dtype = int(dtype)
        if devices is not None:
            d = (C.c_int * len(devices))(*[int(x) for x in devices])
            rc = self._lib.bpltv_create_sharded(C.byref(self._h), self.M, self.N, self.O, d, len(devices), self.dtype)
        elif ngpus is not None:
            rc = self._lib.bpltv_create_multi(C.byref(self._h), self.M, self.N, self.O, int(ngpus), self.dtype)
        else:
            rc = self._lib.bpltv_create(C.byref(self._h), self.M, self.N, self.O, int(device), self.dtype)
        if rc:
            msg = self._lib.bpltv_last_error(self._h).decode() if self._h else "bpltv_create failed"
            if self._h:
                self._lib.bpltv_destroy(self._h)
                self._h = C.c_void_p()
            raise _lib.BpltvError(rc, msg)

    # -- plumbing -------------------------------------------------------------------------
    def _check(self, rc):
        if rc:
            raise _lib.BpltvError(rc, self._lib.bpltv_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) and self._h:
            self._lib.bpltv_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def params(self, _sumregs=False, **kw):
        p = _lib.BpltvParams()
        (self._lib.bpltv_sumregs_default_params if _sumregs else self._lib.bpltv_default_params)(C.byref(p))
        variant = kw.pop("variant", None)
        chains = kw.pop("chains", None)
        serialize = kw.pop("serialize_chains", None)
        xcd = kw.pop("xcd", None)
        one_thread = kw.pop("one_thread", None)
        adjm = kw.pop("adjoint_method", None)
        for k, v in kw.items():
            if k in _IGNORED:
                continue
            if k not in _PARAM_ALIASES:
                raise TypeError("unknown solver parameter %r" % k)
            f = _PARAM_ALIASES[k]
            cur = getattr(p, f)
            setattr(p, f, type(cur)(v))
        if variant is not None:
            p.reserved[0] = int(variant)   # PDHG kernel variant (1-based), 0 = auto
        if chains is not None:
            p.reserved[1] = int(chains)    # independent launch chains in the hipGraph, 0 = auto
        if serialize is not None:
            p.reserved[2] = int(bool(serialize))  # replay launch chains one after the other (timing aid)
        if xcd is not None:
            p.reserved[2] |= 2 * int(xcd)        # 1: XCD-aware tile order, 2: natural order (0 = by image size)
        if one_thread:
            p.reserved[2] |= 8                   # both launch chains from the calling thread (timing aid)
        if adjm is not None:
            p.reserved[4] = {"auto": 0, "band": 1, "bcr": 2, "nd": 3}.get(adjm, adjm)  # adjoint factorisation
        return p

    def _batch(self, a, what):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim == 2:
            a = a[None]
        if a.shape != (self.O, self.N, self.M):
            raise ValueError("%s has shape %s, expected (O=%d, N=%d, M=%d)" % (what, a.shape, self.O, self.N, self.M))
        return a

    # -- data ---------------------------------------------------------------------------------
    def set_data(self, ubar, f):
        ubar = self._batch(ubar, "ubar")
        f = self._batch(f, "f")
        self._check(self._lib.bpltv_set_data(self._h, _ptr(ubar), _ptr(f)))

    def set_data_device(self, ubar_ptr, f_ptr):
        """Dataset already resident in HBM (raw device pointers, e.g. torch tensor .data_ptr())."""
        self._check(self._lib.bpltv_set_data_device(self._h, C.c_void_p(ubar_ptr), C.c_void_p(f_ptr)))

    # -- solve --------------------------------------------------------------------------------
    def denoise(self, x, fetch=True, **kw):
        a, am, an, _ = _alpha_arg(x)
        p = self.params(**kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_denoise(self._h, _ptr(a), am, an, C.byref(p), _ptr(u) if fetch else None))
        return u

    def denoise_device(self, alpha_ptr, am=1, an=1, **kw):
        """bpltv_denoise_device: the parameter (am x an doubles, column major) already resident in HBM at `alpha_ptr`
        (e.g. a torch tensor's .data_ptr()); the result stays on the device (u_device_ptr / copy_u_device)."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_denoise_device(self._h, C.c_void_p(alpha_ptr), int(am), int(an), C.byref(p)))

    def evaluate(self, x, delta, fetch_u=True, **kw):
        a, am, an, scalar = _alpha_arg(x)
        self._last_npar = am * an
        p = self.params(**kw)
        u = np.empty((self.O, self.N, self.M)) if fetch_u else None
        cost = C.c_double(0.0)
        grad = np.empty(am * an)
        self._check(self._lib.bpltv_evaluate(self._h, _ptr(a), am, an, float(delta), C.byref(p),
                                             _ptr(u) if fetch_u else None, C.byref(cost), _ptr(grad)))
        g = float(grad[0]) if scalar else grad.reshape(an, am)
        return u, cost.value, g

    def evaluate_partial(self, x, delta, fetch_u=True, **kw):
        """[cost, grad...] of this handle's images only (to be all-reduced across shards)."""
        a, am, an, _ = _alpha_arg(x)
        self._last_npar = am * an
        p = self.params(**kw)
        u = np.empty((self.O, self.N, self.M)) if fetch_u else None
        part = np.empty(1 + am * an)
        self._check(self._lib.bpltv_evaluate_partial(self._h, _ptr(a), am, an, float(delta), C.byref(p),
                                                     _ptr(u) if fetch_u else None, _ptr(part)))
        return u, part

    def evaluate_device(self, x, delta, partial_ptr, **kw):
        """Partial vector written to device memory at `partial_ptr` (1 + am*an doubles)."""
        a, am, an, _ = _alpha_arg(x)
        self._last_npar = am * an
        p = self.params(**kw)
        self._check(self._lib.bpltv_evaluate_device(self._h, _ptr(a), am, an, float(delta), C.byref(p),
                                                    C.c_void_p(partial_ptr)))

    # -- sum-of-regularisers model (/root/reference/src/SumRegsLearningFunction.jl) ----------------------
    def sumregs_denoise(self, x, fetch=True, **kw):
        """sumregs_denoise(data, x, op1, op2, op3[, pOp]) (:38-85).  x: (3,) vector or (3, n, m) patch parameter
        (numpy (3, n, m) == Julia m x n x 3)."""
        a, am, an, _ = _sr_alpha_arg(x)
        p = self.params(_sumregs=True, **kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_sumregs_denoise(self._h, _ptr(a), am, an, C.byref(p), _ptr(u) if fetch else None))
        return u

    def sumregs_evaluate(self, x, delta, fetch_u=True, **kw):
        """sumregs_learning_function(x, data, D; Dt = 1e-3) -> (u, cost, grad) (:8-36); grad has the shape of x."""
        a, am, an, vec = _sr_alpha_arg(x)
        self._last_npar = 3 * am * an
        p = self.params(_sumregs=True, **kw)
        u = np.empty((self.O, self.N, self.M)) if fetch_u else None
        cost = C.c_double(0.0)
        grad = np.empty(3 * am * an)
        self._check(self._lib.bpltv_sumregs_evaluate(self._h, _ptr(a), am, an, float(delta), C.byref(p),
                                                     _ptr(u) if fetch_u else None, C.byref(cost), _ptr(grad)))
        return u, cost.value, (grad.copy() if vec else grad.reshape(3, an, am))

    def sumregs_denoise_device(self, alpha_ptr, am=1, an=1, **kw):
        """bpltv_sumregs_denoise_device: the parameter (3*am*an doubles, three column-major am x an slices -- a
        C-contiguous (3, an, am) array) already resident in HBM at `alpha_ptr`; the result stays on the device
        (u_device_ptr / copy_u_device)."""
        p = self.params(_sumregs=True, **kw)
        self._check(self._lib.bpltv_sumregs_denoise_device(self._h, C.c_void_p(alpha_ptr), int(am), int(an), C.byref(p)))

    def sumregs_vjp(self, u, x, gu, reg=False, want_f=True, want_alpha=True, **kw):
        """Vector-Jacobian product of u = sumregs_denoise(f, x) for the cotangent gu = dL/du (bpltv_sumregs_vjp):
        (grad_f, grad_x).  u, gu: (O, N, M) batches; x: (3,) or (3, n, m).  grad_f has the shape of u (None unless
        want_f), grad_x the shape of x (None unless want_alpha).  gu = u - ubar gives sumregs_evaluate's gradient
        bitwise (reg = the evaluate's delta <= delta_t)."""
        if not (want_f or want_alpha):
            raise ValueError("sumregs_vjp: want_f and want_alpha are both False")
        a, am, an, vec = _sr_alpha_arg(x)
        p = self.params(_sumregs=True, **kw)
        u = self._batch(u, "u")
        gu = self._batch(gu, "gu")
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(3 * am * an) if want_alpha else None
        self._check(self._lib.bpltv_sumregs_vjp(self._h, _ptr(u), _ptr(a), am, an, int(bool(reg)), C.byref(p),
                                                _ptr(gu), _ptr(gf) if want_f else None,
                                                _ptr(ga) if want_alpha else None))
        if ga is not None and not vec:
            ga = ga.reshape(3, an, am)
        return gf, ga

    def sumregs_vjp_device(self, u_ptr, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, reg=False, **kw):
        """bpltv_sumregs_vjp_device: u, gu and grad_f (M*N*O doubles), the parameter and grad_alpha (3*am*an doubles)
        all resident in HBM; either output pointer may be 0 / None, not both."""
        p = self.params(_sumregs=True, **kw)
        self._check(self._lib.bpltv_sumregs_vjp_device(self._h, C.c_void_p(u_ptr), C.c_void_p(alpha_ptr), int(am),
                                                       int(an), int(bool(reg)), C.byref(p), C.c_void_p(gu_ptr),
                                                       C.c_void_p(grad_f_ptr or None),
                                                       C.c_void_p(grad_alpha_ptr or None)))

    # -- forward mode of the sum-of-regularisers model (bpltv_sumregs_jvp / bpltv_sumregs_gauss_newton) ------------
    def sumregs_jvp(self, u, x, df=None, dalpha=None, reg=False, **kw):
        """Jacobian-vector product of u = sumregs_denoise(f, x) (bpltv_sumregs_jvp): du for the tangents (df, dalpha),
        the linear map whose transpose sumregs_vjp computes.  x: (3,) or (3, n, m); df: (O, N, M), or (K, O, N, M) for K
        directions solved against one factorisation; dalpha: shaped like x, or with a leading K; either may be None
        (zero), not both.  Returns du of shape (O, N, M), or (K, O, N, M) when a leading K was given."""
        a, am, an, _vec = _sr_alpha_arg(x)
        df, dalpha, K, batched = self._tangents("sumregs_jvp", df, dalpha, a.shape)
        p = self.params(_sumregs=True, **kw)
        u = self._batch(u, "u")
        du = np.empty((K, self.O, self.N, self.M))
        self._check(self._lib.bpltv_sumregs_jvp(self._h, _ptr(u), _ptr(a), am, an, int(bool(reg)), C.byref(p), K,
                                                _ptr(df) if df is not None else None,
                                                _ptr(dalpha) if dalpha is not None else None, _ptr(du)))
        return du if batched else du[0]

    def sumregs_jvp_device(self, u_ptr, alpha_ptr, am, an, df_ptr, dalpha_ptr, du_ptr, ndir=1, reg=False, **kw):
        """bpltv_sumregs_jvp_device: u (M*N*O doubles), the parameter (3*am*an), df and du (ndir*M*N*O) and dalpha
        (ndir*3*am*an) all resident in HBM (raw device pointers); either tangent pointer may be 0 / None, not both."""
        p = self.params(_sumregs=True, **kw)
        self._check(self._lib.bpltv_sumregs_jvp_device(self._h, C.c_void_p(u_ptr), C.c_void_p(alpha_ptr), int(am),
                                                       int(an), int(bool(reg)), C.byref(p), int(ndir),
                                                       C.c_void_p(df_ptr or None), C.c_void_p(dalpha_ptr or None),
                                                       C.c_void_p(du_ptr)))

    def sumregs_gauss_newton(self, u, ubar, x, reg=False, **kw):
        """Gauss-Newton model of 0.5||u(x) - ubar||^2 (bpltv_sumregs_gauss_newton): (grad, H) with grad = J^T (u - ubar)
        shaped like x and H = J^T J of shape (P, P), P = x.size <= 16, ordered as numpy's x.ravel() (the library's
        parameter layout).  x: (3,), or a (3, n, m) patch."""
        a, am, an, _vec = _sr_alpha_arg(x)
        p = self.params(_sumregs=True, **kw)
        u = self._batch(u, "u")
        ubar = self._batch(ubar, "ubar")
        P = 3 * am * an
        grad, H = np.empty(P), np.empty((P, P))
        self._check(self._lib.bpltv_sumregs_gauss_newton(self._h, _ptr(u), _ptr(ubar), _ptr(a), am, an,
                                                         int(bool(reg)), C.byref(p), _ptr(grad), _ptr(H)))
        return grad.reshape(a.shape), H

    def gradient(self, u, ubar, x, reg=False, **kw):
        a, am, an, scalar = _alpha_arg(x)
        p = self.params(**kw)
        u = self._batch(u, "u")
        ubar = self._batch(ubar, "ubar")
        grad = np.empty(am * an)
        self._check(self._lib.bpltv_gradient(self._h, _ptr(u), _ptr(ubar), _ptr(a), am, an, int(bool(reg)),
                                             C.byref(p), _ptr(grad)))
        return float(grad[0]) if scalar else grad.reshape(an, am)

    def vjp(self, u, x, gu, reg=False, want_f=True, want_alpha=True, **kw):
        """Vector-Jacobian product of u = denoise(f, x) for the cotangent gu = dL/du (bpltv_vjp): (grad_f, grad_x).
        u, gu: (O, N, M) batches; x: a float or an (n, m) parameter.  grad_f has the shape of u (None unless want_f),
        grad_x the type / shape of x (None unless want_alpha).  gu = u - ubar gives gradient(u, ubar, x, reg) bitwise."""
        if not (want_f or want_alpha):
            raise ValueError("vjp: want_f and want_alpha are both False")
        a, am, an, scalar = _alpha_arg(x)
        p = self.params(**kw)
        u = self._batch(u, "u")
        gu = self._batch(gu, "gu")
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(am * an) if want_alpha else None
        self._check(self._lib.bpltv_vjp(self._h, _ptr(u), _ptr(a), am, an, int(bool(reg)), C.byref(p), _ptr(gu),
                                        _ptr(gf) if want_f else None, _ptr(ga) if want_alpha else None))
        if ga is not None:
            ga = float(ga[0]) if scalar else ga.reshape(an, am)
        return gf, ga

    def vjp_device(self, u_ptr, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, reg=False, **kw):
        """bpltv_vjp_device: u, gu and grad_f (M*N*O doubles), the parameter and grad_alpha (am*an doubles, column
        major) all resident in HBM (raw device pointers, e.g. torch tensors' .data_ptr()); either output pointer may
        be 0 / None, not both."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_vjp_device(self._h, C.c_void_p(u_ptr), C.c_void_p(alpha_ptr), int(am), int(an),
                                               int(bool(reg)), C.byref(p), C.c_void_p(gu_ptr),
                                               C.c_void_p(grad_f_ptr or None), C.c_void_p(grad_alpha_ptr or None)))

    # -- per-pixel data-fidelity weight (bpltv_weighted_*) ------------------------------------------------------
    def _weight(self, w):
        """(array, wo) of a fidelity weight: (N, M) -- one plane for the batch -- or (O, N, M), one per image."""
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.shape == (self.N, self.M):
            return w, 1
        if w.shape == (self.O, self.N, self.M):
            return w, self.O
        raise ValueError("w has shape %s, expected (N=%d, M=%d) or (O=%d, N=%d, M=%d)"
                         % (w.shape, self.N, self.M, self.O, self.N, self.M))

    def weighted_denoise(self, x, w, fetch=True, **kw):
        """min_u 0.5 sum w (u - f)^2 + sum alpha |grad u| on the resident f (bpltv_weighted_denoise).  x: as denoise;
        w >= 0: (N, M) or (O, N, M).  w = 1 everywhere is denoise(x) bit for bit."""
        a, am, an, _ = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self.params(**kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_weighted_denoise(self._h, _ptr(wa), wo, _ptr(a), am, an, C.byref(p),
                                                     _ptr(u) if fetch else None))
        return u

    def weighted_denoise_device(self, w_ptr, wo, alpha_ptr, am=1, an=1, **kw):
        """bpltv_weighted_denoise_device: w (wo planes of M*N doubles, wo = 1 or O) and the parameter (am x an doubles)
        already resident in HBM; the result stays on the device (u_device_ptr / copy_u_device)."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_weighted_denoise_device(self._h, C.c_void_p(w_ptr), int(wo), C.c_void_p(alpha_ptr),
                                                            int(am), int(an), C.byref(p)))

    def weighted_vjp(self, u, f, x, w, gu, want_f=True, want_alpha=True, want_w=True, **kw):
        """Vector-Jacobian product of u = weighted_denoise(f, x, w) for the cotangent gu (bpltv_weighted_vjp):
        (grad_f, grad_x, grad_w).  u, gu: (O, N, M); f: (O, N, M), or None when grad_w is not wanted; w > 0: (N, M) or
        (O, N, M).  grad_w has the shape of w -- for (N, M) the sum over the images; an output not wanted is None."""
        if not (want_f or want_alpha or want_w):
            raise ValueError("weighted_vjp: want_f, want_alpha and want_w are all False")
        a, am, an, scalar = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self.params(**kw)
        u = self._batch(u, "u")
        gu = self._batch(gu, "gu")
        if want_w and f is None:
            raise ValueError("weighted_vjp: grad_w needs f")
        f = self._batch(f, "f") if f is not None else None
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(am * an) if want_alpha else None
        gw = np.empty(wa.shape) if want_w else None
        self._check(self._lib.bpltv_weighted_vjp(self._h, _ptr(u), _ptr(f) if f is not None else None, _ptr(wa), wo,
                                                 _ptr(a), am, an, C.byref(p), _ptr(gu),
                                                 _ptr(gf) if want_f else None, _ptr(ga) if want_alpha else None,
                                                 _ptr(gw) if want_w else None))
        if ga is not None:
            ga = float(ga[0]) if scalar else ga.reshape(an, am)
        return gf, ga, gw

    def weighted_vjp_device(self, u_ptr, f_ptr, w_ptr, wo, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr,
                            grad_w_ptr, **kw):
        """bpltv_weighted_vjp_device: every array resident in HBM (raw device pointers); any output pointer may be
        0 / None, not all three; f_ptr may be 0 / None only if grad_w_ptr is."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_weighted_vjp_device(self._h, C.c_void_p(u_ptr), C.c_void_p(f_ptr or None),
                                                        C.c_void_p(w_ptr), int(wo), C.c_void_p(alpha_ptr), int(am),
                                                        int(an), C.byref(p), C.c_void_p(gu_ptr),
                                                        C.c_void_p(grad_f_ptr or None),
                                                        C.c_void_p(grad_alpha_ptr or None),
                                                        C.c_void_p(grad_w_ptr or None)))

    # -- reverse mode through the iterations (bpltv_unrolled_*) --------------------------------------------------
    # Every *_unrolled_tape_doubles, *_unrolled_denoise* and *_unrolled_vjp* method takes checkpoint_every=C on top of the
    # params keywords (option "tape_checkpoint"): None / 0 the full tape, C >= 1 the iteration state
    # every C iterations instead of a tape -- the sweep then recomputes each segment's tape, same bits, one more forward
    # solve -- and -1 the spacing of least memory (auto_checkpoint_every).  Solve, sweep and tape_doubles of one tape take the
    # same value.
    def _taped_params(self, kw, **model):
        """params(**kw) without checkpoint_every=, which becomes the handle's tape_checkpoint option right before the
        ABI call; absent means 0, so a handle shared between calls never inherits a spacing.  A spacing set here is taken
        back when the method returns (_restores_full_tape), so the handle keeps none for direct ABI calls either."""
        c = kw.pop("checkpoint_every", None)
        p = self.params(**model, **kw)
        self.set_option("tape_checkpoint", 0 if c is None else c)
        self._spacing_set = bool(c)
        return p

    @staticmethod
    def auto_checkpoint_every(maxiter, model="tv"):
        """The spacing checkpoint_every=-1 stands for: ceil(sqrt(nplanes * maxiter / tape_planes)) in [1, maxiter], which
        minimises nplanes * ceil(maxiter / C) + tape_planes * C up to rounding.  model: "tv" (3 state planes, 2 tape
        planes per iteration), "weighted" (3, 3) or "sumregs" (7, 6)."""
        nplanes, tape_planes = {"tv": (3, 2), "weighted": (3, 3), "sumregs": (7, 6)}[model]
        maxiter = int(maxiter)
        if maxiter < 1:
            raise ValueError("auto_checkpoint_every: maxiter must be at least 1")
        need = nplanes * maxiter
        c = math.isqrt(need // tape_planes)
        while c * c * tape_planes < need:
            c += 1
        return max(1, min(c, maxiter))

    def unrolled_tape_doubles(self, **kw):
        """Doubles of the tape an unrolled solve with these params records: 2 * maxiter * M*N*O."""
        p = self._taped_params(kw)
        n = C.c_ulonglong(0)
        self._check(self._lib.bpltv_unrolled_tape_doubles(self._h, C.byref(p), C.byref(n)))
        return int(n.value)

    def unrolled_denoise(self, x, fetch=True, **kw):
        """denoise(x) with rho = 0 -- the same u bit for bit -- that also records the tape of the iterations in the
        handle, for unrolled_vjp with the same x and params (bpltv_unrolled_denoise)."""
        a, am, an, _ = _alpha_arg(x)
        p = self._taped_params(kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_unrolled_denoise(self._h, _ptr(a), am, an, C.byref(p), _ptr(u) if fetch else None))
        return u

    def unrolled_denoise_device(self, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_unrolled_denoise_device: the parameter resident in HBM, the result left there (u_device_ptr /
        copy_u_device); tape_ptr: a caller-owned HBM buffer of unrolled_tape_doubles(**kw) doubles, or None / 0 for
        the handle's own tape."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_unrolled_denoise_device(self._h, C.c_void_p(alpha_ptr), int(am), int(an),
                                                            C.byref(p), C.c_void_p(tape_ptr or None)))

    def unrolled_vjp(self, x, gu, want_f=True, want_alpha=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = unrolled_denoise(x) for the cotangent gu = dL/du, by a
        reverse sweep over the handle's tape (bpltv_unrolled_vjp): (grad_f, grad_x).  x and the params must be those
        of the solve.  gu: (O, N, M); grad_f has its shape (None unless want_f), grad_x the type / shape of x (None
        unless want_alpha)."""
        if not (want_f or want_alpha):
            raise ValueError("unrolled_vjp: want_f and want_alpha are both False")
        a, am, an, scalar = _alpha_arg(x)
        p = self._taped_params(kw)
        gu = self._batch(gu, "gu")
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(am * an) if want_alpha else None
        self._check(self._lib.bpltv_unrolled_vjp(self._h, _ptr(a), am, an, C.byref(p), _ptr(gu),
                                                 _ptr(gf) if want_f else None, _ptr(ga) if want_alpha else None))
        if ga is not None:
            ga = float(ga[0]) if scalar else ga.reshape(an, am)
        return gf, ga

    def unrolled_vjp_device(self, tape_ptr, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, **kw):
        """bpltv_unrolled_vjp_device: the tape (None / 0: the handle's own), the parameter, gu and the outputs resident
        in HBM (raw device pointers); either output pointer may be 0 / None, not both."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_unrolled_vjp_device(self._h, C.c_void_p(tape_ptr or None), C.c_void_p(alpha_ptr),
                                                        int(am), int(an), C.byref(p), C.c_void_p(gu_ptr),
                                                        C.c_void_p(grad_f_ptr or None),
                                                        C.c_void_p(grad_alpha_ptr or None)))

    # -- channel-coupled TV for colour images (bpltv_color_*) ------------------------------------------------------
    # The handle's O planes are O / channels colour images of `channels` consecutive planes; x is one parameter shared by the
    # batch and the channels.  The tape has the TV tape's size: unrolled_tape_doubles.
    def color_denoise(self, x, channels, fetch=True, **kw):
        """Vectorial TV: the channels of a colour image share one projection per pixel (bpltv_color_denoise).  No tape, any
        maxiter >= 1; u is bitwise color_unrolled_denoise's."""
        a, am, an, _ = _alpha_arg(x)
        p = self.params(**kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_color_denoise(self._h, int(channels), _ptr(a), am, an, C.byref(p), _ptr(u) if fetch else None))
        return u

    def color_denoise_device(self, channels, alpha_ptr, am=1, an=1, **kw):
        """bpltv_color_denoise_device: the parameter resident in HBM, the result left there (u_device_ptr / copy_u_device)."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_color_denoise_device(self._h, int(channels), C.c_void_p(alpha_ptr), int(am), int(an), C.byref(p)))

    def color_unrolled_denoise(self, x, channels, fetch=True, **kw):
        """color_denoise that also records the tape of the iterations in the handle, for color_unrolled_vjp with the same
        x, channels and params (bpltv_color_unrolled_denoise)."""
        a, am, an, _ = _alpha_arg(x)
        p = self._taped_params(kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_color_unrolled_denoise(self._h, int(channels), _ptr(a), am, an, C.byref(p),
                                                           _ptr(u) if fetch else None))
        return u

    def color_unrolled_denoise_device(self, channels, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_color_unrolled_denoise_device: the parameter resident in HBM, the result left there; tape_ptr: a
        caller-owned HBM buffer of unrolled_tape_doubles(**kw) doubles, or None / 0 for the handle's colour tape."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_color_unrolled_denoise_device(self._h, int(channels), C.c_void_p(alpha_ptr), int(am), int(an),
                                                                  C.byref(p), C.c_void_p(tape_ptr or None)))

    def color_unrolled_vjp(self, x, channels, gu, want_f=True, want_alpha=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = color_unrolled_denoise(x, channels) for the cotangent gu, by
        a reverse sweep over the handle's colour tape (bpltv_color_unrolled_vjp): (grad_f, grad_x), as unrolled_vjp."""
        if not (want_f or want_alpha):
            raise ValueError("color_unrolled_vjp: want_f and want_alpha are both False")
        a, am, an, scalar = _alpha_arg(x)
        p = self._taped_params(kw)
        gu = self._batch(gu, "gu")
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(am * an) if want_alpha else None
        self._check(self._lib.bpltv_color_unrolled_vjp(self._h, int(channels), _ptr(a), am, an, C.byref(p), _ptr(gu),
                                                       _ptr(gf) if want_f else None, _ptr(ga) if want_alpha else None))
        if ga is not None:
            ga = float(ga[0]) if scalar else ga.reshape(an, am)
        return gf, ga

    def color_unrolled_vjp_device(self, channels, tape_ptr, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, **kw):
        """bpltv_color_unrolled_vjp_device: the tape (None / 0: the handle's own), the parameter, gu and the outputs
        resident in HBM (raw device pointers); either output pointer may be 0 / None, not both."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_color_unrolled_vjp_device(self._h, int(channels), C.c_void_p(tape_ptr or None),
                                                              C.c_void_p(alpha_ptr), int(am), int(an), C.byref(p),
                                                              C.c_void_p(gu_ptr), C.c_void_p(grad_f_ptr or None),
                                                              C.c_void_p(grad_alpha_ptr or None)))

    def color_unrolled_jvp(self, x, channels, df=None, dalpha=None, want_u=False, **kw):
        """Jacobian-vector product of the maxiter-step map u = color_denoise(x, channels) of the resident f
        (bpltv_color_unrolled_jvp): a tangent sweep through the channel-coupled iterations, no tape -- the linear map whose
        transpose color_unrolled_vjp computes.  Tangents, result and want_u as unrolled_jvp; channels = 1 is unrolled_jvp
        bit for bit."""
        a, am, an, scalar = _alpha_arg(x)
        df, dalpha, K, batched = self._tangents("color_unrolled_jvp", df, dalpha, () if scalar else (an, am))
        p = self.params(**kw)
        du = np.empty((K, self.O, self.N, self.M))
        u = np.empty((self.O, self.N, self.M)) if want_u else None
        self._check(self._lib.bpltv_color_unrolled_jvp(self._h, int(channels), _ptr(a), am, an, C.byref(p), K,
                                                       _ptr(df) if df is not None else None,
                                                       _ptr(dalpha) if dalpha is not None else None, _ptr(du),
                                                       _ptr(u) if want_u else None))
        du = du if batched else du[0]
        return (du, u) if want_u else du

    def color_unrolled_jvp_device(self, channels, alpha_ptr, am, an, df_ptr, dalpha_ptr, du_ptr, u_ptr=None, ndir=1, **kw):
        """bpltv_color_unrolled_jvp_device: as unrolled_jvp_device, for colour images of `channels` planes."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_color_unrolled_jvp_device(self._h, int(channels), C.c_void_p(alpha_ptr), int(am), int(an),
                                                              C.byref(p), int(ndir), C.c_void_p(df_ptr or None),
                                                              C.c_void_p(dalpha_ptr or None), C.c_void_p(du_ptr),
                                                              C.c_void_p(u_ptr or None)))

    def color_unrolled_gauss_newton(self, x, channels, **kw):
        """Gauss-Newton model of the maxiter-step loss 0.5||u_K(x) - ubar||^2 of the channel-coupled solve, over all planes
        (bpltv_color_unrolled_gauss_newton): (cost, grad, H) as unrolled_gauss_newton."""
        a, am, an, scalar = _alpha_arg(x)
        p = self.params(**kw)
        P = am * an
        cost, grad, H = C.c_double(0.0), np.empty(P), np.empty((P, P))
        self._check(self._lib.bpltv_color_unrolled_gauss_newton(self._h, int(channels), _ptr(a), am, an, C.byref(p),
                                                                C.byref(cost), _ptr(grad), _ptr(H)))
        return float(cost.value), (float(grad[0]) if scalar else grad.reshape(an, am)), H

    # -- channel-coupled TV with a per-pixel fidelity weight (bpltv_color_weighted_*) ------------------------------
    # w >= 0, zeros allowed: (N, M) -- one plane for every plane of the batch -- or (O, N, M), one per plane (per channel).  The
    # tape has the weighted tape's size: weighted_unrolled_tape_doubles.
    def color_weighted_denoise(self, x, channels, w, fetch=True, **kw):
        """Vectorial TV with the fidelity 0.5 sum_c w_c (u_c - f_c)^2 (bpltv_color_weighted_denoise): colour inpainting,
        demosaicing, a variance per channel.  No tape; u is bitwise color_weighted_unrolled_denoise's, and with w = 1
        color_denoise's."""
        a, am, an, _ = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self.params(**kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_color_weighted_denoise(self._h, int(channels), _ptr(wa), wo, _ptr(a), am, an, C.byref(p),
                                                           _ptr(u) if fetch else None))
        return u

    def color_weighted_denoise_device(self, channels, w_ptr, wo, alpha_ptr, am=1, an=1, **kw):
        """bpltv_color_weighted_denoise_device: w (wo planes) and the parameter resident in HBM, the result left there."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_color_weighted_denoise_device(self._h, int(channels), C.c_void_p(w_ptr), int(wo),
                                                                  C.c_void_p(alpha_ptr), int(am), int(an), C.byref(p)))

    def color_weighted_unrolled_denoise(self, x, channels, w, fetch=True, **kw):
        """color_weighted_denoise that also records the tape of the iterations in the handle, for
        color_weighted_unrolled_vjp with the same x, channels, w and params (bpltv_color_weighted_unrolled_denoise)."""
        a, am, an, _ = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self._taped_params(kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_color_weighted_unrolled_denoise(self._h, int(channels), _ptr(wa), wo, _ptr(a), am, an,
                                                                    C.byref(p), _ptr(u) if fetch else None))
        return u

    def color_weighted_unrolled_denoise_device(self, channels, w_ptr, wo, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_color_weighted_unrolled_denoise_device: w (wo planes) and the parameter resident in HBM, the result left
        there; tape_ptr: a caller-owned HBM buffer of weighted_unrolled_tape_doubles(**kw) doubles, or None / 0 for the
        handle's colour-weighted tape."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_color_weighted_unrolled_denoise_device(self._h, int(channels), C.c_void_p(w_ptr), int(wo),
                                                                           C.c_void_p(alpha_ptr), int(am), int(an), C.byref(p),
                                                                           C.c_void_p(tape_ptr or None)))

    def color_weighted_unrolled_vjp(self, x, channels, w, gu, want_f=True, want_alpha=True, want_w=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = color_weighted_unrolled_denoise(x, channels, w) for the
        cotangent gu, by a reverse sweep over the handle's colour-weighted tape (bpltv_color_weighted_unrolled_vjp):
        (grad_f, grad_x, grad_w), as weighted_unrolled_vjp.  grad_w has the shape of w -- for (N, M) the sum over the planes."""
        if not (want_f or want_alpha or want_w):
            raise ValueError("color_weighted_unrolled_vjp: want_f, want_alpha and want_w are all False")
        a, am, an, scalar = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self._taped_params(kw)
        gu = self._batch(gu, "gu")
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(am * an) if want_alpha else None
        gw = np.empty(wa.shape) if want_w else None
        self._check(self._lib.bpltv_color_weighted_unrolled_vjp(self._h, int(channels), _ptr(wa), wo, _ptr(a), am, an, C.byref(p),
                                                                _ptr(gu), _ptr(gf) if want_f else None,
                                                                _ptr(ga) if want_alpha else None,
                                                                _ptr(gw) if want_w else None))
        if ga is not None:
            ga = float(ga[0]) if scalar else ga.reshape(an, am)
        return gf, ga, gw

    def color_weighted_unrolled_vjp_device(self, channels, tape_ptr, w_ptr, wo, alpha_ptr, am, an, gu_ptr, grad_f_ptr,
                                           grad_alpha_ptr, grad_w_ptr, **kw):
        """bpltv_color_weighted_unrolled_vjp_device: the tape (None / 0: the handle's own), w, the parameter, gu and the
        outputs resident in HBM (raw device pointers); any output pointer may be 0 / None, not all three."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_color_weighted_unrolled_vjp_device(self._h, int(channels), C.c_void_p(tape_ptr or None),
                                                                       C.c_void_p(w_ptr), int(wo), C.c_void_p(alpha_ptr),
                                                                       int(am), int(an), C.byref(p), C.c_void_p(gu_ptr),
                                                                       C.c_void_p(grad_f_ptr or None),
                                                                       C.c_void_p(grad_alpha_ptr or None),
                                                                       C.c_void_p(grad_w_ptr or None)))

    # -- reverse mode through the weighted iterations (bpltv_weighted_unrolled_*) --------------------------------
    def weighted_unrolled_tape_doubles(self, **kw):
        """Doubles of the tape a weighted unrolled solve with these params records: 3 * maxiter * M*N*O."""
        p = self._taped_params(kw)
        n = C.c_ulonglong(0)
        self._check(self._lib.bpltv_weighted_unrolled_tape_doubles(self._h, C.byref(p), C.byref(n)))
        return int(n.value)

    def weighted_unrolled_denoise(self, x, w, fetch=True, **kw):
        """weighted_denoise(x, w) -- the same u bit for bit, w >= 0 with zeros allowed -- that also records the tape of
        the iterations in the handle, for weighted_unrolled_vjp with the same x, w and params
        (bpltv_weighted_unrolled_denoise)."""
        a, am, an, _ = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self._taped_params(kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_weighted_unrolled_denoise(self._h, _ptr(wa), wo, _ptr(a), am, an, C.byref(p),
                                                              _ptr(u) if fetch else None))
        return u

    def weighted_unrolled_denoise_device(self, w_ptr, wo, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_weighted_unrolled_denoise_device: w (wo planes) and the parameter resident in HBM, the result left
        there; tape_ptr: a caller-owned HBM buffer of weighted_unrolled_tape_doubles(**kw) doubles, or None / 0 for the
        handle's own weighted tape."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_weighted_unrolled_denoise_device(self._h, C.c_void_p(w_ptr), int(wo),
                                                                     C.c_void_p(alpha_ptr), int(am), int(an),
                                                                     C.byref(p), C.c_void_p(tape_ptr or None)))

    def weighted_unrolled_vjp(self, x, w, gu, want_f=True, want_alpha=True, want_w=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = weighted_unrolled_denoise(x, w) for the cotangent gu, by
        a reverse sweep over the handle's weighted tape (bpltv_weighted_unrolled_vjp): (grad_f, grad_x, grad_w).  x, w
        and the params must be those of the solve; w >= 0, zeros allowed.  grad_w has the shape of w -- for (N, M) the
        sum over the images; an output not wanted is None."""
        if not (want_f or want_alpha or want_w):
            raise ValueError("weighted_unrolled_vjp: want_f, want_alpha and want_w are all False")
        a, am, an, scalar = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self._taped_params(kw)
        gu = self._batch(gu, "gu")
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(am * an) if want_alpha else None
        gw = np.empty(wa.shape) if want_w else None
        self._check(self._lib.bpltv_weighted_unrolled_vjp(self._h, _ptr(wa), wo, _ptr(a), am, an, C.byref(p), _ptr(gu),
                                                          _ptr(gf) if want_f else None,
                                                          _ptr(ga) if want_alpha else None,
                                                          _ptr(gw) if want_w else None))
        if ga is not None:
            ga = float(ga[0]) if scalar else ga.reshape(an, am)
        return gf, ga, gw

    def weighted_unrolled_vjp_device(self, tape_ptr, w_ptr, wo, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr,
                                     grad_w_ptr, **kw):
        """bpltv_weighted_unrolled_vjp_device: the tape (None / 0: the handle's own), w, the parameter, gu and the
        outputs resident in HBM (raw device pointers); any output pointer may be 0 / None, not all three."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_weighted_unrolled_vjp_device(self._h, C.c_void_p(tape_ptr or None),
                                                                 C.c_void_p(w_ptr), int(wo), C.c_void_p(alpha_ptr),
                                                                 int(am), int(an), C.byref(p), C.c_void_p(gu_ptr),
                                                                 C.c_void_p(grad_f_ptr or None),
                                                                 C.c_void_p(grad_alpha_ptr or None),
                                                                 C.c_void_p(grad_w_ptr or None)))

    # -- TV-L1: the data term w |u - f|, for impulse noise (bpltv_lone_*) ------------------------------------------
    # w >= 0, zeros allowed: (N, M) or (O, N, M).  The tape has the weighted tape's size: weighted_unrolled_tape_doubles.
    def l1_denoise(self, x, w, fetch=True, **kw):
        """TV-L1 denoising of the resident f (bpltv_lone_denoise): min sum w |u - f| + sum alpha |grad u|, maxiter iterations
        of the weighted recurrence with a soft threshold around f as the primal step.  Removes isolated outliers exactly
        and keeps the contrast of the rest.  No tape; u is bitwise l1_unrolled_denoise's."""
        a, am, an, _ = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self.params(**kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_lone_denoise(self._h, _ptr(wa), wo, _ptr(a), am, an, C.byref(p), _ptr(u) if fetch else None))
        return u

    def l1_denoise_device(self, w_ptr, wo, alpha_ptr, am=1, an=1, **kw):
        """bpltv_lone_denoise_device: w (wo planes) and the parameter resident in HBM, the result left there."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_lone_denoise_device(self._h, C.c_void_p(w_ptr), int(wo), C.c_void_p(alpha_ptr), int(am),
                                                      int(an), C.byref(p)))

    def l1_unrolled_denoise(self, x, w, fetch=True, **kw):
        """l1_denoise(x, w) -- the same u bit for bit -- that also records the tape of the iterations in the handle, for
        l1_unrolled_vjp with the same x, w and params (bpltv_lone_unrolled_denoise)."""
        a, am, an, _ = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self._taped_params(kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_lone_unrolled_denoise(self._h, _ptr(wa), wo, _ptr(a), am, an, C.byref(p),
                                                        _ptr(u) if fetch else None))
        return u

    def l1_unrolled_denoise_device(self, w_ptr, wo, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_lone_unrolled_denoise_device: w (wo planes) and the parameter resident in HBM, the result left there;
        tape_ptr: a caller-owned HBM buffer of weighted_unrolled_tape_doubles(**kw) doubles, or None / 0 for the handle's
        own L1 tape."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_lone_unrolled_denoise_device(self._h, C.c_void_p(w_ptr), int(wo), C.c_void_p(alpha_ptr),
                                                               int(am), int(an), C.byref(p), C.c_void_p(tape_ptr or None)))

    def l1_unrolled_vjp(self, x, w, gu, want_f=True, want_alpha=True, want_w=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = l1_unrolled_denoise(x, w) for the cotangent gu, by a reverse
        sweep over the handle's L1 tape (bpltv_lone_unrolled_vjp): (grad_f, grad_x, grad_w), as weighted_unrolled_vjp."""
        if not (want_f or want_alpha or want_w):
            raise ValueError("l1_unrolled_vjp: want_f, want_alpha and want_w are all False")
        a, am, an, scalar = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self._taped_params(kw)
        gu = self._batch(gu, "gu")
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(am * an) if want_alpha else None
        gw = np.empty(wa.shape) if want_w else None
        self._check(self._lib.bpltv_lone_unrolled_vjp(self._h, _ptr(wa), wo, _ptr(a), am, an, C.byref(p), _ptr(gu),
                                                    _ptr(gf) if want_f else None, _ptr(ga) if want_alpha else None,
                                                    _ptr(gw) if want_w else None))
        if ga is not None:
            ga = float(ga[0]) if scalar else ga.reshape(an, am)
        return gf, ga, gw

    def l1_unrolled_vjp_device(self, tape_ptr, w_ptr, wo, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, grad_w_ptr, **kw):
        """bpltv_lone_unrolled_vjp_device: the tape (None / 0: the handle's own), w, the parameter, gu and the outputs resident
        in HBM (raw device pointers); any output pointer may be 0 / None, not all three."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_lone_unrolled_vjp_device(self._h, C.c_void_p(tape_ptr or None), C.c_void_p(w_ptr), int(wo),
                                                           C.c_void_p(alpha_ptr), int(am), int(an), C.byref(p),
                                                           C.c_void_p(gu_ptr), C.c_void_p(grad_f_ptr or None),
                                                           C.c_void_p(grad_alpha_ptr or None), C.c_void_p(grad_w_ptr or None)))

    # -- TV-KL: the data term w (u - f log u), for Poisson noise (bpltv_kl_*) ------------------------------------------
    # f finite and >= 0 (zero counts allowed); w >= 0, zeros allowed: (N, M) or (O, N, M).  The tape has the weighted tape's size.
    def kl_denoise(self, x, w, fetch=True, **kw):
        """TV-KL denoising of the resident f (bpltv_kl_denoise): min sum w (u - f log u) + sum alpha |grad u| over u >= 0,
        maxiter iterations of the weighted recurrence with the closed-form prox of the Kullback-Leibler divergence as the primal
        step.  The model for photon counts.  No tape; u is bitwise kl_unrolled_denoise's."""
        a, am, an, _ = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self.params(**kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_kl_denoise(self._h, _ptr(wa), wo, _ptr(a), am, an, C.byref(p), _ptr(u) if fetch else None))
        return u

    def kl_denoise_device(self, w_ptr, wo, alpha_ptr, am=1, an=1, **kw):
        """bpltv_kl_denoise_device: w (wo planes) and the parameter resident in HBM, the result left there."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_kl_denoise_device(self._h, C.c_void_p(w_ptr), int(wo), C.c_void_p(alpha_ptr), int(am),
                                                      int(an), C.byref(p)))

    def kl_unrolled_denoise(self, x, w, fetch=True, **kw):
        """kl_denoise(x, w) -- the same u bit for bit -- that also records the tape of the iterations in the handle, for
        kl_unrolled_vjp with the same x, w and params (bpltv_kl_unrolled_denoise)."""
        a, am, an, _ = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self._taped_params(kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_kl_unrolled_denoise(self._h, _ptr(wa), wo, _ptr(a), am, an, C.byref(p),
                                                        _ptr(u) if fetch else None))
        return u

    def kl_unrolled_denoise_device(self, w_ptr, wo, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_kl_unrolled_denoise_device: w (wo planes) and the parameter resident in HBM, the result left there;
        tape_ptr: a caller-owned HBM buffer of weighted_unrolled_tape_doubles(**kw) doubles, or None / 0 for the handle's
        own KL tape."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_kl_unrolled_denoise_device(self._h, C.c_void_p(w_ptr), int(wo), C.c_void_p(alpha_ptr),
                                                               int(am), int(an), C.byref(p), C.c_void_p(tape_ptr or None)))

    def kl_unrolled_vjp(self, x, w, gu, want_f=True, want_alpha=True, want_w=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = kl_unrolled_denoise(x, w) for the cotangent gu, by a reverse
        sweep over the handle's KL tape (bpltv_kl_unrolled_vjp): (grad_f, grad_x, grad_w), as weighted_unrolled_vjp."""
        if not (want_f or want_alpha or want_w):
            raise ValueError("kl_unrolled_vjp: want_f, want_alpha and want_w are all False")
        a, am, an, scalar = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self._taped_params(kw)
        gu = self._batch(gu, "gu")
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(am * an) if want_alpha else None
        gw = np.empty(wa.shape) if want_w else None
        self._check(self._lib.bpltv_kl_unrolled_vjp(self._h, _ptr(wa), wo, _ptr(a), am, an, C.byref(p), _ptr(gu),
                                                    _ptr(gf) if want_f else None, _ptr(ga) if want_alpha else None,
                                                    _ptr(gw) if want_w else None))
        if ga is not None:
            ga = float(ga[0]) if scalar else ga.reshape(an, am)
        return gf, ga, gw

    def kl_unrolled_vjp_device(self, tape_ptr, w_ptr, wo, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, grad_w_ptr, **kw):
        """bpltv_kl_unrolled_vjp_device: the tape (None / 0: the handle's own), w, the parameter, gu and the outputs resident
        in HBM (raw device pointers); any output pointer may be 0 / None, not all three."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_kl_unrolled_vjp_device(self._h, C.c_void_p(tape_ptr or None), C.c_void_p(w_ptr), int(wo),
                                                           C.c_void_p(alpha_ptr), int(am), int(an), C.byref(p),
                                                           C.c_void_p(gu_ptr), C.c_void_p(grad_f_ptr or None),
                                                           C.c_void_p(grad_alpha_ptr or None), C.c_void_p(grad_w_ptr or None)))

    # -- forward mode (bpltv_jvp / bpltv_gauss_newton) -------------------------------------------------------
    def _tangents(self, what, df, dalpha, ashape):
        """(df, dalpha, K, batched): the tangents as contiguous (K, ...) stacks, either None; batched = a leading K was
        given.  df: (O, N, M) or (K, O, N, M); dalpha: shaped like the parameter (ashape: a TV parameter, the three
        slices (3,) / (3, n, m) of the sum-of-regularisers model, or O blocks of either) or with a leading K."""
        if df is None and dalpha is None:
            raise ValueError("%s: df and dalpha are both None" % what)
        K, batched = None, False
        if df is not None:
            df = np.ascontiguousarray(df, dtype=np.float64)
            if df.ndim == 2:
                df = df[None]
            if df.ndim == 3:
                df = df[None]
            else:
                batched = True
            if df.ndim != 4 or df.shape[1:] != (self.O, self.N, self.M):
                raise ValueError("%s: df has shape %s, expected (O=%d, N=%d, M=%d) or (K, O, N, M)"
                                 % (what, df.shape, self.O, self.N, self.M))
            K = df.shape[0]
        if dalpha is not None:
            dalpha = np.asarray(dalpha, dtype=np.float64)
            if dalpha.shape == tuple(ashape):
                dalpha = dalpha[None]
            elif dalpha.ndim >= 1 and dalpha.shape[1:] == tuple(ashape):
                batched = True
            else:
                raise ValueError("%s: dalpha has shape %s, expected %s or (K,) + %s"
                                 % (what, dalpha.shape, tuple(ashape), tuple(ashape)))
            dalpha = np.ascontiguousarray(dalpha)
            if K is None:
                K = dalpha.shape[0]
        if K < 1 or (df is not None and df.shape[0] != K) or (dalpha is not None and dalpha.shape[0] != K):
            raise ValueError("%s: df and dalpha hold different numbers of directions" % what)
        return df, dalpha, K, batched

    def jvp(self, u, x, df=None, dalpha=None, reg=False, **kw):
        """Jacobian-vector product of u = denoise(f, x) (bpltv_jvp): du for the tangents (df, dalpha), the linear map
        whose transpose vjp computes.  df: (O, N, M), or (K, O, N, M) for K directions solved against one
        factorisation; dalpha: shaped like x, or with a leading K; either may be None (zero), not both.  Returns du
        of shape (O, N, M), or (K, O, N, M) when a leading K was given."""
        a, am, an, scalar = _alpha_arg(x)
        df, dalpha, K, batched = self._tangents("jvp", df, dalpha, () if scalar else (an, am))
        p = self.params(**kw)
        u = self._batch(u, "u")
        du = np.empty((K, self.O, self.N, self.M))
        self._check(self._lib.bpltv_jvp(self._h, _ptr(u), _ptr(a), am, an, int(bool(reg)), C.byref(p), K,
                                        _ptr(df) if df is not None else None,
                                        _ptr(dalpha) if dalpha is not None else None, _ptr(du)))
        return du if batched else du[0]

    def jvp_device(self, u_ptr, alpha_ptr, am, an, df_ptr, dalpha_ptr, du_ptr, ndir=1, reg=False, **kw):
        """bpltv_jvp_device: u (M*N*O doubles), the parameter (am*an), df and du (ndir*M*N*O) and dalpha (ndir*am*an)
        all resident in HBM (raw device pointers); either tangent pointer may be 0 / None, not both."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_jvp_device(self._h, C.c_void_p(u_ptr), C.c_void_p(alpha_ptr), int(am), int(an),
                                               int(bool(reg)), C.byref(p), int(ndir), C.c_void_p(df_ptr or None),
                                               C.c_void_p(dalpha_ptr or None), C.c_void_p(du_ptr)))

    def jvp_each(self, u, alphas, df=None, dalphas=None, reg=False, **kw):
        """jvp with image k's own parameter alphas[k] (bpltv_jvp_each).  dalphas: shaped like alphas, or with a leading
        K; df and the result as in jvp."""
        a, am, an = self._each_arg(alphas)
        df, dalphas, K, batched = self._tangents("jvp_each", df, dalphas, a.shape)
        p = self.params(**kw)
        u = self._batch(u, "u")
        du = np.empty((K, self.O, self.N, self.M))
        self._check(self._lib.bpltv_jvp_each(self._h, _ptr(u), _ptr(a), am, an, int(bool(reg)), C.byref(p), K,
                                             _ptr(df) if df is not None else None,
                                             _ptr(dalphas) if dalphas is not None else None, _ptr(du)))
        return du if batched else du[0]

    def jvp_each_device(self, u_ptr, alphas_ptr, am, an, df_ptr, dalphas_ptr, du_ptr, ndir=1, reg=False, **kw):
        """bpltv_jvp_each_device: as jvp_device with O parameter blocks (O*am*an doubles) and ndir*O tangent blocks."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_jvp_each_device(self._h, C.c_void_p(u_ptr), C.c_void_p(alphas_ptr), int(am),
                                                    int(an), int(bool(reg)), C.byref(p), int(ndir),
                                                    C.c_void_p(df_ptr or None), C.c_void_p(dalphas_ptr or None),
                                                    C.c_void_p(du_ptr)))

    def gauss_newton(self, u, ubar, x, reg=False, **kw):
        """Gauss-Newton model of 0.5||u(x) - ubar||^2 (bpltv_gauss_newton): (grad, H) with grad = J^T (u - ubar) shaped
        like x and H = J^T J of shape (P, P), P = x.size, ordered as x's column-major (Julia) entries -- numpy's
        x.ravel().  A float or an (n, m) patch parameter with at most 16 entries."""
        a, am, an, scalar = _alpha_arg(x)
        p = self.params(**kw)
        u = self._batch(u, "u")
        ubar = self._batch(ubar, "ubar")
        P = am * an
        grad, H = np.empty(P), np.empty((P, P))
        self._check(self._lib.bpltv_gauss_newton(self._h, _ptr(u), _ptr(ubar), _ptr(a), am, an, int(bool(reg)),
                                                 C.byref(p), _ptr(grad), _ptr(H)))
        return (float(grad[0]) if scalar else grad.reshape(an, am)), H

    # -- forward mode through the iterations (bpltv_unrolled_jvp / bpltv_unrolled_gauss_newton) ---------------
    def unrolled_jvp(self, x, df=None, dalpha=None, want_u=False, **kw):
        """Jacobian-vector product of the maxiter-step map u = unrolled_denoise(x) of the resident f (bpltv_unrolled_jvp):
        a tangent sweep through the iterations, no tape -- the linear map whose transpose unrolled_vjp computes.  df:
        (O, N, M), or (K, O, N, M) for K directions; dalpha: shaped like x, or with a leading K; either may be None
        (zero), not both.  Returns du of shape (O, N, M), or (K, O, N, M) when a leading K was given; with want_u,
        (du, u) with u = denoise(x) bit for bit."""
        a, am, an, scalar = _alpha_arg(x)
        df, dalpha, K, batched = self._tangents("unrolled_jvp", df, dalpha, () if scalar else (an, am))
        p = self.params(**kw)
        du = np.empty((K, self.O, self.N, self.M))
        u = np.empty((self.O, self.N, self.M)) if want_u else None
        self._check(self._lib.bpltv_unrolled_jvp(self._h, _ptr(a), am, an, C.byref(p), K,
                                                 _ptr(df) if df is not None else None,
                                                 _ptr(dalpha) if dalpha is not None else None, _ptr(du),
                                                 _ptr(u) if want_u else None))
        du = du if batched else du[0]
        return (du, u) if want_u else du

    def unrolled_jvp_device(self, alpha_ptr, am, an, df_ptr, dalpha_ptr, du_ptr, u_ptr=None, ndir=1, **kw):
        """bpltv_unrolled_jvp_device: the parameter (am*an doubles), df and du (ndir*M*N*O), dalpha (ndir*am*an) and u
        (M*N*O) all resident in HBM (raw device pointers); either tangent pointer may be 0 / None, not both; u_ptr may
        be 0 / None."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_unrolled_jvp_device(self._h, C.c_void_p(alpha_ptr), int(am), int(an), C.byref(p),
                                                        int(ndir), C.c_void_p(df_ptr or None),
                                                        C.c_void_p(dalpha_ptr or None), C.c_void_p(du_ptr),
                                                        C.c_void_p(u_ptr or None)))

    def unrolled_gauss_newton(self, x, **kw):
        """Gauss-Newton model of the maxiter-step loss 0.5||u_K(x) - ubar||^2 on the resident dataset
        (bpltv_unrolled_gauss_newton): (cost, grad, H) with grad = J^T (u_K - ubar) shaped like x and H = J^T J of shape
        (P, P), P = x.size, ordered as numpy's x.ravel(); J by P tangent sweeps.  A float or an (n, m) patch parameter
        with at most 16 entries."""
        a, am, an, scalar = _alpha_arg(x)
        p = self.params(**kw)
        P = am * an
        cost, grad, H = C.c_double(0.0), np.empty(P), np.empty((P, P))
        self._check(self._lib.bpltv_unrolled_gauss_newton(self._h, _ptr(a), am, an, C.byref(p),
                                                          C.byref(cost), _ptr(grad), _ptr(H)))
        return float(cost.value), (float(grad[0]) if scalar else grad.reshape(an, am)), H

    # -- forward mode through the weighted iterations (bpltv_weighted_unrolled_jvp / _gauss_newton) -----------
    def _weighted_jvp(self, what, fn, x, w, df, dalpha, dw, want_u, kw):
        """weighted_unrolled_jvp and its TV-L1 / TV-KL twins: the tangents as stacks of K directions, one call of fn."""
        a, am, an, scalar = _alpha_arg(x)
        wa, wo = self._weight(w)
        if df is None and dalpha is None and dw is None:
            raise ValueError("%s: df, dalpha and dw are all None" % what)
        K, batched = None, False
        if df is not None or dalpha is not None:
            df, dalpha, K, batched = self._tangents(what, df, dalpha, () if scalar else (an, am))
        if dw is not None:
            dw = np.ascontiguousarray(dw, dtype=np.float64)
            if dw.shape == wa.shape:
                dw = dw[None]
            elif dw.shape[1:] == wa.shape:
                batched = True
            else:
                raise ValueError("%s: dw has shape %s, expected %s or (K,) + %s" % (what, dw.shape, wa.shape, wa.shape))
            if K is None:
                K = dw.shape[0]
            if K < 1 or dw.shape[0] != K:
                raise ValueError("%s: the tangents hold different numbers of directions" % what)
        p = self.params(**kw)
        du = np.empty((K, self.O, self.N, self.M))
        u = np.empty((self.O, self.N, self.M)) if want_u else None
        self._check(fn(self._h, _ptr(wa), wo, _ptr(a), am, an, C.byref(p), K,
                       _ptr(df) if df is not None else None,
                       _ptr(dalpha) if dalpha is not None else None,
                       _ptr(dw) if dw is not None else None, _ptr(du),
                       _ptr(u) if want_u else None))
        du = du if batched else du[0]
        return (du, u) if want_u else du

    def _weighted_jvp_device(self, fn, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr, dw_ptr, du_ptr, u_ptr, ndir, kw):
        p = self.params(**kw)
        self._check(fn(self._h, C.c_void_p(w_ptr), int(wo), C.c_void_p(alpha_ptr), int(am), int(an), C.byref(p), int(ndir),
                       C.c_void_p(df_ptr or None), C.c_void_p(dalpha_ptr or None), C.c_void_p(dw_ptr or None),
                       C.c_void_p(du_ptr), C.c_void_p(u_ptr or None)))

    def _weighted_gauss_newton(self, fn, x, w, kw):
        a, am, an, scalar = _alpha_arg(x)
        wa, wo = self._weight(w)
        p = self.params(**kw)
        P = am * an
        cost, grad, H = C.c_double(0.0), np.empty(P), np.empty((P, P))
        self._check(fn(self._h, _ptr(wa), wo, _ptr(a), am, an, C.byref(p), C.byref(cost), _ptr(grad), _ptr(H)))
        return float(cost.value), (float(grad[0]) if scalar else grad.reshape(an, am)), H

    def weighted_unrolled_jvp(self, x, w, df=None, dalpha=None, dw=None, want_u=False, **kw):
        """Jacobian-vector product of the maxiter-step map u = weighted_unrolled_denoise(x, w) of the resident f
        (bpltv_weighted_unrolled_jvp): a tangent sweep through the weighted iterations, no tape -- the linear map whose
        transpose weighted_unrolled_vjp computes; w >= 0, zeros allowed (a mask).  df: (O, N, M), or (K, O, N, M) for K
        directions; dalpha: shaped like x, or with a leading K; dw: shaped like w, or with a leading K; any may be None
        (zero), not all three.  Returns du of shape (O, N, M), or (K, O, N, M) when a leading K was given; with want_u,
        (du, u) with u = weighted_denoise(x, w) bit for bit.  The step table (gamma = min w) is held fixed."""
        return self._weighted_jvp("weighted_unrolled_jvp", self._lib.bpltv_weighted_unrolled_jvp, x, w, df, dalpha, dw, want_u, kw)

    def weighted_unrolled_jvp_device(self, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr, dw_ptr, du_ptr, u_ptr=None,
                                     ndir=1, **kw):
        """bpltv_weighted_unrolled_jvp_device: w (wo planes), the parameter (am*an doubles), df and du (ndir*M*N*O), dalpha
        (ndir*am*an), dw (ndir*M*N*wo) and u (M*N*O) all resident in HBM (raw device pointers); any tangent pointer may be
        0 / None, not all three; u_ptr may be 0 / None."""
        self._weighted_jvp_device(self._lib.bpltv_weighted_unrolled_jvp_device, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr,
                                  dw_ptr, du_ptr, u_ptr, ndir, kw)

    def weighted_unrolled_gauss_newton(self, x, w, **kw):
        """Gauss-Newton model of the maxiter-step loss 0.5||u_K(x) - ubar||^2 of the weighted iterations on the resident
        dataset (bpltv_weighted_unrolled_gauss_newton): (cost, grad, H) as unrolled_gauss_newton's, J by P tangent sweeps
        in the parameter.  A float or an (n, m) patch parameter with at most 16 entries; w >= 0, zeros allowed."""
        return self._weighted_gauss_newton(self._lib.bpltv_weighted_unrolled_gauss_newton, x, w, kw)

    # -- forward mode through the TV-L1 and the TV-KL iterations (bpltv_lone_unrolled_jvp, bpltv_kl_unrolled_jvp) -----
    def l1_unrolled_jvp(self, x, w, df=None, dalpha=None, dw=None, want_u=False, **kw):
        """Jacobian-vector product of the maxiter-step map u = l1_denoise(x, w) of the resident f (bpltv_lone_unrolled_jvp): a
        tangent sweep through the TV-L1 iterations, no tape -- the linear map whose transpose l1_unrolled_vjp computes, with
        its conventions (a pixel held at f moves with f alone).  Arguments and result as weighted_unrolled_jvp; with want_u,
        (du, u) with u = l1_denoise(x, w) bit for bit."""
        return self._weighted_jvp("l1_unrolled_jvp", self._lib.bpltv_lone_unrolled_jvp, x, w, df, dalpha, dw, want_u, kw)

    def l1_unrolled_jvp_device(self, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr, dw_ptr, du_ptr, u_ptr=None, ndir=1, **kw):
        """bpltv_lone_unrolled_jvp_device: everything resident in HBM (raw device pointers), as weighted_unrolled_jvp_device."""
        self._weighted_jvp_device(self._lib.bpltv_lone_unrolled_jvp_device, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr,
                                  dw_ptr, du_ptr, u_ptr, ndir, kw)

    def l1_unrolled_gauss_newton(self, x, w, **kw):
        """Gauss-Newton model of the maxiter-step loss 0.5||u_K(x) - ubar||^2 of the TV-L1 iterations on the resident dataset
        (bpltv_lone_unrolled_gauss_newton): (cost, grad, H) as weighted_unrolled_gauss_newton's."""
        return self._weighted_gauss_newton(self._lib.bpltv_lone_unrolled_gauss_newton, x, w, kw)

    def kl_unrolled_jvp(self, x, w, df=None, dalpha=None, dw=None, want_u=False, **kw):
        """Jacobian-vector product of the maxiter-step map u = kl_denoise(x, w) of the resident f >= 0 (bpltv_kl_unrolled_jvp): a
        tangent sweep through the TV-KL iterations, no tape -- the linear map whose transpose kl_unrolled_vjp computes, with
        its convention (a pixel clamped at zero passes nothing).  Arguments and result as weighted_unrolled_jvp; with want_u,
        (du, u) with u = kl_denoise(x, w) bit for bit."""
        return self._weighted_jvp("kl_unrolled_jvp", self._lib.bpltv_kl_unrolled_jvp, x, w, df, dalpha, dw, want_u, kw)

    def kl_unrolled_jvp_device(self, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr, dw_ptr, du_ptr, u_ptr=None, ndir=1, **kw):
        """bpltv_kl_unrolled_jvp_device: everything resident in HBM (raw device pointers), as weighted_unrolled_jvp_device."""
        self._weighted_jvp_device(self._lib.bpltv_kl_unrolled_jvp_device, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr,
                                  dw_ptr, du_ptr, u_ptr, ndir, kw)

    def kl_unrolled_gauss_newton(self, x, w, **kw):
        """Gauss-Newton model of the maxiter-step loss 0.5||u_K(x) - ubar||^2 of the TV-KL iterations on the resident dataset
        (bpltv_kl_unrolled_gauss_newton): (cost, grad, H) as weighted_unrolled_gauss_newton's."""
        return self._weighted_gauss_newton(self._lib.bpltv_kl_unrolled_gauss_newton, x, w, kw)

    # -- one parameter per image (bpltv_denoise_each / bpltv_vjp_each) ---------------------------------------
    def _each_arg(self, alphas):
        """alphas: (O,) scalars or (O, n, m) blocks (numpy (n, m) == Julia m x n), one per image."""
        a = np.ascontiguousarray(alphas, dtype=np.float64)
        if a.ndim == 1:
            am, an = 1, 1
        elif a.ndim == 3:
            an, am = a.shape[1], a.shape[2]
        else:
            raise ValueError("alphas must have shape (O,) or (O, n, m), got %s" % (a.shape,))
        if a.shape[0] != self.O:
            raise ValueError("alphas has %d blocks, the handle holds O=%d images" % (a.shape[0], self.O))
        return a, am, an

    def denoise_each(self, alphas, fetch=True, **kw):
        """denoise with image k's own parameter alphas[k] (bpltv_denoise_each); u[k] is bitwise a one-image solve of
        (f[k], alphas[k])."""
        a, am, an = self._each_arg(alphas)
        p = self.params(**kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_denoise_each(self._h, _ptr(a), am, an, C.byref(p), _ptr(u) if fetch else None))
        return u

    def denoise_each_device(self, alphas_ptr, am=1, an=1, **kw):
        """bpltv_denoise_each_device: O parameter blocks (O*am*an doubles, block k column major at k*am*an) resident in
        HBM at `alphas_ptr`; the result stays on the device (u_device_ptr / copy_u_device)."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_denoise_each_device(self._h, C.c_void_p(alphas_ptr), int(am), int(an), C.byref(p)))

    def vjp_each(self, u, alphas, gu, reg=False, want_f=True, want_alpha=True, **kw):
        """vjp with image k's own parameter alphas[k] (bpltv_vjp_each): (grad_f, grad_alphas).  grad_alphas has the shape
        of alphas; grad_alphas[k] is image k's term alone, not summed over the images."""
        if not (want_f or want_alpha):
            raise ValueError("vjp_each: want_f and want_alpha are both False")
        a, am, an = self._each_arg(alphas)
        p = self.params(**kw)
        u = self._batch(u, "u")
        gu = self._batch(gu, "gu")
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(a.shape) if want_alpha else None
        self._check(self._lib.bpltv_vjp_each(self._h, _ptr(u), _ptr(a), am, an, int(bool(reg)), C.byref(p), _ptr(gu),
                                             _ptr(gf) if want_f else None, _ptr(ga) if want_alpha else None))
        return gf, ga

    def vjp_each_device(self, u_ptr, alphas_ptr, am, an, gu_ptr, grad_f_ptr, grad_alphas_ptr, reg=False, **kw):
        """bpltv_vjp_each_device: u, gu and grad_f (M*N*O doubles), the O parameter blocks and their O gradients
        (O*am*an doubles each) all resident in HBM; either output pointer may be 0 / None, not both."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_vjp_each_device(self._h, C.c_void_p(u_ptr), C.c_void_p(alphas_ptr), int(am),
                                                    int(an), int(bool(reg)), C.byref(p), C.c_void_p(gu_ptr),
                                                    C.c_void_p(grad_f_ptr or None), C.c_void_p(grad_alphas_ptr or None)))

    # -- one parameter per image through the iterations (bpltv_unrolled_*_each) ----------------------------------
    def unrolled_denoise_each(self, alphas, fetch=True, **kw):
        """unrolled_denoise with image k's own parameter alphas[k] (bpltv_unrolled_denoise_each): denoise_each's u bit for
        bit, and the handle's tape, recorded per image, for unrolled_vjp_each with the same alphas and params."""
        a, am, an = self._each_arg(alphas)
        p = self._taped_params(kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_unrolled_denoise_each(self._h, _ptr(a), am, an, C.byref(p),
                                                          _ptr(u) if fetch else None))
        return u

    def unrolled_denoise_each_device(self, alphas_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_unrolled_denoise_each_device: O parameter blocks (O*am*an doubles, block k column major at k*am*an)
        resident in HBM, the result left there; tape_ptr as in unrolled_denoise_device."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_unrolled_denoise_each_device(self._h, C.c_void_p(alphas_ptr), int(am), int(an),
                                                                 C.byref(p), C.c_void_p(tape_ptr or None)))

    def unrolled_vjp_each(self, alphas, gu, want_f=True, want_alpha=True, **kw):
        """unrolled_vjp with image k's own parameter alphas[k], over the handle's per-image tape
        (bpltv_unrolled_vjp_each): (grad_f, grad_alphas).  grad_alphas has the shape of alphas; grad_alphas[k] is image
        k's term alone, not summed over the images."""
        if not (want_f or want_alpha):
            raise ValueError("unrolled_vjp_each: want_f and want_alpha are both False")
        a, am, an = self._each_arg(alphas)
        p = self._taped_params(kw)
        gu = self._batch(gu, "gu")
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(a.shape) if want_alpha else None
        self._check(self._lib.bpltv_unrolled_vjp_each(self._h, _ptr(a), am, an, C.byref(p), _ptr(gu),
                                                      _ptr(gf) if want_f else None, _ptr(ga) if want_alpha else None))
        return gf, ga

    def unrolled_vjp_each_device(self, tape_ptr, alphas_ptr, am, an, gu_ptr, grad_f_ptr, grad_alphas_ptr, **kw):
        """bpltv_unrolled_vjp_each_device: as unrolled_vjp_device with O parameter blocks and their O gradients (O*am*an
        doubles each) resident in HBM; either output pointer may be 0 / None, not both."""
        p = self._taped_params(kw)
        self._check(self._lib.bpltv_unrolled_vjp_each_device(self._h, C.c_void_p(tape_ptr or None),
                                                             C.c_void_p(alphas_ptr), int(am), int(an), C.byref(p),
                                                             C.c_void_p(gu_ptr), C.c_void_p(grad_f_ptr or None),
                                                             C.c_void_p(grad_alphas_ptr or None)))

    def unrolled_jvp_each(self, alphas, df=None, dalphas=None, want_u=False, **kw):
        """unrolled_jvp with image k's own parameter alphas[k] (bpltv_unrolled_jvp_each).  dalphas: shaped like alphas,
        or with a leading K; df, want_u and the result as in unrolled_jvp (u = denoise_each(alphas) bit for bit)."""
        a, am, an = self._each_arg(alphas)
        df, dalphas, K, batched = self._tangents("unrolled_jvp_each", df, dalphas, a.shape)
        p = self.params(**kw)
        du = np.empty((K, self.O, self.N, self.M))
        u = np.empty((self.O, self.N, self.M)) if want_u else None
        self._check(self._lib.bpltv_unrolled_jvp_each(self._h, _ptr(a), am, an, C.byref(p), K,
                                                      _ptr(df) if df is not None else None,
                                                      _ptr(dalphas) if dalphas is not None else None, _ptr(du),
                                                      _ptr(u) if want_u else None))
        du = du if batched else du[0]
        return (du, u) if want_u else du

    def unrolled_jvp_each_device(self, alphas_ptr, am, an, df_ptr, dalphas_ptr, du_ptr, u_ptr=None, ndir=1, **kw):
        """bpltv_unrolled_jvp_each_device: as unrolled_jvp_device with O parameter blocks (O*am*an doubles) and ndir*O
        tangent blocks, direction first."""
        p = self.params(**kw)
        self._check(self._lib.bpltv_unrolled_jvp_each_device(self._h, C.c_void_p(alphas_ptr), int(am), int(an),
                                                             C.byref(p), int(ndir), C.c_void_p(df_ptr or None),
                                                             C.c_void_p(dalphas_ptr or None), C.c_void_p(du_ptr),
                                                             C.c_void_p(u_ptr or None)))

    # -- one block of three weights per image (bpltv_sumregs_denoise_each / bpltv_sumregs_vjp_each) ---------------
    def _sr_each_arg(self, alphas):
        """alphas: (O, 3) vectors or (O, 3, n, m) patch / map blocks (the layout of sumregs_evaluate per block), one per
        image."""
        a = np.ascontiguousarray(alphas, dtype=np.float64)
        if a.ndim == 2 and a.shape[1] == 3:
            am, an = 1, 1
        elif a.ndim == 4 and a.shape[1] == 3:
            an, am = a.shape[2], a.shape[3]
        else:
            raise ValueError("alphas must have shape (O, 3) or (O, 3, n, m), got %s" % (a.shape,))
        if a.shape[0] != self.O:
            raise ValueError("alphas has %d blocks, the handle holds O=%d images" % (a.shape[0], self.O))
        return a, am, an

    def sumregs_denoise_each(self, alphas, fetch=True, **kw):
        """sumregs_denoise with image k's own three weights alphas[k] (bpltv_sumregs_denoise_each); u[k] is bitwise a
        one-image solve of (f[k], alphas[k])."""
        a, am, an = self._sr_each_arg(alphas)
        p = self.params(_sumregs=True, **kw)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_sumregs_denoise_each(self._h, _ptr(a), am, an, C.byref(p),
                                                         _ptr(u) if fetch else None))
        return u

    def sumregs_denoise_each_device(self, alphas_ptr, am=1, an=1, **kw):
        """bpltv_sumregs_denoise_each_device: O parameter blocks (O*3*am*an doubles, a C-contiguous (O, 3, an, am)
        array) resident in HBM at `alphas_ptr`; the result stays on the device (u_device_ptr / copy_u_device)."""
        p = self.params(_sumregs=True, **kw)
        self._check(self._lib.bpltv_sumregs_denoise_each_device(self._h, C.c_void_p(alphas_ptr), int(am), int(an),
                                                                C.byref(p)))

    def sumregs_vjp_each(self, u, alphas, gu, reg=False, want_f=True, want_alpha=True, **kw):
        """sumregs_vjp with image k's own block alphas[k] (bpltv_sumregs_vjp_each): (grad_f, grad_alphas).  grad_alphas
        has the shape of alphas; grad_alphas[k] is image k's term alone, not summed over the images."""
        if not (want_f or want_alpha):
            raise ValueError("sumregs_vjp_each: want_f and want_alpha are both False")
        a, am, an = self._sr_each_arg(alphas)
        u = self._batch(u, "u")
        gu = self._batch(gu, "gu")
        p = self.params(_sumregs=True, **kw)
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(a.shape) if want_alpha else None
        self._check(self._lib.bpltv_sumregs_vjp_each(self._h, _ptr(u), _ptr(a), am, an, int(bool(reg)), C.byref(p),
                                                     _ptr(gu), _ptr(gf) if want_f else None,
                                                     _ptr(ga) if want_alpha else None))
        return gf, ga

    def sumregs_vjp_each_device(self, u_ptr, alphas_ptr, am, an, gu_ptr, grad_f_ptr, grad_alphas_ptr, reg=False, **kw):
        """bpltv_sumregs_vjp_each_device: u, gu and grad_f (M*N*O doubles), the O parameter blocks and their O gradients
        (O*3*am*an doubles each) all resident in HBM; either output pointer may be 0 / None, not both."""
        p = self.params(_sumregs=True, **kw)
        self._check(self._lib.bpltv_sumregs_vjp_each_device(self._h, C.c_void_p(u_ptr), C.c_void_p(alphas_ptr), int(am),
                                                            int(an), int(bool(reg)), C.byref(p), C.c_void_p(gu_ptr),
                                                            C.c_void_p(grad_f_ptr or None),
                                                            C.c_void_p(grad_alphas_ptr or None)))

    def sumregs_jvp_each(self, u, alphas, df=None, dalphas=None, reg=False, **kw):
        """sumregs_jvp with image k's own block alphas[k] (bpltv_sumregs_jvp_each).  dalphas: shaped like alphas, or
        with a leading K; df and the result as in sumregs_jvp."""
        a, am, an = self._sr_each_arg(alphas)
        df, dalphas, K, batched = self._tangents("sumregs_jvp_each", df, dalphas, a.shape)
        p = self.params(_sumregs=True, **kw)
        u = self._batch(u, "u")
        du = np.empty((K, self.O, self.N, self.M))
        self._check(self._lib.bpltv_sumregs_jvp_each(self._h, _ptr(u), _ptr(a), am, an, int(bool(reg)), C.byref(p), K,
                                                     _ptr(df) if df is not None else None,
                                                     _ptr(dalphas) if dalphas is not None else None, _ptr(du)))
        return du if batched else du[0]

    def sumregs_jvp_each_device(self, u_ptr, alphas_ptr, am, an, df_ptr, dalphas_ptr, du_ptr, ndir=1, reg=False, **kw):
        """bpltv_sumregs_jvp_each_device: as sumregs_jvp_device with O parameter blocks (O*3*am*an doubles) and ndir*O
        tangent blocks."""
        p = self.params(_sumregs=True, **kw)
        self._check(self._lib.bpltv_sumregs_jvp_each_device(self._h, C.c_void_p(u_ptr), C.c_void_p(alphas_ptr), int(am),
                                                            int(an), int(bool(reg)), C.byref(p), int(ndir),
                                                            C.c_void_p(df_ptr or None), C.c_void_p(dalphas_ptr or None),
                                                            C.c_void_p(du_ptr)))

    # -- reverse mode through the sum-of-regularisers iterations (bpltv_sumregs_unrolled_*) ------------------------
    def sumregs_unrolled_tape_doubles(self, **kw):
        """Doubles of the tape a sum-of-regularisers unrolled solve with these params records: 6 * maxiter * M*N*O."""
        p = self._taped_params(kw, _sumregs=True)
        n = C.c_ulonglong(0)
        self._check(self._lib.bpltv_sumregs_unrolled_tape_doubles(self._h, C.byref(p), C.byref(n)))
        return int(n.value)

    def sumregs_unrolled_denoise(self, x, fetch=True, **kw):
        """sumregs_denoise(x) with rho = 0 -- the same u bit for bit -- that also records the tape of the iterations in
        the handle, for sumregs_unrolled_vjp with the same x and params (bpltv_sumregs_unrolled_denoise)."""
        a, am, an, _ = _sr_alpha_arg(x)
        p = self._taped_params(kw, _sumregs=True)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_sumregs_unrolled_denoise(self._h, _ptr(a), am, an, C.byref(p),
                                                             _ptr(u) if fetch else None))
        return u

    def sumregs_unrolled_denoise_device(self, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_sumregs_unrolled_denoise_device: the parameter (3*am*an doubles) resident in HBM, the result left there
        (u_device_ptr / copy_u_device); tape_ptr: a caller-owned HBM buffer of sumregs_unrolled_tape_doubles(**kw)
        doubles, or None / 0 for the handle's own tape."""
        p = self._taped_params(kw, _sumregs=True)
        self._check(self._lib.bpltv_sumregs_unrolled_denoise_device(self._h, C.c_void_p(alpha_ptr), int(am), int(an),
                                                                    C.byref(p), C.c_void_p(tape_ptr or None)))

    def sumregs_unrolled_vjp(self, x, gu, want_f=True, want_alpha=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = sumregs_unrolled_denoise(x) for the cotangent gu = dL/du,
        by a reverse sweep over the handle's tape (bpltv_sumregs_unrolled_vjp): (grad_f, grad_x).  x and the params must
        be those of the solve.  gu: (O, N, M); grad_f has its shape (None unless want_f), grad_x the shape of x (None
        unless want_alpha)."""
        if not (want_f or want_alpha):
            raise ValueError("sumregs_unrolled_vjp: want_f and want_alpha are both False")
        a, am, an, vec = _sr_alpha_arg(x)
        p = self._taped_params(kw, _sumregs=True)
        gu = self._batch(gu, "gu")
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(3 * am * an) if want_alpha else None
        self._check(self._lib.bpltv_sumregs_unrolled_vjp(self._h, _ptr(a), am, an, C.byref(p), _ptr(gu),
                                                         _ptr(gf) if want_f else None,
                                                         _ptr(ga) if want_alpha else None))
        if ga is not None and not vec:
            ga = ga.reshape(3, an, am)
        return gf, ga

    def sumregs_unrolled_vjp_device(self, tape_ptr, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, **kw):
        """bpltv_sumregs_unrolled_vjp_device: the tape (None / 0: the handle's own), the parameter, gu and the outputs
        resident in HBM (raw device pointers); either output pointer may be 0 / None, not both."""
        p = self._taped_params(kw, _sumregs=True)
        self._check(self._lib.bpltv_sumregs_unrolled_vjp_device(self._h, C.c_void_p(tape_ptr or None),
                                                                C.c_void_p(alpha_ptr), int(am), int(an), C.byref(p),
                                                                C.c_void_p(gu_ptr), C.c_void_p(grad_f_ptr or None),
                                                                C.c_void_p(grad_alpha_ptr or None)))

    def sumregs_unrolled_denoise_each(self, alphas, fetch=True, **kw):
        """sumregs_unrolled_denoise with image k's own three weights alphas[k] (bpltv_sumregs_unrolled_denoise_each):
        sumregs_denoise_each's u bit for bit, and the handle's tape, recorded per image."""
        a, am, an = self._sr_each_arg(alphas)
        p = self._taped_params(kw, _sumregs=True)
        u = np.empty((self.O, self.N, self.M)) if fetch else None
        self._check(self._lib.bpltv_sumregs_unrolled_denoise_each(self._h, _ptr(a), am, an, C.byref(p),
                                                                  _ptr(u) if fetch else None))
        return u

    def sumregs_unrolled_denoise_each_device(self, alphas_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_sumregs_unrolled_denoise_each_device: O parameter blocks (a C-contiguous (O, 3, an, am) array) resident
        in HBM, the result left there; tape_ptr as in sumregs_unrolled_denoise_device."""
        p = self._taped_params(kw, _sumregs=True)
        self._check(self._lib.bpltv_sumregs_unrolled_denoise_each_device(self._h, C.c_void_p(alphas_ptr), int(am),
                                                                         int(an), C.byref(p),
                                                                         C.c_void_p(tape_ptr or None)))

    def sumregs_unrolled_vjp_each(self, alphas, gu, want_f=True, want_alpha=True, **kw):
        """sumregs_unrolled_vjp with image k's own block alphas[k], over the handle's per-image tape
        (bpltv_sumregs_unrolled_vjp_each): (grad_f, grad_alphas).  grad_alphas has the shape of alphas; grad_alphas[k]
        is image k's term alone, not summed over the images."""
        if not (want_f or want_alpha):
            raise ValueError("sumregs_unrolled_vjp_each: want_f and want_alpha are both False")
        a, am, an = self._sr_each_arg(alphas)
        p = self._taped_params(kw, _sumregs=True)
        gu = self._batch(gu, "gu")
        gf = np.empty((self.O, self.N, self.M)) if want_f else None
        ga = np.empty(a.shape) if want_alpha else None
        self._check(self._lib.bpltv_sumregs_unrolled_vjp_each(self._h, _ptr(a), am, an, C.byref(p), _ptr(gu),
                                                              _ptr(gf) if want_f else None,
                                                              _ptr(ga) if want_alpha else None))
        return gf, ga

    def sumregs_unrolled_vjp_each_device(self, tape_ptr, alphas_ptr, am, an, gu_ptr, grad_f_ptr, grad_alphas_ptr, **kw):
        """bpltv_sumregs_unrolled_vjp_each_device: as sumregs_unrolled_vjp_device with O parameter blocks and their O
        gradients (O*3*am*an doubles each) resident in HBM; either output pointer may be 0 / None, not both."""
        p = self._taped_params(kw, _sumregs=True)
        self._check(self._lib.bpltv_sumregs_unrolled_vjp_each_device(self._h, C.c_void_p(tape_ptr or None),
                                                                     C.c_void_p(alphas_ptr), int(am), int(an),
                                                                     C.byref(p), C.c_void_p(gu_ptr),
                                                                     C.c_void_p(grad_f_ptr or None),
                                                                     C.c_void_p(grad_alphas_ptr or None)))

    def sweep(self, alphas, fetch_u=False, **kw):
        """costs[k] = 0.5*||denoise(f, alphas[k]) - ubar||^2 for K parameters in one batched solve
        (generate_cost / generate_2d_cost, /root/reference/src/BPLDenoising.jl:92-111,136-158).
        alphas: (K,) scalars or (K, n, m) parameter matrices."""
        a = np.ascontiguousarray(alphas, dtype=np.float64)
        if a.ndim == 1:
            K, am, an = a.shape[0], 1, 1
        elif a.ndim == 3:
            K, an, am = a.shape
        else:
            raise ValueError("alphas must have shape (K,) or (K, n, m)")
        p = self.params(**kw)
        costs = np.empty(K)
        u = np.empty((K, self.O, self.N, self.M)) if fetch_u else None
        self._check(self._lib.bpltv_sweep(self._h, _ptr(a), K, am, an, C.byref(p), _ptr(costs),
                                          _ptr(u) if fetch_u else None))
        return (costs, u) if fetch_u else costs

    def sumregs_sweep(self, alphas, fetch_u=False, **kw):
        """costs[k] = 0.5*||sumregs_denoise(f, alphas[k]) - ubar||^2 for K parameter triples in one batched solve
        (generate_cost with denoise_function = sumregs_denoise: the reference's src/BPLDenoising.jl:92-158 and
        src/SumRegsLearningFunction.jl:38-85).  alphas: (K, 3) vectors or (K, 3, n, m) patch / map blocks
        (the layout of sumregs_evaluate per block)."""
        a = np.ascontiguousarray(alphas, dtype=np.float64)
        if a.ndim == 2 and a.shape[1] == 3:
            K, am, an = a.shape[0], 1, 1
        elif a.ndim == 4 and a.shape[1] == 3:
            K, _, an, am = a.shape
        else:
            raise ValueError("alphas must have shape (K, 3) or (K, 3, n, m), got %s" % (a.shape,))
        p = self.params(_sumregs=True, **kw)
        costs = np.empty(K)
        u = np.empty((K, self.O, self.N, self.M)) if fetch_u else None
        self._check(self._lib.bpltv_sumregs_sweep(self._h, _ptr(a), K, am, an, C.byref(p), _ptr(costs),
                                                  _ptr(u) if fetch_u else None))
        return (costs, u) if fetch_u else costs

    def per_image(self):
        """(O, 1 + am*an) rows [cost_k, grad_k...] of the last evaluate (scalar / patch parameter): the totals
        are these rows added in image order."""
        out = np.empty((self.O, 1 + self._last_npar))
        self._check(self._lib.bpltv_per_image(self._h, _ptr(out)))
        return out

    def u_device_ptr(self):
        p = C.c_void_p()
        self._check(self._lib.bpltv_u_device(self._h, C.byref(p)))
        return p.value

    def copy_u_device(self, dst_ptr):
        self._check(self._lib.bpltv_copy_u_device(self._h, C.c_void_p(dst_ptr)))

    def duality_gap(self):
        g = np.empty(self.O)
        self._check(self._lib.bpltv_duality_gap(self._h, _ptr(g)))
        return g

    def grad_fwd(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        d1 = np.empty_like(x); d2 = np.empty_like(x)
        self._check(self._lib.bpltv_grad_fwd(self._h, _ptr(x), _ptr(d1), _ptr(d2)))
        return d1, d2

    def grad_fwd_adjoint(self, y1, y2):
        y1 = np.ascontiguousarray(y1, dtype=np.float64)
        y2 = np.ascontiguousarray(y2, dtype=np.float64)
        out = np.empty_like(y1)
        self._check(self._lib.bpltv_grad_fwd_adjoint(self._h, _ptr(y1), _ptr(y2), _ptr(out)))
        return out

    def set_option(self, name, value):
        """bpltv_set_option: test / measurement aids (include/bpltv.h), e.g. set_option("adjoint_budget_mb", 40)."""
        self._check(self._lib.bpltv_set_option(self._h, name.encode(), float(value)))

    def stats(self):
        s = _lib.BpltvStats()
        self._check(self._lib.bpltv_stats(self._h, C.byref(s)))
        return s.as_dict()


# ---------------------------------------------------------------------------------------------
# Reference-named entry points.  The solver (and the dataset upload) is cached per dataset object,
# because bilevel_learn passes the same `ds` to every evaluation (/root/reference/src/TRBox.jl:210,227).
# ---------------------------------------------------------------------------------------------
_cache = {}
_devices = {"ngpus": None, "devices": None}


def use_devices(ngpus=None, devices=None):
    """Devices behind the reference-named entry points below: None (default) = one GPU; `ngpus` = one in-library handle
    over that many devices (bpltv_create_multi: images sharded for evaluate / denoise, and -- a dataset with fewer
    images than devices, the reference's default num_samples = 1 -- the parameters of a sweep split over replicas);
    `devices` = explicit placement (bpltv_create_sharded; a repeated device rehearses the path on one GPU).  The
    environment variable BPLTV_NGPUS sets the same default the Julia glue reads."""
    new = {"ngpus": None if ngpus is None else int(ngpus), "devices": None if devices is None else [int(d) for d in devices]}
    if new != _devices:
        clear_cache()
        _devices.update(new)


def _device_kwargs():
    if _devices["devices"] is not None:
        return {"devices": _devices["devices"]}
    if _devices["ngpus"] is not None:
        return {"ngpus": _devices["ngpus"]}
    import os
    e = os.environ.get("BPLTV_NGPUS")
    return {"ngpus": int(e)} if e and int(e) != 1 else {}


def _fingerprint(a):
    """Cheap content check of a dataset array (two memory-bound passes, ~0.1 ms for 10x128x128): catches
    in-place edits of an array the cache already holds."""
    a = np.asarray(a)
    # plain numpy reductions, no BLAS call: np.vdot wakes the BLAS thread pool, whose spinning workers cost the calling
    # process tens of milliseconds of stalls per evaluation on a CPU-quota'd box (measured: 7 ms -> 30-80 ms per evaluate)
    return (a.shape, float(a.sum()), float(np.square(a).sum()))


def _solver_for(ubar, f):
    """The solver (and the dataset upload) cached per dataset.  The cache keys on the CALLER's objects --
    not on the `[None]` / `asarray` views made here, which are new objects on every call -- keeps references
    to them (so a later array cannot reuse their id()), and re-uploads when their content fingerprint
    changed (in-place edits between calls)."""
    key = (id(ubar), id(f), repr(_device_kwargs()))
    fp = (None if ubar is None else _fingerprint(ubar), _fingerprint(f))
    ent = _cache.get("s")
    if ent is not None and ent["key"] == key and ent["fp"] == fp:
        return ent["solver"]
    f3 = np.asarray(f, dtype=np.float64)
    if f3.ndim == 2:
        f3 = f3[None]
    u3 = f3 if ubar is None else np.asarray(ubar, dtype=np.float64)
    if u3.ndim == 2:
        u3 = u3[None]
    O, N, M = f3.shape
    s = ent["solver"] if ent is not None else None
    if s is None or (s.M, s.N, s.O) != (M, N, O):
        if s is not None:
            s.close()
        s = TVSolver(M, N, O, **_device_kwargs())
    s.set_data(u3, f3)
    _cache["s"] = {"key": key, "fp": fp, "solver": s, "refs": (ubar, f)}
    return s


def clear_cache():
    """Drop the cached solver (frees its HBM)."""
    ent = _cache.pop("s", None)
    if ent is not None:
        ent["solver"].close()


def tv_op_learning_function(x, data, Δ, Δt=1e-6, **kwargs):
    """(u, cost, grad) -- /root/reference/src/TVLearningFunctionVec.jl:14-27.

    data = (ubar, f); grad has the type/shape of x (float for scalar x, (n, m) array otherwise)."""
    ubar, f = data[0], data[1]
    s = _solver_for(ubar, f)
    return s.evaluate(x, Δ, delta_t=Δt, **kwargs)


def denoise(data, x, op=None, **kwargs):
    """u = denoise(f, x, op; kwargs...) -- /root/reference/src/TVLearningFunctionVec.jl:45-70.
    The array-x method of the reference takes no kwargs (:57); they are accepted here for both."""
    if op is not None and not isinstance(op, FwdGradientOp):
        raise TypeError("only FwdGradientOp is supported on this path")
    s = _solver_for(None, data)
    return s.denoise(x, **kwargs)


def sumregs_learning_function(x, data, Δ, Δt=1e-3, **kwargs):
    """(u, cost, grad) -- /root/reference/src/SumRegsLearningFunction.jl:8-36.  x: (3,) or (3, n, m)."""
    s = _solver_for(data[0], data[1])
    return s.sumregs_evaluate(x, Δ, delta_t=Δt, **kwargs)


def sumregs_denoise(data, x, op1=None, op2=None, op3=None, pOp=None, **kwargs):
    """u = sumregs_denoise(f, x, op1, op2, op3[, pOp]) -- /root/reference/src/SumRegsLearningFunction.jl:38-85 (the
    operators are fixed on this path: forward, backward, centred differences)."""
    s = _solver_for(None, data)
    return s.sumregs_denoise(x, **kwargs)


def TVDenoise(data, parameter, **kwargs):
    """/root/reference/src/BPLDenoising.jl:41-82: the same solve with maxiter = 10000."""
    kwargs.setdefault("maxiter", 10000)
    return denoise(data, parameter, FwdGradientOp(), **kwargs)


def generate_cost(data, parameters, denoise_function=None, **kwargs):
    """cost curve over a parameter range -- /root/reference/src/BPLDenoising.jl:92-111
    (`generate_cost`: loop of denoise_function + L2CostFunction), as ONE batched solve.
    data = (ubar, f).  denoise_function None / TVDenoise (maxiter = 10000): parameters (K,) scalars or (K, n, m)
    matrices (generate_2d_cost: (K, 1, 2)).  denoise_function = sumregs_denoise (maxiter = 5000, as sumregs_denoise):
    parameters (K, 3) triples or (K, 3, n, m) blocks."""
    if denoise_function is None or denoise_function is TVDenoise:
        kwargs.setdefault("maxiter", 10000)
        s = _solver_for(data[0], data[1])
        return s.sweep(parameters, **kwargs)
    if denoise_function is sumregs_denoise:
        s = _solver_for(data[0], data[1])
        return s.sumregs_sweep(parameters, **kwargs)
    raise TypeError("generate_cost: denoise_function must be TVDenoise or sumregs_denoise (the batched sweeps), got %r"
                    % (denoise_function,))


def L2CostFunction(u, true_):
    """0.5*norm2^2(u - true) -- /root/reference/src/BPLDenoising.jl:84-86 (host arithmetic on
    results already fetched; inside evaluate the loss is reduced on the GPU)."""
    d = np.asarray(u, dtype=np.float64) - np.asarray(true_, dtype=np.float64)
    return 0.5 * float(np.sum(d * d))


for _name in [n for n in vars(TVSolver) if re.search(r"unrolled_(tape_doubles|denoise|vjp)", n)]:
    setattr(TVSolver, _name, _restores_full_tape(getattr(TVSolver, _name)))
del _name
