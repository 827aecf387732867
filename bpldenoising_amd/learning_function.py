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
import math
import typing
import numpy as np

from . import _lib

_dp = C.POINTER(C.c_double)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def _opt(a):
    """A host array an entry may do without: NULL for None."""
    return _ptr(a) if a is not None else None


def _dev(ptr):
    """A device address an entry may do without: NULL for 0 / None."""
    return C.c_void_p(ptr or None)


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

    # -- the cores ---------------------------------------------------------------------
    # Every public solve, vjp, jvp and gauss_newton method below is one of these with a row of the _Model table under the class:
    # the row says which entries to call and what their argument lists splice in, the public method keeps name, signature and text.
    def _param(self, row, x):
        """(a, am, an, scalar) by row's parser; scalar: a TV float, whose gradient goes back as a float."""
        if row.each:
            return row.parse(self, x) + (False,)
        a, am, an, one = row.parse(x)
        return a, am, an, one and row.slices == 1

    def _call(self, row, op, p, alpha, am, an, tail, lead=(), w=None, wo=None, channels=None, reg=None, device=False):
        """One call of row's entry `op`.  Every entry splices its arguments in the same places: the handle, [channels], the
        leading arrays (u, f, ubar or the tape), [w, wo], alpha, am, an, [reg], the params, then the entry's own tail.  w and
        alpha go as double pointers from the host and as addresses with device=True; lead and tail come converted."""
        conv = C.c_void_p if device else _ptr
        args = [self._h]
        if row.channels:
            args.append(int(channels))
        args += lead
        if row.w:
            args += [conv(w), int(wo)]
        args += [conv(alpha), int(am), int(an)]
        if reg is not None:
            args.append(int(bool(reg)))
        args.append(C.byref(p))
        args += tail
        self._check(getattr(self._lib, row.entry(op, device))(*args))

    def _taped_params(self, row, kw):
        """(params, spacing set): params(**kw), for a taped row without checkpoint_every=, which becomes the handle's
        tape_checkpoint option right here, before the ABI call; absent means 0, so a handle shared between calls never inherits
        a spacing.  The caller's finally hands `spacing set` to _full_tape, so the handle keeps none for direct ABI calls either."""
        if not row.taped:
            return self.params(_sumregs=row.sumregs, **kw), False
        c = kw.pop("checkpoint_every", None)
        p = self.params(_sumregs=row.sumregs, **kw)
        self.set_option("tape_checkpoint", 0 if c is None else c)
        return p, bool(c)

    def _full_tape(self, spacing_set):
        if spacing_set and self._h:
            self._lib.bpltv_set_option(self._h, b"tape_checkpoint", 0.0)

    def _like(self, g, a, scalar):
        """A gradient in the library's flat layout as the type / shape of the parameter."""
        if g is None:
            return None
        if scalar:
            return float(g[0])
        return g if g.shape == a.shape else g.reshape(a.shape)

    def _solve(self, row, x, fetch, kw, w=None, channels=None):
        """<row>_denoise: u (None unless fetch); a taped row also records the tape in the handle."""
        a, am, an, _ = self._param(row, x)
        wa, wo = self._weight(w) if row.w else (None, None)
        p, spacing_set = self._taped_params(row, kw)
        try:
            u = np.empty((self.O, self.N, self.M)) if fetch else None
            self._call(row, "denoise", p, a, am, an, [_opt(u)], w=wa, wo=wo, channels=channels)
            return u
        finally:
            self._full_tape(spacing_set)

    def _solve_device(self, row, alpha_ptr, am, an, kw, w_ptr=None, wo=None, channels=None, tape_ptr=None):
        """<row>_denoise_device; a taped row ends on the tape pointer (0 / None: the handle's own tape)."""
        p, spacing_set = self._taped_params(row, kw)
        try:
            self._call(row, "denoise", p, alpha_ptr, am, an, [_dev(tape_ptr)] if row.taped else [], w=w_ptr, wo=wo,
                       channels=channels, device=True)
        finally:
            self._full_tape(spacing_set)

    def _tape_doubles(self, row, kw):
        p, spacing_set = self._taped_params(row, kw)
        try:
            n = C.c_ulonglong(0)
            self._check(getattr(self._lib, row.entry("tape_doubles"))(self._h, C.byref(p), C.byref(n)))
            return int(n.value)
        finally:
            self._full_tape(spacing_set)

    def _evaluate(self, row, x, delta, fetch_u, kw):
        a, am, an, scalar = self._param(row, x)
        self._last_npar = row.slices * am * an
        p = self.params(_sumregs=row.sumregs, **kw)
        u = np.empty((self.O, self.N, self.M)) if fetch_u else None
        cost = C.c_double(0.0)
        grad = np.empty(row.slices * am * an)
        self._check(getattr(self._lib, row.entry("evaluate"))(self._h, _ptr(a), am, an, float(delta), C.byref(p), _opt(u),
                                                              C.byref(cost), _ptr(grad)))
        return u, cost.value, self._like(grad, a, scalar)

    def _vjp(self, row, what, x, gu, want, kw, w=None, channels=None, u=None, f=None, reg=None, arrays_first=False):
        """<row>_vjp: (grad_f, grad_x[, grad_w]), want = (want_f, want_alpha[, want_w]).  A taped row sweeps the handle's tape;
        any other is implicit -- it leads with the solution u, then f where there is a w (read for grad_w only), and takes reg
        where there is none.  arrays_first: u and gu are checked before the keywords (sumregs_vjp_each always did)."""
        if not any(want):
            raise ValueError("%s: %s False" % (what, "want_f, want_alpha and want_w are all" if row.w else
                                               "want_f and want_alpha are both"))
        a, am, an, scalar = self._param(row, x)
        wa, wo = self._weight(w) if row.w else (None, None)
        if arrays_first:
            u, gu = self._batch(u, "u"), self._batch(gu, "gu")
        p, spacing_set = self._taped_params(row, kw)
        try:
            lead = []
            if not row.taped:
                u = self._batch(u, "u")
                lead.append(_ptr(u))
            gu = self._batch(gu, "gu")
            if row.w and not row.taped:
                if want[2] and f is None:
                    raise ValueError("%s: grad_w needs f" % what)
                f = self._batch(f, "f") if f is not None else None
                lead.append(_opt(f))
            gf = np.empty((self.O, self.N, self.M)) if want[0] else None
            ga = np.empty(a.shape if row.each else row.slices * am * an) if want[1] else None
            gw = np.empty(wa.shape) if row.w and want[2] else None
            self._call(row, "vjp", p, a, am, an, [_ptr(gu), _opt(gf), _opt(ga)] + ([_opt(gw)] if row.w else []), lead=lead,
                       w=wa, wo=wo, channels=channels, reg=None if row.taped or row.w else bool(reg))
            return (gf, self._like(ga, a, scalar)) + ((gw,) if row.w else ())
        finally:
            self._full_tape(spacing_set)

    def _vjp_device(self, row, first_ptr, alpha_ptr, am, an, gu_ptr, grad_ptrs, kw, w_ptr=None, wo=None, channels=None, f_ptr=None,
                    reg=None):
        """<row>_vjp_device.  first_ptr: the tape of a taped row (0 / None: the handle's own), u of an implicit one; grad_ptrs:
        the outputs in the order of _vjp's result, any of them 0 / None."""
        p, spacing_set = self._taped_params(row, kw)
        try:
            lead = [_dev(first_ptr)] if row.taped else [C.c_void_p(first_ptr)] + ([_dev(f_ptr)] if row.w else [])
            self._call(row, "vjp", p, alpha_ptr, am, an, [C.c_void_p(gu_ptr)] + [_dev(g) for g in grad_ptrs], lead=lead, w=w_ptr,
                       wo=wo, channels=channels, reg=None if row.taped or row.w else bool(reg), device=True)
        finally:
            self._full_tape(spacing_set)

    def _jvp(self, row, what, x, df, dalpha, kw, w=None, dw=None, channels=None, u=None, reg=None, want_u=False):
        """<row>_jvp: du for the tangents as stacks of K directions, one call.  An unrolled (taped) row sweeps the iterations --
        no tape, the spacing is never touched -- and ends on u (None unless want_u); any other is implicit: it leads with the
        solution u and takes reg.  A row with a w takes the tangent dw after dalpha."""
        a, am, an, scalar = self._param(row, x)
        wa, wo = self._weight(w) if row.w else (None, None)
        if row.w and df is None and dalpha is None and dw is None:
            raise ValueError("%s: df, dalpha and dw are all None" % what)
        K, batched = None, False
        if not row.w or df is not None or dalpha is not None:
            df, dalpha, K, batched = self._tangents(what, df, dalpha, () if scalar else a.shape)
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
        p = self.params(_sumregs=row.sumregs, **kw)
        lead = []
        if not row.taped:
            u = self._batch(u, "u")
            lead.append(_ptr(u))
        du = np.empty((K, self.O, self.N, self.M))
        uo = np.empty((self.O, self.N, self.M)) if want_u else None
        self._call(row, "jvp", p, a, am, an, [K, _opt(df), _opt(dalpha)] + ([_opt(dw)] if row.w else []) + [_ptr(du)]
                   + ([_opt(uo)] if row.taped else []), lead=lead, w=wa, wo=wo, channels=channels,
                   reg=None if row.taped else bool(reg))
        du = du if batched else du[0]
        return (du, uo) if want_u else du

    def _jvp_device(self, row, alpha_ptr, am, an, tangent_ptrs, du_ptr, ndir, kw, w_ptr=None, wo=None, channels=None, u_ptr=None,
                    reg=None):
        """<row>_jvp_device.  tangent_ptrs: (df, dalpha[, dw]), any of them 0 / None; u_ptr: the solution an implicit row leads
        with, the output an unrolled one ends on (0 / None: not wanted)."""
        p = self.params(_sumregs=row.sumregs, **kw)
        self._call(row, "jvp", p, alpha_ptr, am, an, [int(ndir)] + [_dev(t) for t in tangent_ptrs] + [C.c_void_p(du_ptr)]
                   + ([_dev(u_ptr)] if row.taped else []), lead=[] if row.taped else [C.c_void_p(u_ptr)], w=w_ptr, wo=wo,
                   channels=channels, reg=None if row.taped else bool(reg), device=True)

    def _gauss_newton(self, row, x, kw, w=None, channels=None, u=None, ubar=None, reg=None):
        """<row>_gauss_newton: (grad, H) of an implicit row, for the given u and ubar; (cost, grad, H) of an unrolled (taped)
        one, on the resident dataset.  grad has the type / shape of x, H is (P, P) with P = x.size."""
        a, am, an, scalar = self._param(row, x)
        wa, wo = self._weight(w) if row.w else (None, None)
        p = self.params(_sumregs=row.sumregs, **kw)
        P = row.slices * am * an
        cost, grad, H = C.c_double(0.0), np.empty(P), np.empty((P, P))
        if row.taped:
            self._call(row, "gauss_newton", p, a, am, an, [C.byref(cost), _ptr(grad), _ptr(H)], w=wa, wo=wo, channels=channels)
            return float(cost.value), self._like(grad, a, scalar), H
        u = self._batch(u, "u")
        ubar = self._batch(ubar, "ubar")
        self._call(row, "gauss_newton", p, a, am, an, [_ptr(grad), _ptr(H)], lead=[_ptr(u), _ptr(ubar)], reg=bool(reg))
        return self._like(grad, a, scalar), H

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
        return self._solve(_TV, x, fetch, kw)

    def denoise_device(self, alpha_ptr, am=1, an=1, **kw):
        """bpltv_denoise_device: the parameter (am x an doubles, column major) already resident in HBM at `alpha_ptr`
        (e.g. a torch tensor's .data_ptr()); the result stays on the device (u_device_ptr / copy_u_device)."""
        self._solve_device(_TV, alpha_ptr, am, an, kw)

    def evaluate(self, x, delta, fetch_u=True, **kw):
        return self._evaluate(_TV, x, delta, fetch_u, kw)

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
        return self._solve(_SUMREGS, x, fetch, kw)

    def sumregs_evaluate(self, x, delta, fetch_u=True, **kw):
        """sumregs_learning_function(x, data, D; Dt = 1e-3) -> (u, cost, grad) (:8-36); grad has the shape of x."""
        return self._evaluate(_SUMREGS, x, delta, fetch_u, kw)

    def sumregs_denoise_device(self, alpha_ptr, am=1, an=1, **kw):
        """bpltv_sumregs_denoise_device: the parameter (3*am*an doubles, three column-major am x an slices -- a
        C-contiguous (3, an, am) array) already resident in HBM at `alpha_ptr`; the result stays on the device
        (u_device_ptr / copy_u_device)."""
        self._solve_device(_SUMREGS, alpha_ptr, am, an, kw)

    def sumregs_vjp(self, u, x, gu, reg=False, want_f=True, want_alpha=True, **kw):
        """Vector-Jacobian product of u = sumregs_denoise(f, x) for the cotangent gu = dL/du (bpltv_sumregs_vjp):
        (grad_f, grad_x).  u, gu: (O, N, M) batches; x: (3,) or (3, n, m).  grad_f has the shape of u (None unless
        want_f), grad_x the shape of x (None unless want_alpha).  gu = u - ubar gives sumregs_evaluate's gradient
        bitwise (reg = the evaluate's delta <= delta_t)."""
        return self._vjp(_SUMREGS, "sumregs_vjp", x, gu, (want_f, want_alpha), kw, u=u, reg=reg)

    def sumregs_vjp_device(self, u_ptr, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, reg=False, **kw):
        """bpltv_sumregs_vjp_device: u, gu and grad_f (M*N*O doubles), the parameter and grad_alpha (3*am*an doubles)
        all resident in HBM; either output pointer may be 0 / None, not both."""
        self._vjp_device(_SUMREGS, u_ptr, alpha_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alpha_ptr), kw, reg=reg)

    # -- forward mode of the sum-of-regularisers model (bpltv_sumregs_jvp / bpltv_sumregs_gauss_newton) ------------
    def sumregs_jvp(self, u, x, df=None, dalpha=None, reg=False, **kw):
        """Jacobian-vector product of u = sumregs_denoise(f, x) (bpltv_sumregs_jvp): du for the tangents (df, dalpha),
        the linear map whose transpose sumregs_vjp computes.  x: (3,) or (3, n, m); df: (O, N, M), or (K, O, N, M) for K
        directions solved against one factorisation; dalpha: shaped like x, or with a leading K; either may be None
        (zero), not both.  Returns du of shape (O, N, M), or (K, O, N, M) when a leading K was given."""
        return self._jvp(_SUMREGS, "sumregs_jvp", x, df, dalpha, kw, u=u, reg=reg)

    def sumregs_jvp_device(self, u_ptr, alpha_ptr, am, an, df_ptr, dalpha_ptr, du_ptr, ndir=1, reg=False, **kw):
        """bpltv_sumregs_jvp_device: u (M*N*O doubles), the parameter (3*am*an), df and du (ndir*M*N*O) and dalpha
        (ndir*3*am*an) all resident in HBM (raw device pointers); either tangent pointer may be 0 / None, not both."""
        self._jvp_device(_SUMREGS, alpha_ptr, am, an, (df_ptr, dalpha_ptr), du_ptr, ndir, kw, u_ptr=u_ptr, reg=reg)

    def sumregs_gauss_newton(self, u, ubar, x, reg=False, **kw):
        """Gauss-Newton model of 0.5||u(x) - ubar||^2 (bpltv_sumregs_gauss_newton): (grad, H) with grad = J^T (u - ubar)
        shaped like x and H = J^T J of shape (P, P), P = x.size <= 16, ordered as numpy's x.ravel() (the library's
        parameter layout).  x: (3,), or a (3, n, m) patch."""
        return self._gauss_newton(_SUMREGS, x, kw, u=u, ubar=ubar, reg=reg)

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
        return self._vjp(_TV, "vjp", x, gu, (want_f, want_alpha), kw, u=u, reg=reg)

    def vjp_device(self, u_ptr, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, reg=False, **kw):
        """bpltv_vjp_device: u, gu and grad_f (M*N*O doubles), the parameter and grad_alpha (am*an doubles, column
        major) all resident in HBM (raw device pointers, e.g. torch tensors' .data_ptr()); either output pointer may
        be 0 / None, not both."""
        self._vjp_device(_TV, u_ptr, alpha_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alpha_ptr), kw, reg=reg)

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
        return self._solve(_WEIGHTED, x, fetch, kw, w=w)

    def weighted_denoise_device(self, w_ptr, wo, alpha_ptr, am=1, an=1, **kw):
        """bpltv_weighted_denoise_device: w (wo planes of M*N doubles, wo = 1 or O) and the parameter (am x an doubles)
        already resident in HBM; the result stays on the device (u_device_ptr / copy_u_device)."""
        self._solve_device(_WEIGHTED, alpha_ptr, am, an, kw, w_ptr=w_ptr, wo=wo)

    def weighted_vjp(self, u, f, x, w, gu, want_f=True, want_alpha=True, want_w=True, **kw):
        """Vector-Jacobian product of u = weighted_denoise(f, x, w) for the cotangent gu (bpltv_weighted_vjp):
        (grad_f, grad_x, grad_w).  u, gu: (O, N, M); f: (O, N, M), or None when grad_w is not wanted; w > 0: (N, M) or
        (O, N, M).  grad_w has the shape of w -- for (N, M) the sum over the images; an output not wanted is None."""
        return self._vjp(_WEIGHTED, "weighted_vjp", x, gu, (want_f, want_alpha, want_w), kw, w=w, u=u, f=f)

    def weighted_vjp_device(self, u_ptr, f_ptr, w_ptr, wo, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr,
                            grad_w_ptr, **kw):
        """bpltv_weighted_vjp_device: every array resident in HBM (raw device pointers); any output pointer may be
        0 / None, not all three; f_ptr may be 0 / None only if grad_w_ptr is."""
        self._vjp_device(_WEIGHTED, u_ptr, alpha_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alpha_ptr, grad_w_ptr), kw,
                         w_ptr=w_ptr, wo=wo, f_ptr=f_ptr)

    # -- reverse mode through the iterations (bpltv_unrolled_*) --------------------------------------------------
    # Every *_unrolled_tape_doubles, *_unrolled_denoise* and *_unrolled_vjp* method takes checkpoint_every=C on top of the
    # params keywords (option "tape_checkpoint"): None / 0 the full tape, C >= 1 the iteration state
    # every C iterations instead of a tape -- the sweep then recomputes each segment's tape, same bits, one more forward
    # solve -- and -1 the spacing of least memory (auto_checkpoint_every).  Solve, sweep and tape_doubles of one tape take the
    # same value.  The taped cores set the option (_taped_params) and take it back in their own finally (_full_tape).
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
        return self._tape_doubles(_UNROLLED, kw)

    def unrolled_denoise(self, x, fetch=True, **kw):
        """denoise(x) with rho = 0 -- the same u bit for bit -- that also records the tape of the iterations in the
        handle, for unrolled_vjp with the same x and params (bpltv_unrolled_denoise)."""
        return self._solve(_UNROLLED, x, fetch, kw)

    def unrolled_denoise_device(self, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_unrolled_denoise_device: the parameter resident in HBM, the result left there (u_device_ptr /
        copy_u_device); tape_ptr: a caller-owned HBM buffer of unrolled_tape_doubles(**kw) doubles, or None / 0 for
        the handle's own tape."""
        self._solve_device(_UNROLLED, alpha_ptr, am, an, kw, tape_ptr=tape_ptr)

    def unrolled_vjp(self, x, gu, want_f=True, want_alpha=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = unrolled_denoise(x) for the cotangent gu = dL/du, by a
        reverse sweep over the handle's tape (bpltv_unrolled_vjp): (grad_f, grad_x).  x and the params must be those
        of the solve.  gu: (O, N, M); grad_f has its shape (None unless want_f), grad_x the type / shape of x (None
        unless want_alpha)."""
        return self._vjp(_UNROLLED, "unrolled_vjp", x, gu, (want_f, want_alpha), kw)

    def unrolled_vjp_device(self, tape_ptr, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, **kw):
        """bpltv_unrolled_vjp_device: the tape (None / 0: the handle's own), the parameter, gu and the outputs resident
        in HBM (raw device pointers); either output pointer may be 0 / None, not both."""
        self._vjp_device(_UNROLLED, tape_ptr, alpha_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alpha_ptr), kw)

    # -- channel-coupled TV for colour images (bpltv_color_*) ------------------------------------------------------
    # The handle's O planes are O / channels colour images of `channels` consecutive planes; x is one parameter shared by the
    # batch and the channels.  The tape has the TV tape's size: unrolled_tape_doubles.
    def color_denoise(self, x, channels, fetch=True, **kw):
        """Vectorial TV: the channels of a colour image share one projection per pixel (bpltv_color_denoise).  No tape, any
        maxiter >= 1; u is bitwise color_unrolled_denoise's."""
        return self._solve(_COLOR, x, fetch, kw, channels=channels)

    def color_denoise_device(self, channels, alpha_ptr, am=1, an=1, **kw):
        """bpltv_color_denoise_device: the parameter resident in HBM, the result left there (u_device_ptr / copy_u_device)."""
        self._solve_device(_COLOR, alpha_ptr, am, an, kw, channels=channels)

    def color_unrolled_denoise(self, x, channels, fetch=True, **kw):
        """color_denoise that also records the tape of the iterations in the handle, for color_unrolled_vjp with the same
        x, channels and params (bpltv_color_unrolled_denoise)."""
        return self._solve(_COLOR_UNROLLED, x, fetch, kw, channels=channels)

    def color_unrolled_denoise_device(self, channels, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_color_unrolled_denoise_device: the parameter resident in HBM, the result left there; tape_ptr: a
        caller-owned HBM buffer of unrolled_tape_doubles(**kw) doubles, or None / 0 for the handle's colour tape."""
        self._solve_device(_COLOR_UNROLLED, alpha_ptr, am, an, kw, channels=channels, tape_ptr=tape_ptr)

    def color_unrolled_vjp(self, x, channels, gu, want_f=True, want_alpha=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = color_unrolled_denoise(x, channels) for the cotangent gu, by
        a reverse sweep over the handle's colour tape (bpltv_color_unrolled_vjp): (grad_f, grad_x), as unrolled_vjp."""
        return self._vjp(_COLOR_UNROLLED, "color_unrolled_vjp", x, gu, (want_f, want_alpha), kw, channels=channels)

    def color_unrolled_vjp_device(self, channels, tape_ptr, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, **kw):
        """bpltv_color_unrolled_vjp_device: the tape (None / 0: the handle's own), the parameter, gu and the outputs
        resident in HBM (raw device pointers); either output pointer may be 0 / None, not both."""
        self._vjp_device(_COLOR_UNROLLED, tape_ptr, alpha_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alpha_ptr), kw,
                         channels=channels)

    def color_unrolled_jvp(self, x, channels, df=None, dalpha=None, want_u=False, **kw):
        """Jacobian-vector product of the maxiter-step map u = color_denoise(x, channels) of the resident f
        (bpltv_color_unrolled_jvp): a tangent sweep through the channel-coupled iterations, no tape -- the linear map whose
        transpose color_unrolled_vjp computes.  Tangents, result and want_u as unrolled_jvp; channels = 1 is unrolled_jvp
        bit for bit."""
        return self._jvp(_COLOR_UNROLLED, "color_unrolled_jvp", x, df, dalpha, kw, channels=channels, want_u=want_u)

    def color_unrolled_jvp_device(self, channels, alpha_ptr, am, an, df_ptr, dalpha_ptr, du_ptr, u_ptr=None, ndir=1, **kw):
        """bpltv_color_unrolled_jvp_device: as unrolled_jvp_device, for colour images of `channels` planes."""
        self._jvp_device(_COLOR_UNROLLED, alpha_ptr, am, an, (df_ptr, dalpha_ptr), du_ptr, ndir, kw, channels=channels,
                         u_ptr=u_ptr)

    def color_unrolled_gauss_newton(self, x, channels, **kw):
        """Gauss-Newton model of the maxiter-step loss 0.5||u_K(x) - ubar||^2 of the channel-coupled solve, over all planes
        (bpltv_color_unrolled_gauss_newton): (cost, grad, H) as unrolled_gauss_newton."""
        return self._gauss_newton(_COLOR_UNROLLED, x, kw, channels=channels)

    # -- channel-coupled TV with a per-pixel fidelity weight (bpltv_color_weighted_*) ------------------------------
    # w >= 0, zeros allowed: (N, M) -- one plane for every plane of the batch -- or (O, N, M), one per plane (per channel).  The
    # tape has the weighted tape's size: weighted_unrolled_tape_doubles.
    def color_weighted_denoise(self, x, channels, w, fetch=True, **kw):
        """Vectorial TV with the fidelity 0.5 sum_c w_c (u_c - f_c)^2 (bpltv_color_weighted_denoise): colour inpainting,
        demosaicing, a variance per channel.  No tape; u is bitwise color_weighted_unrolled_denoise's, and with w = 1
        color_denoise's."""
        return self._solve(_COLOR_WEIGHTED, x, fetch, kw, w=w, channels=channels)

    def color_weighted_denoise_device(self, channels, w_ptr, wo, alpha_ptr, am=1, an=1, **kw):
        """bpltv_color_weighted_denoise_device: w (wo planes) and the parameter resident in HBM, the result left there."""
        self._solve_device(_COLOR_WEIGHTED, alpha_ptr, am, an, kw, w_ptr=w_ptr, wo=wo, channels=channels)

    def color_weighted_unrolled_denoise(self, x, channels, w, fetch=True, **kw):
        """color_weighted_denoise that also records the tape of the iterations in the handle, for
        color_weighted_unrolled_vjp with the same x, channels, w and params (bpltv_color_weighted_unrolled_denoise)."""
        return self._solve(_COLOR_WEIGHTED_UNROLLED, x, fetch, kw, w=w, channels=channels)

    def color_weighted_unrolled_denoise_device(self, channels, w_ptr, wo, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_color_weighted_unrolled_denoise_device: w (wo planes) and the parameter resident in HBM, the result left
        there; tape_ptr: a caller-owned HBM buffer of weighted_unrolled_tape_doubles(**kw) doubles, or None / 0 for the
        handle's colour-weighted tape."""
        self._solve_device(_COLOR_WEIGHTED_UNROLLED, alpha_ptr, am, an, kw, w_ptr=w_ptr, wo=wo, channels=channels,
                           tape_ptr=tape_ptr)

    def color_weighted_unrolled_vjp(self, x, channels, w, gu, want_f=True, want_alpha=True, want_w=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = color_weighted_unrolled_denoise(x, channels, w) for the
        cotangent gu, by a reverse sweep over the handle's colour-weighted tape (bpltv_color_weighted_unrolled_vjp):
        (grad_f, grad_x, grad_w), as weighted_unrolled_vjp.  grad_w has the shape of w -- for (N, M) the sum over the planes."""
        return self._vjp(_COLOR_WEIGHTED_UNROLLED, "color_weighted_unrolled_vjp", x, gu, (want_f, want_alpha, want_w), kw, w=w,
                         channels=channels)

    def color_weighted_unrolled_vjp_device(self, channels, tape_ptr, w_ptr, wo, alpha_ptr, am, an, gu_ptr, grad_f_ptr,
                                           grad_alpha_ptr, grad_w_ptr, **kw):
        """bpltv_color_weighted_unrolled_vjp_device: the tape (None / 0: the handle's own), w, the parameter, gu and the
        outputs resident in HBM (raw device pointers); any output pointer may be 0 / None, not all three."""
        self._vjp_device(_COLOR_WEIGHTED_UNROLLED, tape_ptr, alpha_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alpha_ptr,
                         grad_w_ptr), kw, w_ptr=w_ptr, wo=wo, channels=channels)

    # -- reverse mode through the weighted iterations (bpltv_weighted_unrolled_*) --------------------------------
    def weighted_unrolled_tape_doubles(self, **kw):
        """Doubles of the tape a weighted unrolled solve with these params records: 3 * maxiter * M*N*O."""
        return self._tape_doubles(_WEIGHTED_UNROLLED, kw)

    def weighted_unrolled_denoise(self, x, w, fetch=True, **kw):
        """weighted_denoise(x, w) -- the same u bit for bit, w >= 0 with zeros allowed -- that also records the tape of
        the iterations in the handle, for weighted_unrolled_vjp with the same x, w and params
        (bpltv_weighted_unrolled_denoise)."""
        return self._solve(_WEIGHTED_UNROLLED, x, fetch, kw, w=w)

    def weighted_unrolled_denoise_device(self, w_ptr, wo, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_weighted_unrolled_denoise_device: w (wo planes) and the parameter resident in HBM, the result left
        there; tape_ptr: a caller-owned HBM buffer of weighted_unrolled_tape_doubles(**kw) doubles, or None / 0 for the
        handle's own weighted tape."""
        self._solve_device(_WEIGHTED_UNROLLED, alpha_ptr, am, an, kw, w_ptr=w_ptr, wo=wo, tape_ptr=tape_ptr)

    def weighted_unrolled_vjp(self, x, w, gu, want_f=True, want_alpha=True, want_w=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = weighted_unrolled_denoise(x, w) for the cotangent gu, by
        a reverse sweep over the handle's weighted tape (bpltv_weighted_unrolled_vjp): (grad_f, grad_x, grad_w).  x, w
        and the params must be those of the solve; w >= 0, zeros allowed.  grad_w has the shape of w -- for (N, M) the
        sum over the images; an output not wanted is None."""
        return self._vjp(_WEIGHTED_UNROLLED, "weighted_unrolled_vjp", x, gu, (want_f, want_alpha, want_w), kw, w=w)

    def weighted_unrolled_vjp_device(self, tape_ptr, w_ptr, wo, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr,
                                     grad_w_ptr, **kw):
        """bpltv_weighted_unrolled_vjp_device: the tape (None / 0: the handle's own), w, the parameter, gu and the
        outputs resident in HBM (raw device pointers); any output pointer may be 0 / None, not all three."""
        self._vjp_device(_WEIGHTED_UNROLLED, tape_ptr, alpha_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alpha_ptr, grad_w_ptr), kw,
                         w_ptr=w_ptr, wo=wo)

    # -- TV-L1: the data term w |u - f|, for impulse noise (bpltv_lone_*) ------------------------------------------
    # w >= 0, zeros allowed: (N, M) or (O, N, M).  The tape has the weighted tape's size: weighted_unrolled_tape_doubles.
    def l1_denoise(self, x, w, fetch=True, **kw):
        """TV-L1 denoising of the resident f (bpltv_lone_denoise): min sum w |u - f| + sum alpha |grad u|, maxiter iterations
        of the weighted recurrence with a soft threshold around f as the primal step.  Removes isolated outliers exactly
        and keeps the contrast of the rest.  No tape; u is bitwise l1_unrolled_denoise's."""
        return self._solve(_L1, x, fetch, kw, w=w)

    def l1_denoise_device(self, w_ptr, wo, alpha_ptr, am=1, an=1, **kw):
        """bpltv_lone_denoise_device: w (wo planes) and the parameter resident in HBM, the result left there."""
        self._solve_device(_L1, alpha_ptr, am, an, kw, w_ptr=w_ptr, wo=wo)

    def l1_unrolled_denoise(self, x, w, fetch=True, **kw):
        """l1_denoise(x, w) -- the same u bit for bit -- that also records the tape of the iterations in the handle, for
        l1_unrolled_vjp with the same x, w and params (bpltv_lone_unrolled_denoise)."""
        return self._solve(_L1_UNROLLED, x, fetch, kw, w=w)

    def l1_unrolled_denoise_device(self, w_ptr, wo, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_lone_unrolled_denoise_device: w (wo planes) and the parameter resident in HBM, the result left there;
        tape_ptr: a caller-owned HBM buffer of weighted_unrolled_tape_doubles(**kw) doubles, or None / 0 for the handle's
        own L1 tape."""
        self._solve_device(_L1_UNROLLED, alpha_ptr, am, an, kw, w_ptr=w_ptr, wo=wo, tape_ptr=tape_ptr)

    def l1_unrolled_vjp(self, x, w, gu, want_f=True, want_alpha=True, want_w=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = l1_unrolled_denoise(x, w) for the cotangent gu, by a reverse
        sweep over the handle's L1 tape (bpltv_lone_unrolled_vjp): (grad_f, grad_x, grad_w), as weighted_unrolled_vjp."""
        return self._vjp(_L1_UNROLLED, "l1_unrolled_vjp", x, gu, (want_f, want_alpha, want_w), kw, w=w)

    def l1_unrolled_vjp_device(self, tape_ptr, w_ptr, wo, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, grad_w_ptr, **kw):
        """bpltv_lone_unrolled_vjp_device: the tape (None / 0: the handle's own), w, the parameter, gu and the outputs resident
        in HBM (raw device pointers); any output pointer may be 0 / None, not all three."""
        self._vjp_device(_L1_UNROLLED, tape_ptr, alpha_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alpha_ptr, grad_w_ptr), kw,
                         w_ptr=w_ptr, wo=wo)

    # -- TV-KL: the data term w (u - f log u), for Poisson noise (bpltv_kl_*) ------------------------------------------
    # f finite and >= 0 (zero counts allowed); w >= 0, zeros allowed: (N, M) or (O, N, M).  The tape has the weighted tape's size.
    def kl_denoise(self, x, w, fetch=True, **kw):
        """TV-KL denoising of the resident f (bpltv_kl_denoise): min sum w (u - f log u) + sum alpha |grad u| over u >= 0,
        maxiter iterations of the weighted recurrence with the closed-form prox of the Kullback-Leibler divergence as the primal
        step.  The model for photon counts.  No tape; u is bitwise kl_unrolled_denoise's."""
        return self._solve(_KL, x, fetch, kw, w=w)

    def kl_denoise_device(self, w_ptr, wo, alpha_ptr, am=1, an=1, **kw):
        """bpltv_kl_denoise_device: w (wo planes) and the parameter resident in HBM, the result left there."""
        self._solve_device(_KL, alpha_ptr, am, an, kw, w_ptr=w_ptr, wo=wo)

    def kl_unrolled_denoise(self, x, w, fetch=True, **kw):
        """kl_denoise(x, w) -- the same u bit for bit -- that also records the tape of the iterations in the handle, for
        kl_unrolled_vjp with the same x, w and params (bpltv_kl_unrolled_denoise)."""
        return self._solve(_KL_UNROLLED, x, fetch, kw, w=w)

    def kl_unrolled_denoise_device(self, w_ptr, wo, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_kl_unrolled_denoise_device: w (wo planes) and the parameter resident in HBM, the result left there;
        tape_ptr: a caller-owned HBM buffer of weighted_unrolled_tape_doubles(**kw) doubles, or None / 0 for the handle's
        own KL tape."""
        self._solve_device(_KL_UNROLLED, alpha_ptr, am, an, kw, w_ptr=w_ptr, wo=wo, tape_ptr=tape_ptr)

    def kl_unrolled_vjp(self, x, w, gu, want_f=True, want_alpha=True, want_w=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = kl_unrolled_denoise(x, w) for the cotangent gu, by a reverse
        sweep over the handle's KL tape (bpltv_kl_unrolled_vjp): (grad_f, grad_x, grad_w), as weighted_unrolled_vjp."""
        return self._vjp(_KL_UNROLLED, "kl_unrolled_vjp", x, gu, (want_f, want_alpha, want_w), kw, w=w)

    def kl_unrolled_vjp_device(self, tape_ptr, w_ptr, wo, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, grad_w_ptr, **kw):
        """bpltv_kl_unrolled_vjp_device: the tape (None / 0: the handle's own), w, the parameter, gu and the outputs resident
        in HBM (raw device pointers); any output pointer may be 0 / None, not all three."""
        self._vjp_device(_KL_UNROLLED, tape_ptr, alpha_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alpha_ptr, grad_w_ptr), kw,
                         w_ptr=w_ptr, wo=wo)

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
        return self._jvp(_TV, "jvp", x, df, dalpha, kw, u=u, reg=reg)

    def jvp_device(self, u_ptr, alpha_ptr, am, an, df_ptr, dalpha_ptr, du_ptr, ndir=1, reg=False, **kw):
        """bpltv_jvp_device: u (M*N*O doubles), the parameter (am*an), df and du (ndir*M*N*O) and dalpha (ndir*am*an)
        all resident in HBM (raw device pointers); either tangent pointer may be 0 / None, not both."""
        self._jvp_device(_TV, alpha_ptr, am, an, (df_ptr, dalpha_ptr), du_ptr, ndir, kw, u_ptr=u_ptr, reg=reg)

    def jvp_each(self, u, alphas, df=None, dalphas=None, reg=False, **kw):
        """jvp with image k's own parameter alphas[k] (bpltv_jvp_each).  dalphas: shaped like alphas, or with a leading
        K; df and the result as in jvp."""
        return self._jvp(_TV_EACH, "jvp_each", alphas, df, dalphas, kw, u=u, reg=reg)

    def jvp_each_device(self, u_ptr, alphas_ptr, am, an, df_ptr, dalphas_ptr, du_ptr, ndir=1, reg=False, **kw):
        """bpltv_jvp_each_device: as jvp_device with O parameter blocks (O*am*an doubles) and ndir*O tangent blocks."""
        self._jvp_device(_TV_EACH, alphas_ptr, am, an, (df_ptr, dalphas_ptr), du_ptr, ndir, kw, u_ptr=u_ptr, reg=reg)

    def gauss_newton(self, u, ubar, x, reg=False, **kw):
        """Gauss-Newton model of 0.5||u(x) - ubar||^2 (bpltv_gauss_newton): (grad, H) with grad = J^T (u - ubar) shaped
        like x and H = J^T J of shape (P, P), P = x.size, ordered as x's column-major (Julia) entries -- numpy's
        x.ravel().  A float or an (n, m) patch parameter with at most 16 entries."""
        return self._gauss_newton(_TV, x, kw, u=u, ubar=ubar, reg=reg)

    # -- forward mode through the iterations (bpltv_unrolled_jvp / bpltv_unrolled_gauss_newton) ---------------
    def unrolled_jvp(self, x, df=None, dalpha=None, want_u=False, **kw):
        """Jacobian-vector product of the maxiter-step map u = unrolled_denoise(x) of the resident f (bpltv_unrolled_jvp):
        a tangent sweep through the iterations, no tape -- the linear map whose transpose unrolled_vjp computes.  df:
        (O, N, M), or (K, O, N, M) for K directions; dalpha: shaped like x, or with a leading K; either may be None
        (zero), not both.  Returns du of shape (O, N, M), or (K, O, N, M) when a leading K was given; with want_u,
        (du, u) with u = denoise(x) bit for bit."""
        return self._jvp(_UNROLLED, "unrolled_jvp", x, df, dalpha, kw, want_u=want_u)

    def unrolled_jvp_device(self, alpha_ptr, am, an, df_ptr, dalpha_ptr, du_ptr, u_ptr=None, ndir=1, **kw):
        """bpltv_unrolled_jvp_device: the parameter (am*an doubles), df and du (ndir*M*N*O), dalpha (ndir*am*an) and u
        (M*N*O) all resident in HBM (raw device pointers); either tangent pointer may be 0 / None, not both; u_ptr may
        be 0 / None."""
        self._jvp_device(_UNROLLED, alpha_ptr, am, an, (df_ptr, dalpha_ptr), du_ptr, ndir, kw, u_ptr=u_ptr)

    def unrolled_gauss_newton(self, x, **kw):
        """Gauss-Newton model of the maxiter-step loss 0.5||u_K(x) - ubar||^2 on the resident dataset
        (bpltv_unrolled_gauss_newton): (cost, grad, H) with grad = J^T (u_K - ubar) shaped like x and H = J^T J of shape
        (P, P), P = x.size, ordered as numpy's x.ravel(); J by P tangent sweeps.  A float or an (n, m) patch parameter
        with at most 16 entries."""
        return self._gauss_newton(_UNROLLED, x, kw)

    # -- forward mode through the weighted iterations (bpltv_weighted_unrolled_jvp / _gauss_newton) -----------
    def weighted_unrolled_jvp(self, x, w, df=None, dalpha=None, dw=None, want_u=False, **kw):
        """Jacobian-vector product of the maxiter-step map u = weighted_unrolled_denoise(x, w) of the resident f
        (bpltv_weighted_unrolled_jvp): a tangent sweep through the weighted iterations, no tape -- the linear map whose
        transpose weighted_unrolled_vjp computes; w >= 0, zeros allowed (a mask).  df: (O, N, M), or (K, O, N, M) for K
        directions; dalpha: shaped like x, or with a leading K; dw: shaped like w, or with a leading K; any may be None
        (zero), not all three.  Returns du of shape (O, N, M), or (K, O, N, M) when a leading K was given; with want_u,
        (du, u) with u = weighted_denoise(x, w) bit for bit.  The step table (gamma = min w) is held fixed."""
        return self._jvp(_WEIGHTED_UNROLLED, "weighted_unrolled_jvp", x, df, dalpha, kw, w=w, dw=dw, want_u=want_u)

    def weighted_unrolled_jvp_device(self, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr, dw_ptr, du_ptr, u_ptr=None,
                                     ndir=1, **kw):
        """bpltv_weighted_unrolled_jvp_device: w (wo planes), the parameter (am*an doubles), df and du (ndir*M*N*O), dalpha
        (ndir*am*an), dw (ndir*M*N*wo) and u (M*N*O) all resident in HBM (raw device pointers); any tangent pointer may be
        0 / None, not all three; u_ptr may be 0 / None."""
        self._jvp_device(_WEIGHTED_UNROLLED, alpha_ptr, am, an, (df_ptr, dalpha_ptr, dw_ptr), du_ptr, ndir, kw, w_ptr=w_ptr,
                         wo=wo, u_ptr=u_ptr)

    def weighted_unrolled_gauss_newton(self, x, w, **kw):
        """Gauss-Newton model of the maxiter-step loss 0.5||u_K(x) - ubar||^2 of the weighted iterations on the resident
        dataset (bpltv_weighted_unrolled_gauss_newton): (cost, grad, H) as unrolled_gauss_newton's, J by P tangent sweeps
        in the parameter.  A float or an (n, m) patch parameter with at most 16 entries; w >= 0, zeros allowed."""
        return self._gauss_newton(_WEIGHTED_UNROLLED, x, kw, w=w)

    # -- forward mode through the TV-L1 and the TV-KL iterations (bpltv_lone_unrolled_jvp, bpltv_kl_unrolled_jvp) -----
    def l1_unrolled_jvp(self, x, w, df=None, dalpha=None, dw=None, want_u=False, **kw):
        """Jacobian-vector product of the maxiter-step map u = l1_denoise(x, w) of the resident f (bpltv_lone_unrolled_jvp): a
        tangent sweep through the TV-L1 iterations, no tape -- the linear map whose transpose l1_unrolled_vjp computes, with
        its conventions (a pixel held at f moves with f alone).  Arguments and result as weighted_unrolled_jvp; with want_u,
        (du, u) with u = l1_denoise(x, w) bit for bit."""
        return self._jvp(_L1_UNROLLED, "l1_unrolled_jvp", x, df, dalpha, kw, w=w, dw=dw, want_u=want_u)

    def l1_unrolled_jvp_device(self, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr, dw_ptr, du_ptr, u_ptr=None, ndir=1, **kw):
        """bpltv_lone_unrolled_jvp_device: everything resident in HBM (raw device pointers), as weighted_unrolled_jvp_device."""
        self._jvp_device(_L1_UNROLLED, alpha_ptr, am, an, (df_ptr, dalpha_ptr, dw_ptr), du_ptr, ndir, kw, w_ptr=w_ptr, wo=wo,
                         u_ptr=u_ptr)

    def l1_unrolled_gauss_newton(self, x, w, **kw):
        """Gauss-Newton model of the maxiter-step loss 0.5||u_K(x) - ubar||^2 of the TV-L1 iterations on the resident dataset
        (bpltv_lone_unrolled_gauss_newton): (cost, grad, H) as weighted_unrolled_gauss_newton's."""
        return self._gauss_newton(_L1_UNROLLED, x, kw, w=w)

    def kl_unrolled_jvp(self, x, w, df=None, dalpha=None, dw=None, want_u=False, **kw):
        """Jacobian-vector product of the maxiter-step map u = kl_denoise(x, w) of the resident f >= 0 (bpltv_kl_unrolled_jvp): a
        tangent sweep through the TV-KL iterations, no tape -- the linear map whose transpose kl_unrolled_vjp computes, with
        its convention (a pixel clamped at zero passes nothing).  Arguments and result as weighted_unrolled_jvp; with want_u,
        (du, u) with u = kl_denoise(x, w) bit for bit."""
        return self._jvp(_KL_UNROLLED, "kl_unrolled_jvp", x, df, dalpha, kw, w=w, dw=dw, want_u=want_u)

    def kl_unrolled_jvp_device(self, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr, dw_ptr, du_ptr, u_ptr=None, ndir=1, **kw):
        """bpltv_kl_unrolled_jvp_device: everything resident in HBM (raw device pointers), as weighted_unrolled_jvp_device."""
        self._jvp_device(_KL_UNROLLED, alpha_ptr, am, an, (df_ptr, dalpha_ptr, dw_ptr), du_ptr, ndir, kw, w_ptr=w_ptr, wo=wo,
                         u_ptr=u_ptr)

    def kl_unrolled_gauss_newton(self, x, w, **kw):
        """Gauss-Newton model of the maxiter-step loss 0.5||u_K(x) - ubar||^2 of the TV-KL iterations on the resident dataset
        (bpltv_kl_unrolled_gauss_newton): (cost, grad, H) as weighted_unrolled_gauss_newton's."""
        return self._gauss_newton(_KL_UNROLLED, x, kw, w=w)

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
        return self._solve(_TV_EACH, alphas, fetch, kw)

    def denoise_each_device(self, alphas_ptr, am=1, an=1, **kw):
        """bpltv_denoise_each_device: O parameter blocks (O*am*an doubles, block k column major at k*am*an) resident in
        HBM at `alphas_ptr`; the result stays on the device (u_device_ptr / copy_u_device)."""
        self._solve_device(_TV_EACH, alphas_ptr, am, an, kw)

    def vjp_each(self, u, alphas, gu, reg=False, want_f=True, want_alpha=True, **kw):
        """vjp with image k's own parameter alphas[k] (bpltv_vjp_each): (grad_f, grad_alphas).  grad_alphas has the shape
        of alphas; grad_alphas[k] is image k's term alone, not summed over the images."""
        return self._vjp(_TV_EACH, "vjp_each", alphas, gu, (want_f, want_alpha), kw, u=u, reg=reg)

    def vjp_each_device(self, u_ptr, alphas_ptr, am, an, gu_ptr, grad_f_ptr, grad_alphas_ptr, reg=False, **kw):
        """bpltv_vjp_each_device: u, gu and grad_f (M*N*O doubles), the O parameter blocks and their O gradients
        (O*am*an doubles each) all resident in HBM; either output pointer may be 0 / None, not both."""
        self._vjp_device(_TV_EACH, u_ptr, alphas_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alphas_ptr), kw, reg=reg)

    # -- one parameter per image through the iterations (bpltv_unrolled_*_each) ----------------------------------
    def unrolled_denoise_each(self, alphas, fetch=True, **kw):
        """unrolled_denoise with image k's own parameter alphas[k] (bpltv_unrolled_denoise_each): denoise_each's u bit for
        bit, and the handle's tape, recorded per image, for unrolled_vjp_each with the same alphas and params."""
        return self._solve(_UNROLLED_EACH, alphas, fetch, kw)

    def unrolled_denoise_each_device(self, alphas_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_unrolled_denoise_each_device: O parameter blocks (O*am*an doubles, block k column major at k*am*an)
        resident in HBM, the result left there; tape_ptr as in unrolled_denoise_device."""
        self._solve_device(_UNROLLED_EACH, alphas_ptr, am, an, kw, tape_ptr=tape_ptr)

    def unrolled_vjp_each(self, alphas, gu, want_f=True, want_alpha=True, **kw):
        """unrolled_vjp with image k's own parameter alphas[k], over the handle's per-image tape
        (bpltv_unrolled_vjp_each): (grad_f, grad_alphas).  grad_alphas has the shape of alphas; grad_alphas[k] is image
        k's term alone, not summed over the images."""
        return self._vjp(_UNROLLED_EACH, "unrolled_vjp_each", alphas, gu, (want_f, want_alpha), kw)

    def unrolled_vjp_each_device(self, tape_ptr, alphas_ptr, am, an, gu_ptr, grad_f_ptr, grad_alphas_ptr, **kw):
        """bpltv_unrolled_vjp_each_device: as unrolled_vjp_device with O parameter blocks and their O gradients (O*am*an
        doubles each) resident in HBM; either output pointer may be 0 / None, not both."""
        self._vjp_device(_UNROLLED_EACH, tape_ptr, alphas_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alphas_ptr), kw)

    def unrolled_jvp_each(self, alphas, df=None, dalphas=None, want_u=False, **kw):
        """unrolled_jvp with image k's own parameter alphas[k] (bpltv_unrolled_jvp_each).  dalphas: shaped like alphas,
        or with a leading K; df, want_u and the result as in unrolled_jvp (u = denoise_each(alphas) bit for bit)."""
        return self._jvp(_UNROLLED_EACH, "unrolled_jvp_each", alphas, df, dalphas, kw, want_u=want_u)

    def unrolled_jvp_each_device(self, alphas_ptr, am, an, df_ptr, dalphas_ptr, du_ptr, u_ptr=None, ndir=1, **kw):
        """bpltv_unrolled_jvp_each_device: as unrolled_jvp_device with O parameter blocks (O*am*an doubles) and ndir*O
        tangent blocks, direction first."""
        self._jvp_device(_UNROLLED_EACH, alphas_ptr, am, an, (df_ptr, dalphas_ptr), du_ptr, ndir, kw, u_ptr=u_ptr)

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
        return self._solve(_SUMREGS_EACH, alphas, fetch, kw)

    def sumregs_denoise_each_device(self, alphas_ptr, am=1, an=1, **kw):
        """bpltv_sumregs_denoise_each_device: O parameter blocks (O*3*am*an doubles, a C-contiguous (O, 3, an, am)
        array) resident in HBM at `alphas_ptr`; the result stays on the device (u_device_ptr / copy_u_device)."""
        self._solve_device(_SUMREGS_EACH, alphas_ptr, am, an, kw)

    def sumregs_vjp_each(self, u, alphas, gu, reg=False, want_f=True, want_alpha=True, **kw):
        """sumregs_vjp with image k's own block alphas[k] (bpltv_sumregs_vjp_each): (grad_f, grad_alphas).  grad_alphas
        has the shape of alphas; grad_alphas[k] is image k's term alone, not summed over the images."""
        return self._vjp(_SUMREGS_EACH, "sumregs_vjp_each", alphas, gu, (want_f, want_alpha), kw, u=u, reg=reg,
                         arrays_first=True)

    def sumregs_vjp_each_device(self, u_ptr, alphas_ptr, am, an, gu_ptr, grad_f_ptr, grad_alphas_ptr, reg=False, **kw):
        """bpltv_sumregs_vjp_each_device: u, gu and grad_f (M*N*O doubles), the O parameter blocks and their O gradients
        (O*3*am*an doubles each) all resident in HBM; either output pointer may be 0 / None, not both."""
        self._vjp_device(_SUMREGS_EACH, u_ptr, alphas_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alphas_ptr), kw, reg=reg)

    def sumregs_jvp_each(self, u, alphas, df=None, dalphas=None, reg=False, **kw):
        """sumregs_jvp with image k's own block alphas[k] (bpltv_sumregs_jvp_each).  dalphas: shaped like alphas, or
        with a leading K; df and the result as in sumregs_jvp."""
        return self._jvp(_SUMREGS_EACH, "sumregs_jvp_each", alphas, df, dalphas, kw, u=u, reg=reg)

    def sumregs_jvp_each_device(self, u_ptr, alphas_ptr, am, an, df_ptr, dalphas_ptr, du_ptr, ndir=1, reg=False, **kw):
        """bpltv_sumregs_jvp_each_device: as sumregs_jvp_device with O parameter blocks (O*3*am*an doubles) and ndir*O
        tangent blocks."""
        self._jvp_device(_SUMREGS_EACH, alphas_ptr, am, an, (df_ptr, dalphas_ptr), du_ptr, ndir, kw, u_ptr=u_ptr, reg=reg)

    # -- reverse mode through the sum-of-regularisers iterations (bpltv_sumregs_unrolled_*) ------------------------
    def sumregs_unrolled_tape_doubles(self, **kw):
        """Doubles of the tape a sum-of-regularisers unrolled solve with these params records: 6 * maxiter * M*N*O."""
        return self._tape_doubles(_SUMREGS_UNROLLED, kw)

    def sumregs_unrolled_denoise(self, x, fetch=True, **kw):
        """sumregs_denoise(x) with rho = 0 -- the same u bit for bit -- that also records the tape of the iterations in
        the handle, for sumregs_unrolled_vjp with the same x and params (bpltv_sumregs_unrolled_denoise)."""
        return self._solve(_SUMREGS_UNROLLED, x, fetch, kw)

    def sumregs_unrolled_denoise_device(self, alpha_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_sumregs_unrolled_denoise_device: the parameter (3*am*an doubles) resident in HBM, the result left there
        (u_device_ptr / copy_u_device); tape_ptr: a caller-owned HBM buffer of sumregs_unrolled_tape_doubles(**kw)
        doubles, or None / 0 for the handle's own tape."""
        self._solve_device(_SUMREGS_UNROLLED, alpha_ptr, am, an, kw, tape_ptr=tape_ptr)

    def sumregs_unrolled_vjp(self, x, gu, want_f=True, want_alpha=True, **kw):
        """Vector-Jacobian product of the maxiter-step map u = sumregs_unrolled_denoise(x) for the cotangent gu = dL/du,
        by a reverse sweep over the handle's tape (bpltv_sumregs_unrolled_vjp): (grad_f, grad_x).  x and the params must
        be those of the solve.  gu: (O, N, M); grad_f has its shape (None unless want_f), grad_x the shape of x (None
        unless want_alpha)."""
        return self._vjp(_SUMREGS_UNROLLED, "sumregs_unrolled_vjp", x, gu, (want_f, want_alpha), kw)

    def sumregs_unrolled_vjp_device(self, tape_ptr, alpha_ptr, am, an, gu_ptr, grad_f_ptr, grad_alpha_ptr, **kw):
        """bpltv_sumregs_unrolled_vjp_device: the tape (None / 0: the handle's own), the parameter, gu and the outputs
        resident in HBM (raw device pointers); either output pointer may be 0 / None, not both."""
        self._vjp_device(_SUMREGS_UNROLLED, tape_ptr, alpha_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alpha_ptr), kw)

    def sumregs_unrolled_denoise_each(self, alphas, fetch=True, **kw):
        """sumregs_unrolled_denoise with image k's own three weights alphas[k] (bpltv_sumregs_unrolled_denoise_each):
        sumregs_denoise_each's u bit for bit, and the handle's tape, recorded per image."""
        return self._solve(_SUMREGS_UNROLLED_EACH, alphas, fetch, kw)

    def sumregs_unrolled_denoise_each_device(self, alphas_ptr, am=1, an=1, tape_ptr=None, **kw):
        """bpltv_sumregs_unrolled_denoise_each_device: O parameter blocks (a C-contiguous (O, 3, an, am) array) resident
        in HBM, the result left there; tape_ptr as in sumregs_unrolled_denoise_device."""
        self._solve_device(_SUMREGS_UNROLLED_EACH, alphas_ptr, am, an, kw, tape_ptr=tape_ptr)

    def sumregs_unrolled_vjp_each(self, alphas, gu, want_f=True, want_alpha=True, **kw):
        """sumregs_unrolled_vjp with image k's own block alphas[k], over the handle's per-image tape
        (bpltv_sumregs_unrolled_vjp_each): (grad_f, grad_alphas).  grad_alphas has the shape of alphas; grad_alphas[k]
        is image k's term alone, not summed over the images."""
        return self._vjp(_SUMREGS_UNROLLED_EACH, "sumregs_unrolled_vjp_each", alphas, gu, (want_f, want_alpha), kw)

    def sumregs_unrolled_vjp_each_device(self, tape_ptr, alphas_ptr, am, an, gu_ptr, grad_f_ptr, grad_alphas_ptr, **kw):
        """bpltv_sumregs_unrolled_vjp_each_device: as sumregs_unrolled_vjp_device with O parameter blocks and their O
        gradients (O*3*am*an doubles each) resident in HBM; either output pointer may be 0 / None, not both."""
        self._vjp_device(_SUMREGS_UNROLLED_EACH, tape_ptr, alphas_ptr, am, an, gu_ptr, (grad_f_ptr, grad_alphas_ptr), kw)

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


class _Model(typing.NamedTuple):
    """What tells one model's entries from another's; a core (TVSolver._solve, _vjp, _jvp, ...) reads nothing else."""
    prefix: str               # the entries are bpltv_<prefix><op>[_each][_device]
    parse: typing.Callable    # x -> (a, am, an[, scalar]): _alpha_arg, _sr_alpha_arg, TVSolver._each_arg or TVSolver._sr_each_arg
    slices: int = 1           # parameter slices: 3 for the sum-of-regularisers model
    w: bool = False           # takes the fidelity weight (w, wo) in front of the parameter, and returns grad_w / takes dw
    channels: bool = False    # takes the channel count right after the handle
    sumregs: bool = False     # its params start from bpltv_sumregs_default_params
    taped: bool = False       # unrolled: solve and vjp take checkpoint_every= and a tape, jvp and gauss_newton sweep the iterations
    each: bool = False        # one parameter block per image

    def entry(self, op, device=False):
        return "bpltv_%s%s%s%s" % (self.prefix, op, "_each" if self.each else "", "_device" if device else "")

    def unrolled(self):
        return self._replace(prefix=self.prefix + "unrolled_", taped=True)


# one row per model: a new data term or model is a row here and its public methods' docstrings on TVSolver
_TV = _Model("", _alpha_arg)
_TV_EACH = _Model("", TVSolver._each_arg, each=True)
_SUMREGS = _Model("sumregs_", _sr_alpha_arg, slices=3, sumregs=True)
_SUMREGS_EACH = _Model("sumregs_", TVSolver._sr_each_arg, slices=3, sumregs=True, each=True)
_WEIGHTED = _Model("weighted_", _alpha_arg, w=True)
_L1 = _Model("lone_", _alpha_arg, w=True)
_KL = _Model("kl_", _alpha_arg, w=True)
_COLOR = _Model("color_", _alpha_arg, channels=True)
_COLOR_WEIGHTED = _Model("color_weighted_", _alpha_arg, w=True, channels=True)
_UNROLLED, _UNROLLED_EACH = _TV.unrolled(), _TV_EACH.unrolled()
_SUMREGS_UNROLLED, _SUMREGS_UNROLLED_EACH = _SUMREGS.unrolled(), _SUMREGS_EACH.unrolled()
_WEIGHTED_UNROLLED, _L1_UNROLLED, _KL_UNROLLED = _WEIGHTED.unrolled(), _L1.unrolled(), _KL.unrolled()
_COLOR_UNROLLED, _COLOR_WEIGHTED_UNROLLED = _COLOR.unrolled(), _COLOR_WEIGHTED.unrolled()


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
