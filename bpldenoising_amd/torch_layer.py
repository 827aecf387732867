"""PyTorch autograd layers over the TV and the sum-of-regularisers denoisers: u = denoise(f, alpha) as a
differentiable operation.

    u = tv_denoise(f, alpha, reg=False, maxiter=5000)      # forward: one batched PDHG solve on the GPU
    loss(u).backward()                                     # backward: one adjoint solve (bpltv_vjp_device)

f is a float64 tensor of shape (B, H, W) or (H, W) on a ROCm device (torch's "cuda" device type); in the library's
terms O = B, N = H, M = W, the convention of learning_function.py.  alpha is a float64 tensor on the same device: 0-dim
(scalar), (pH, pW) (patch parameter, pH <= H, pW <= W) or (H, W) (pixel map).  The backward pass is the vector-Jacobian
product of include/bpltv.h's bpltv_vjp for the cotangent torch hands it: f.grad and alpha.grad for any loss.  `reg`
selects the reference's gradient_reg linearisation (delta <= delta_t in tv_op_learning_function).  Double backward is
not supported (once_differentiable).

    u = tv_denoise_each(f, alpha, reg=False)               # one parameter per image (bpltv_denoise_each / _vjp_each)

f is then (B, H, W) and alpha float64 of shape (B,) (a scalar per image), (B, pH, pW) (a patch parameter per image) or
(B, H, W) (a map per image) -- what a network that predicts the parameter per sample outputs.  alpha.grad[k] is image k's
term alone.  A separate function: tv_denoise never reads a leading batch dimension off alpha's shape.

    u = sumregs_denoise(f, alpha, reg=False)               # the three-weight model (bpltv_sumregs_*)

alpha is then float64 of shape (3,) (one weight per difference: forward, backward, centred), (3, pH, pW) (patch
parameter) or (3, H, W) (maps); a C-contiguous (3, pH, pW) tensor is already the library's slice layout (an, am =
pH, pW).  The backward pass is bpltv_sumregs_vjp_device's; reg selects sumregs_gradient_reg.

    u = sumregs_denoise_each(f, alpha, reg=False)          # three weights per image (bpltv_sumregs_denoise_each / _vjp_each)

f is then (B, H, W) and alpha float64 of shape (B, 3), (B, 3, pH, pW) or (B, 3, H, W); alpha.grad[k] is image k's term
alone.  A separate function again: sumregs_denoise rejects a leading batch dimension on alpha.

Forward mode: tv_denoise and tv_denoise_each also carry a jvp, so torch.autograd.forward_ad (dual_level, make_dual,
unpack_dual) works through them: the tangent of u is one bpltv_jvp_device / bpltv_jvp_each_device call with one
direction on the u of the forward pass -- the linear map whose transpose backward computes, so forward and reverse
mode agree for both values of reg.  A tangent must be float64 on f's device; an input
without a tangent counts as zero.  As they stand the sum-of-regularisers functions have no forward mode: forward-mode
AD over them raises torch's "not implemented" error, as it always did.  sumregs_denoise(..., forward_mode=True),
sumregs_denoise_each(..., forward_mode=True) and SumRegsDenoise(alpha, forward_mode=True) select functions that carry
the same jvp through bpltv_sumregs_jvp_device / bpltv_sumregs_jvp_each_device (values and backward are bitwise the
same); their reg = 1 patch system is row-scaled, and the library solves with its transpose there, so the identity with
backward holds in that branch too.

    u = tv_denoise_weighted(f, alpha, w)                   # per-pixel data-fidelity weight (bpltv_weighted_*)

min_u 0.5 sum w (u - f)^2 + sum alpha |grad u|: f and alpha as for tv_denoise, w a float64 tensor of shape (H, W) (one
plane for the batch) or f's own shape (B, H, W), on f's device, w >= 0 (> 0 where a gradient is asked for).  backward is
one bpltv_weighted_vjp_device call and returns f.grad, alpha.grad and w.grad (for an (H, W) weight the sum over the
batch); the linearisation is tv_denoise's reg=False.  Like the sum-of-regularisers functions it carries no jvp:
forward-mode AD over it raises torch's "not implemented" error.

    u = tv_denoise_unrolled(f, alpha, maxiter=50)          # reverse mode through the iterations (bpltv_unrolled_*)

f and alpha as for tv_denoise, and the same u bit for bit (rho, init and order must stay 0); but backward is the derivative
of the maxiter-step map itself -- what finite differences of the layer's own output give for any iteration count --
where tv_denoise's is implicit differentiation of the exact minimiser.  The forward pass records the dual before every
projection in a tape it allocates as a torch tensor (2 * maxiter * B*H*W doubles) and saves for backward, which is one
bpltv_unrolled_vjp_device call: a reverse sweep over that tape, no factorisation, no active-set threshold.  Use it for
a layer with a fixed, small iteration count; the reference's learning function uses tv_denoise.  By default it carries no
jvp: forward-mode AD over it raises torch's "not implemented" error.  tv_denoise_unrolled(..., forward_mode=True) and
TVDenoiseUnrolled(alpha, forward_mode=True) select a function whose jvp is one bpltv_unrolled_jvp_device call: a tangent
sweep through the iterations that reads no tape (its forward still records one, so backward works as well).

    u = tv_denoise_unrolled_each(f, alpha, maxiter=30)     # ... with one parameter per image (bpltv_unrolled_*_each)

f is then (B, H, W) and alpha (B,), (B, pH, pW) or (B, H, W), as for tv_denoise_each -- a network that predicts the
parameter per sample in front of a fixed, small number of iterations.  u is tv_denoise_each's bit for bit; forward is
one taped batched solve into a tape tensor of its own, backward one bpltv_unrolled_vjp_each_device call, alpha.grad[k]
image k's term alone; forward_mode=True adds the jvp (one bpltv_unrolled_jvp_each_device call).  A separate function:
tv_denoise_unrolled never reads a leading batch dimension off alpha's shape.  It has no module class: a per-sample
parameter is a network's output, not an nn.Parameter.

    u = tv_denoise_weighted_unrolled(f, alpha, w, maxiter=50)   # ... of the weighted model (bpltv_weighted_unrolled_*)

f, alpha and w as for tv_denoise_weighted, the same u bit for bit, but w may hold zeros wherever it likes: backward is the
derivative of the maxiter-step map (one bpltv_weighted_unrolled_vjp_device call over a tape of 3 * maxiter * B*H*W doubles
the forward pass allocates as a torch tensor), which scales nothing with 1/sqrt(w).  It returns f.grad, alpha.grad and
w.grad as needs_input_grad asks, so alpha, f and a fidelity map can be trained through a masked (inpainting) solve; at
w = 0, w.grad is the one-sided derivative.  The step table (gamma = min w) is held fixed.  By default it carries no jvp;
tv_denoise_weighted_unrolled(..., forward_mode=True) selects a function whose jvp is one bpltv_weighted_unrolled_jvp_device
call: a tangent sweep through the weighted iterations with tangents on f, alpha and w, which reads no tape.

    u = sumregs_denoise_unrolled(f, alpha, maxiter=50)           # ... of the sum-of-regularisers model (bpltv_sumregs_unrolled_*)
    u = sumregs_denoise_unrolled_each(f, alpha, maxiter=30)      # ... with three weights per image

f and alpha as for sumregs_denoise / sumregs_denoise_each, the same u bit for bit; backward is the derivative of the
maxiter-step map (one bpltv_sumregs_unrolled_vjp(_each)_device call over a tape of 6 * maxiter * B*H*W doubles the forward
pass allocates as a torch tensor): no active-set threshold, no factorisation, zeros in alpha allowed.
SumRegsDenoiseUnrolled(alpha, maxiter=...) is the module with a learnable parameter.  No jvp: forward_mode=True raises a
ValueError that names the implicit sumregs_denoise(..., forward_mode=True).

    u = tv_denoise_color_unrolled(f, alpha, maxiter=50)          # colour images: channel-coupled TV (bpltv_color_unrolled_*)

f is (B, C, H, W) or (C, H, W) with 1 <= C <= 4, alpha one 0-dim, (pH, pW) or (H, W) parameter for the batch and the channels.
The model is vectorial TV, 0.5 sum_c |u_c - f_c|^2 + sum alpha sqrt(sum_c |grad u_c|^2): every pixel projects the duals of
its channels onto one ball, so the channels share their edges (reshaping to B*C grey planes is channel-by-channel TV and
gives colour fringes).  Forward is one taped solve into a tape tensor of its own (2 * maxiter * B*C*H*W doubles), backward
one bpltv_color_unrolled_vjp_device call; C = 1 is tv_denoise_unrolled bit for bit.  TVDenoiseColorUnrolled(alpha,
maxiter=50) is the module with a learnable parameter.  The default function has no jvp; tv_denoise_color_unrolled(...,
forward_mode=True) and TVDenoiseColorUnrolled(alpha, forward_mode=True) select a function whose jvp is one
bpltv_color_unrolled_jvp_device call: a tangent sweep through the coupled iterations, which reads no tape.  The other functions
keep refusing 4-D input.

    u = tv_denoise_color_weighted_unrolled(f, alpha, w, maxiter=50)   # ... with a fidelity weight (bpltv_color_weighted_unrolled_*)

f and alpha as for tv_denoise_color_unrolled, w >= 0 (zeros allowed) of shape (H, W) or f's shape: 0.5 sum_c w_c (u_c - f_c)^2
in place of the fidelity.  One mask for the channels is colour inpainting, a mask per channel demosaicing; the coupled
regulariser fills a masked channel in from the others.  backward is one bpltv_color_weighted_unrolled_vjp_device call over a
tape of 3 * maxiter * B*C*H*W doubles and returns f.grad, alpha.grad and w.grad.  No jvp: forward_mode=True raises a ValueError.

    u = tv_l1_denoise_unrolled(f, alpha, w, maxiter=50)          # TV-L1, for impulse noise (bpltv_lone_unrolled_*)

f, alpha and w as for tv_denoise_weighted_unrolled, but the data term is sum w |u - f|: salt-and-pepper noise, outliers and dead
pixels are removed exactly instead of being smeared, and the rest keeps its contrast.  backward is one
bpltv_lone_unrolled_vjp_device call over a tape of 3 * maxiter * B*H*W doubles and returns f.grad, alpha.grad and w.grad, so a
fidelity map can be trained against impulse noise.  TVL1DenoiseUnrolled(alpha, w, maxiter=50, learn_w=False) is the module: w
is a buffer, or a Parameter with learn_w=True.  No jvp: forward_mode=True raises a ValueError that names
tv_l1_denoise_unrolled_fwd(f, alpha, w, maxiter=50), a separate function with the same u and the same backward whose jvp is one
bpltv_lone_unrolled_jvp_device call: a tangent sweep through the TV-L1 iterations, no tape, tangents on f, alpha and w.  The
module takes forward_mode=True and then runs it.

    u = tv_kl_denoise_unrolled(f, alpha, w, maxiter=50)          # TV-KL, for Poisson noise (bpltv_kl_unrolled_*)

f, alpha and w as for tv_l1_denoise_unrolled, but the data term is the Kullback-Leibler divergence sum w (u - f log u) over u >= 0:
the model for photon counts, whose noise grows with the signal.  f must be finite and >= 0 (zero counts are allowed).  backward is
one bpltv_kl_unrolled_vjp_device call over a tape of 3 * maxiter * B*H*W doubles and returns f.grad, alpha.grad and w.grad.
TVKLDenoiseUnrolled(alpha, w, maxiter=50, learn_w=False) is the module.  No jvp: forward_mode=True raises a ValueError that
names tv_kl_denoise_unrolled_fwd(f, alpha, w, maxiter=50), the same function with a jvp (one bpltv_kl_unrolled_jvp_device call);
TVKLDenoiseUnrolled(..., forward_mode=True) runs it.

Streams: the library runs its kernels on its own HIP streams and blocks until they are done.  Every call below first
synchronises the tensors' current torch stream, so that the library reads inputs torch has finished writing; its
outputs are complete when the call returns.

This module imports torch; `import bpldenoising_amd` does not import this module.
"""
import functools
import math
import typing

import torch
from torch.autograd.function import once_differentiable

from .learning_function import TVSolver

_solvers = {}


def _solver(index, M, N, O):
    """One library handle per (device index, M, N, O), kept for the life of the process (clear_solvers frees them)."""
    key = (index, M, N, O)
    s = _solvers.get(key)
    if s is None:
        s = TVSolver(M, N, O, device=index)
        _solvers[key] = s
    return s


def clear_solvers():
    """Free the cached library handles (their HBM)."""
    for s in _solvers.values():
        s.close()
    _solvers.clear()


def _check_tensors(name, f, alpha):
    """The head of every checker below: two float64 tensors."""
    if not isinstance(f, torch.Tensor) or not isinstance(alpha, torch.Tensor):
        raise TypeError("%s: f and alpha must be torch tensors" % name)
    if f.dtype != torch.float64 or alpha.dtype != torch.float64:
        raise TypeError("%s: f and alpha must be float64 (got %s, %s)" % (name, f.dtype, alpha.dtype))


def _check_device(name, f, alpha):
    """The tail of every checker below: both on one ROCm device."""
    if alpha.device != f.device:
        raise ValueError("%s: alpha is on %s, f on %s" % (name, alpha.device, f.device))
    if f.device.type != "cuda":
        raise ValueError("%s: f must be on a ROCm device, got %s" % (name, f.device))


def _check_args(f, alpha, slices=1):
    """(O, N, M, am, an) of a valid (f, alpha) pair; TypeError / ValueError before any library call.  slices = 3: the
    sum-of-regularisers parameter, a leading dimension of 3 on the TV model's vector / patch / map shapes."""
    name = "sumregs_denoise" if slices == 3 else "tv_denoise"
    _check_tensors(name, f, alpha)
    if f.dim() not in (2, 3) or f.numel() == 0:
        raise ValueError("%s: f must have shape (B, H, W) or (H, W), got %s" % (name, tuple(f.shape)))
    H, W = f.shape[-2], f.shape[-1]
    O = f.shape[0] if f.dim() == 3 else 1
    lead = (3,) if slices == 3 else ()
    shape = tuple(alpha.shape)
    if shape[:len(lead)] != lead:
        shape = None
    else:
        shape = shape[len(lead):]
    if shape == ():
        am = an = 1
    elif shape is not None and len(shape) == 2 and 1 <= shape[0] <= H and 1 <= shape[1] <= W:
        an, am = shape
    elif slices == 3:
        raise ValueError("%s: alpha must be (3,), (3, pH, pW) with pH <= %d, pW <= %d, or (3, %d, %d); got %s"
                         % (name, H, W, H, W, tuple(alpha.shape)))
    else:
        raise ValueError("%s: alpha must be 0-dim, (pH, pW) with pH <= %d, pW <= %d, or (%d, %d); got %s"
                         % (name, H, W, H, W, tuple(alpha.shape)))
    _check_device(name, f, alpha)
    return O, H, W, am, an


def _check_args_each(f, alpha, slices=1, name=None):
    """(O, N, M, am, an) of a valid (f, alpha) pair of tv_denoise_each or (slices = 3: a dimension of 3 behind the batch
    dimension) sumregs_denoise_each; TypeError / ValueError before any library call.  name: the caller in the messages,
    when it is another function with tv_denoise_each's shapes."""
    name = name or ("sumregs_denoise_each" if slices == 3 else "tv_denoise_each")
    _check_tensors(name, f, alpha)
    if f.dim() != 3 or f.numel() == 0:
        raise ValueError("%s: f must have shape (B, H, W), got %s" % (name, tuple(f.shape)))
    B, H, W = f.shape
    shape = tuple(alpha.shape)
    if slices == 3:
        if shape == (B, 3):
            am = an = 1
        elif len(shape) == 4 and shape[:2] == (B, 3) and 1 <= shape[2] <= H and 1 <= shape[3] <= W:
            an, am = shape[2], shape[3]
        else:
            raise ValueError("%s: alpha must be (%d, 3), (%d, 3, pH, pW) with pH <= %d, pW <= %d, or (%d, 3, %d, %d); got %s"
                             % (name, B, B, H, W, B, H, W, shape))
    elif shape == (B,):
        am = an = 1
    elif len(shape) == 3 and shape[0] == B and 1 <= shape[1] <= H and 1 <= shape[2] <= W:
        an, am = shape[1], shape[2]
    else:
        raise ValueError("%s: alpha must be (%d,), (%d, pH, pW) with pH <= %d, pW <= %d, or (%d, %d, %d); got %s"
                         % (name, B, B, H, W, B, H, W, shape))
    _check_device(name, f, alpha)
    return B, H, W, am, an


def _check_args_color(f, alpha, name="tv_denoise_color_unrolled"):
    """(B, C, H, W, am, an) of a valid (f, alpha) pair of tv_denoise_color_unrolled (name: the caller in the messages, when
    it is another function with its shapes); TypeError / ValueError before any library call."""
    _check_tensors(name, f, alpha)
    if f.dim() not in (3, 4) or f.numel() == 0:
        raise ValueError("%s: f must have shape (B, C, H, W) or (C, H, W), got %s" % (name, tuple(f.shape)))
    C, H, W = f.shape[-3], f.shape[-2], f.shape[-1]
    B = f.shape[0] if f.dim() == 4 else 1
    if not 1 <= C <= 4:
        raise ValueError("%s: f has %d channels (1 ... 4)" % (name, C))
    shape = tuple(alpha.shape)
    if shape == ():
        am = an = 1
    elif len(shape) == 2 and 1 <= shape[0] <= H and 1 <= shape[1] <= W:
        an, am = shape
    else:
        raise ValueError("%s: alpha must be 0-dim, (pH, pW) with pH <= %d, pW <= %d, or (%d, %d); got %s"
                         % (name, H, W, H, W, shape))
    _check_device(name, f, alpha)
    return B, C, H, W, am, an


def _check_weight(f, w, name="tv_denoise_weighted"):
    """wo (1, or the planes of f: B, of a colour batch B*C) of a valid weight for f; TypeError / ValueError before any library
    call."""
    if not isinstance(w, torch.Tensor):
        raise TypeError("%s: w must be a torch tensor" % name)
    if w.dtype != torch.float64:
        raise TypeError("%s: w must be float64 (got %s)" % (name, w.dtype))
    H, W = f.shape[-2], f.shape[-1]
    if tuple(w.shape) == (H, W):
        wo = 1
    elif f.dim() >= 3 and tuple(w.shape) == tuple(f.shape):
        wo = f.numel() // (H * W)
    else:
        raise ValueError("%s: w must have shape (%d, %d) or f's shape %s; got %s"
                         % (name, H, W, tuple(f.shape), tuple(w.shape)))
    if w.device != f.device:
        raise ValueError("%s: w is on %s, f on %s" % (name, w.device, f.device))
    return wo


def _sync(device):
    torch.cuda.current_stream(device).synchronize()


def _tangent(t, primal, name):
    """A forward-mode tangent as the contiguous float64 tensor the library reads, or None (no tangent: zero); TypeError
    / ValueError before any library call."""
    if t is None:
        return None
    if t.dtype != torch.float64:
        raise TypeError("forward mode: the tangent of %s must be float64, got %s" % (name, t.dtype))
    if t.numel() != primal.numel() or t.device != primal.device:
        raise ValueError("forward mode: the tangent of %s has shape %s on %s, its primal %s on %s"
                         % (name, tuple(t.shape), t.device, tuple(primal.shape), primal.device))
    return t.detach().contiguous()


def _ptr(t):
    """A tensor's device address; None (the library's NULL: an output nobody wants, a tangent that is zero) stays None."""
    return None if t is None else t.data_ptr()


def _no_checkpoint(solver_kw):
    """solver_kw for a tangent sweep, which reads no tape."""
    return {k: v for k, v in solver_kw.items() if k != "checkpoint_every"}


# ---- the one implementation behind the twenty-one Functions below ----------------------------------------------------------------
# A model is a row of this record; _forward, _backward and _jvp are every Function's three methods, written once over it.
# The TVSolver entries are named, not held: they are looked up on the handle of the call.  Their argument lists mirror the C
# ABI and are not regular -- the channel count first, `w, wo` in front of alpha, the tape first in a vjp, a trailing u_ptr in
# an unrolled jvp -- so the three functions splice them.
class _Model(typing.NamedTuple):
    check: typing.Callable   # (f, alpha) -> (O, N, M, am, an), with channels (B, C, N, M, am, an); raises before any library call
    solve: str               # TVSolver's solve ...
    vjp: str                 # ... and the one call of backward
    jvp: typing.Optional[str] = None    # the one call of the tangent; None: the model has no forward mode
    tape: typing.Optional[str] = None   # the entry that sizes the tape of an unrolled model; None: implicit differentiation at u
    slices: int = 1          # parameter planes: 3 in the sum-of-regularisers model
    each: bool = False       # a parameter per image: alpha.grad is written in alpha's own shape
    w: typing.Optional[str] = None      # a per-pixel weight behind alpha: the caller's name in the messages of its check
    w_zeros: bool = False    # ... which may hold zeros, so the layer itself refuses what is negative or not finite
    channels: bool = False   # f is (B, C, H, W): the handle holds B*C planes and every entry takes C first
    reads_f: bool = False    # the reverse sweep reads the dataset whatever is asked of it (TV-L1: f decides the branch)
    f_nonneg: bool = False   # the data term needs f >= 0 (TV-KL): the layer itself refuses what is negative or not finite

    @property
    def reg(self):           # the implicit TV and sum-of-regularisers adjoints take the reference's linearisation switch
        return self.tape is None and self.w is None


_check_sr, _check_sr_each = functools.partial(_check_args, slices=3), functools.partial(_check_args_each, slices=3)
_TV =_Model(_check_args, "denoise_device", "vjp_device", "jvp_device")
_TV_EACH = _Model(_check_args_each, "denoise_each_device", "vjp_each_device", "jvp_each_device", each=True)
_SUMREGS = _Model(_check_sr, "sumregs_denoise_device", "sumregs_vjp_device", "sumregs_jvp_device", slices=3)
_SUMREGS_EACH = _Model(_check_sr_each, "sumregs_denoise_each_device", "sumregs_vjp_each_device", "sumregs_jvp_each_device",
                       slices=3, each=True)
_WEIGHTED = _Model(_check_args, "weighted_denoise_device", "weighted_vjp_device", w="tv_denoise_weighted")
_UNROLLED = _Model(_check_args, "unrolled_denoise_device", "unrolled_vjp_device", "unrolled_jvp_device", "unrolled_tape_doubles")
_UNROLLED_EACH = _Model(functools.partial(_check_args_each, name="tv_denoise_unrolled_each"), "unrolled_denoise_each_device",
                        "unrolled_vjp_each_device", "unrolled_jvp_each_device", "unrolled_tape_doubles", each=True)
_WEIGHTED_UNROLLED = _Model(_check_args, "weighted_unrolled_denoise_device", "weighted_unrolled_vjp_device",
                            "weighted_unrolled_jvp_device", "weighted_unrolled_tape_doubles", w="tv_denoise_weighted_unrolled",
                            w_zeros=True)
_SUMREGS_UNROLLED = _Model(_check_sr, "sumregs_unrolled_denoise_device", "sumregs_unrolled_vjp_device", None,
                           "sumregs_unrolled_tape_doubles", slices=3)
_SUMREGS_UNROLLED_EACH = _Model(functools.partial(_check_sr_each, name="sumregs_denoise_unrolled_each"),
                                "sumregs_unrolled_denoise_each_device", "sumregs_unrolled_vjp_each_device", None,
                                "sumregs_unrolled_tape_doubles", slices=3, each=True)
_COLOR_UNROLLED = _Model(_check_args_color, "color_unrolled_denoise_device", "color_unrolled_vjp_device",
                         "color_unrolled_jvp_device", "unrolled_tape_doubles", channels=True)
_COLOR_WEIGHTED_UNROLLED = _Model(functools.partial(_check_args_color, name="tv_denoise_color_weighted_unrolled"),
                                  "color_weighted_unrolled_denoise_device", "color_weighted_unrolled_vjp_device", None,
                                  "weighted_unrolled_tape_doubles", w="tv_denoise_color_weighted_unrolled", w_zeros=True,
                                  channels=True)
_L1_UNROLLED = _Model(_check_args, "l1_unrolled_denoise_device", "l1_unrolled_vjp_device", None, "weighted_unrolled_tape_doubles",
                      w="tv_l1_denoise_unrolled", w_zeros=True, reads_f=True)
_KL_UNROLLED = _Model(_check_args, "kl_unrolled_denoise_device", "kl_unrolled_vjp_device", None, "weighted_unrolled_tape_doubles",
                      w="tv_kl_denoise_unrolled", w_zeros=True, reads_f=True, f_nonneg=True)
# ... and the same two with the tangent sweep (tv_l1_denoise_unrolled_fwd, tv_kl_denoise_unrolled_fwd): rows of their own, as the
# two above stay without a jvp
_L1_UNROLLED_FWD = _L1_UNROLLED._replace(jvp="l1_unrolled_jvp_device", w="tv_l1_denoise_unrolled_fwd")
_KL_UNROLLED_FWD = _KL_UNROLLED._replace(jvp="kl_unrolled_jvp_device", w="tv_kl_denoise_unrolled_fwd")


def _forward(m, ctx, f, alpha, solver_kw, reg=None, w=None, jvp=False):
    """forward of every Function.  In this order: every check, the cached handle, detached contiguous copies, the tape, _sync,
    f installed, the solve, u fetched; then what backward and (jvp: the class carries one) the tangent need is saved."""
    if m.w:
        if not isinstance(f, torch.Tensor) or f.dim() not in ((3, 4) if m.channels else (2, 3)) or f.numel() == 0:
            m.check(f, alpha)   # raises: f has no (H, W) to hold w against
        wo = _check_weight(f, w, m.w)   # (in front of the device check: a CPU triple with a wrong w reports the w)
        if m.w_zeros and w.numel() and not bool((w.detach() >= 0).all()):   # (a NaN fails the comparison too)
            raise ValueError("%s: w must be finite and >= 0 everywhere (zeros are allowed)" % m.w)
        if m.f_nonneg and not bool((f.detach() >= 0).all() and torch.isfinite(f.detach()).all()):
            raise ValueError("%s: f must be finite and >= 0 everywhere (zero counts are allowed)" % m.w)
    *planes, N, M, am, an = m.check(f, alpha)   # planes: (O,), with channels (B, C)
    index = f.device.index if f.device.index is not None else torch.cuda.current_device()
    s = _solver(index, M, N, math.prod(planes))
    fc = f.detach().contiguous()   # (of (B, C, H, W), colour image b owns the planes b*C ... b*C + C-1)
    ac = alpha.detach().contiguous()
    wc = (w.detach().contiguous(),) if m.w else ()
    u = torch.empty_like(fc)
    lead = ((planes[1],) if m.channels else ()) + ((wc[0].data_ptr(), wo) if m.w else ())
    tape, kw = None, solver_kw
    if m.tape:   # the tape is this call's own: a second forward pass on the handle before backward does not overwrite it
        tape = torch.empty(getattr(s, m.tape)(**solver_kw), dtype=torch.float64, device=f.device)
        kw = dict(tape_ptr=tape.data_ptr(), **solver_kw)
    _sync(f.device)
    s.set_data_device(fc.data_ptr(), fc.data_ptr())   # ubar is not used by a solve
    getattr(s, m.solve)(*lead, ac.data_ptr(), am, an, **kw)
    s.copy_u_device(u.data_ptr())
    # checkpoint_every= (TVSolver's keyword of that name): the "tape" then holds the iteration state every C
    # iterations only, and backward recomputes each segment's tape from it -- the same gradients bit for bit, one more forward
    # solve.  That recompute reads the handle's dataset, so f is saved next to the checkpoints and backward installs it again:
    # another forward pass on the shared solver may have replaced it.  (The weighted models save f anyway: w.grad reads it.)
    x = u if tape is None else tape
    keep_f = (fc,) if tape is not None and solver_kw.get("checkpoint_every") else ()
    ctx.save_for_backward(*((x, fc, ac) + wc if m.w else (x, ac) + keep_f))
    if jvp:
        ctx.save_for_forward(*((u, ac) if tape is None else (fc, ac) + wc))
        ctx.set_materialize_grads(False)   # an input without a tangent reaches jvp as None, and the library as NULL
    ctx.solver, ctx.am, ctx.an, ctx.solver_kw = s, am, an, dict(solver_kw)
    if m.reg:
        ctx.reg = bool(reg)
    if m.w:
        ctx.wo = wo
    if m.channels:
        ctx.channels = planes[1]
    return u


def _backward(m, ctx, gu):
    """backward of every Function: the gradients needs_input_grad asks for from one vjp call (a gradient nobody wants is a NULL
    pointer there), one entry per argument of apply."""
    need = ctx.needs_input_grad
    need_f, need_a, need_w = need[0], need[1], m.w is not None and need[2]
    if gu is None or not (need_f or need_a or need_w):
        return (None,) * len(need)
    x, *rest = ctx.saved_tensors   # x: u, or the tape of an unrolled model
    f, alpha, w = rest if m.w else (rest[1] if len(rest) > 1 else None, rest[0], None)
    gu = gu.to(dtype=torch.float64).contiguous()
    gf = torch.empty_like(gu) if need_f else None
    ga = None
    if need_a:   # a shared parameter: the library's slices * am * an doubles, handed back in alpha's shape
        ga = torch.empty_like(alpha) if m.each else torch.empty(m.slices * ctx.am * ctx.an, dtype=torch.float64, device=gu.device)
    gw = torch.empty_like(w) if need_w else None
    _sync(gu.device)
    s, kw = ctx.solver, ctx.solver_kw
    lead = ((ctx.channels,) if m.channels else ()) + (x.data_ptr(),)
    if m.w:   # the implicit w.grad reads f through a pointer of its own, given only when it is wanted
        lead += (() if m.tape else (_ptr(f if need_w else None),)) + (w.data_ptr(), ctx.wo)
    if m.tape and f is not None and (need_w or m.reads_f or kw.get("checkpoint_every")):
        s.set_data_device(f.data_ptr(), f.data_ptr())   # the unrolled w.grad and a checkpointed sweep's recompute read the dataset
    if m.reg:
        kw = dict(reg=ctx.reg, **kw)
    getattr(s, m.vjp)(*lead, alpha.data_ptr(), ctx.am, ctx.an, gu.data_ptr(), _ptr(gf), _ptr(ga), *((_ptr(gw),) if m.w else ()), **kw)
    grads = (gf, ga.reshape(alpha.shape) if need_a else None) + ((gw,) if m.w else ())
    return grads + (None,) * (len(need) - len(grads))


def _jvp(m, ctx, df, dalpha, dw=None):
    """jvp of every Function that carries one: the tangents checked (None: zero; all None: zero out, no library call), then one
    call with one direction.  An implicit model saved (u, alpha) and solves its linear system at u; an unrolled one saved
    (f, alpha[, w]), installs f and sweeps through the iterations, reading no tape."""
    x, alpha, *w = ctx.saved_tensors
    df, dalpha = _tangent(df, x, "f"), _tangent(dalpha, alpha, "alpha")
    dw = _tangent(dw, w[0], "w") if m.w else None
    if df is None and dalpha is None and dw is None:
        return torch.zeros_like(x)
    du = torch.empty_like(x)
    _sync(x.device)
    s = ctx.solver
    tangents = (_ptr(df), _ptr(dalpha)) + ((_ptr(dw),) if m.w else ())
    if m.tape is None:
        getattr(s, m.jvp)(x.data_ptr(), alpha.data_ptr(), ctx.am, ctx.an, *tangents, du.data_ptr(), ndir=1, reg=ctx.reg,
                          **ctx.solver_kw)
        return du
    lead = ((ctx.channels,) if m.channels else ()) + ((w[0].data_ptr(), ctx.wo) if m.w else ())
    s.set_data_device(x.data_ptr(), x.data_ptr())   # the sweep reads the handle's dataset
    getattr(s, m.jvp)(*lead, alpha.data_ptr(), ctx.am, ctx.an, *tangents, du.data_ptr(), None, ndir=1,
                      **_no_checkpoint(ctx.solver_kw))
    return du


# Each Function below binds the three to its row: forward and jvp with one slot per argument of apply, backward
# once_differentiable.  A ...ForwardFunction is its base with jvp=True in forward and a jvp; backward is inherited.
class TVDenoiseFunction(torch.autograd.Function):
    """autograd.Function of tv_denoise (below); apply(f, alpha, reg, solver_kw)."""
    forward = staticmethod(lambda ctx, f, alpha, reg, solver_kw: _forward(_TV, ctx, f, alpha, solver_kw, reg=reg, jvp=True))
    jvp = staticmethod(lambda ctx, df, dalpha, _reg, _solver_kw: _jvp(_TV, ctx, df, dalpha))
    backward = staticmethod(once_differentiable(lambda ctx, gu: _backward(_TV, ctx, gu)))


def tv_denoise(f, alpha, *, reg=False, **solver_kw):
    """u = denoise(f, alpha) (TVSolver.denoise: the reference's denoise, src/TVLearningFunctionVec.jl:45-70),
    differentiable in f and alpha.  solver_kw: the solver parameters of TVSolver.params (maxiter, ...), used by the
    forward solve and the adjoint alike."""
    return TVDenoiseFunction.apply(f, alpha, reg, solver_kw)


class TVDenoiseEachFunction(torch.autograd.Function):
    """autograd.Function of tv_denoise_each (below); apply(f, alpha, reg, solver_kw)."""
    forward = staticmethod(lambda ctx, f, alpha, reg, solver_kw: _forward(_TV_EACH, ctx, f, alpha, solver_kw, reg=reg, jvp=True))
    jvp = staticmethod(lambda ctx, df, dalpha, _reg, _solver_kw: _jvp(_TV_EACH, ctx, df, dalpha))
    backward = staticmethod(once_differentiable(lambda ctx, gu: _backward(_TV_EACH, ctx, gu)))


def tv_denoise_each(f, alpha, *, reg=False, **solver_kw):
    """u[k] = denoise(f[k], alpha[k]) for a batch f of shape (B, H, W) with one parameter per image: alpha (B,),
    (B, pH, pW) or (B, H, W) on f's device.  One batched solve forward (TVSolver.denoise_each_device) and one adjoint
    solve backward (vjp_each_device); differentiable in f and alpha, alpha.grad[k] being image k's term.  solver_kw: as
    tv_denoise's."""
    return TVDenoiseEachFunction.apply(f, alpha, reg, solver_kw)


class TVDenoise(torch.nn.Module):
    """TV denoising with a learnable parameter: a scalar (alpha = float), a patch parameter or a pixel map
    (alpha = (pH, pW) / (H, W) array).  Move it to the device of its inputs with .to(device)."""

    def __init__(self, alpha, reg=False, **solver_kw):
        super().__init__()
        self.alpha = torch.nn.Parameter(torch.as_tensor(alpha, dtype=torch.float64).clone())
        self.reg = bool(reg)
        self.solver_kw = dict(solver_kw)

    def forward(self, f):
        return tv_denoise(f, self.alpha, reg=self.reg, **self.solver_kw)


class SumRegsDenoiseFunction(torch.autograd.Function):
    """autograd.Function of sumregs_denoise (below); apply(f, alpha, reg, solver_kw)."""
    forward = staticmethod(lambda ctx, f, alpha, reg, solver_kw: _forward(_SUMREGS, ctx, f, alpha, solver_kw, reg=reg))
    backward = staticmethod(once_differentiable(lambda ctx, gu: _backward(_SUMREGS, ctx, gu)))


class SumRegsDenoiseForwardFunction(SumRegsDenoiseFunction):
    """SumRegsDenoiseFunction with a jvp (sumregs_denoise(..., forward_mode=True)): forward and backward are the base
    class's, save_for_forward and set_materialize_grads(False) as the TV functions have them."""
    forward = staticmethod(lambda ctx, f, alpha, reg, solver_kw: _forward(_SUMREGS, ctx, f, alpha, solver_kw, reg=reg, jvp=True))
    jvp = staticmethod(lambda ctx, df, dalpha, _reg, _solver_kw: _jvp(_SUMREGS, ctx, df, dalpha))


def sumregs_denoise(f, alpha, *, reg=False, forward_mode=False, **solver_kw):
    """u = sumregs_denoise(f, alpha) (TVSolver.sumregs_denoise: the reference's sumregs_denoise,
    src/SumRegsLearningFunction.jl:38-85), differentiable in f and alpha.  alpha: (3,), (3, pH, pW) or (3, H, W).
    solver_kw: the solver parameters of TVSolver.params, used by the forward solve and the adjoint alike.
    forward_mode: also usable under torch.autograd.forward_ad (the function then carries a jvp, bpltv_sumregs_jvp_device);
    without it forward-mode AD raises torch's "not implemented" error, as before."""
    fn = SumRegsDenoiseForwardFunction if forward_mode else SumRegsDenoiseFunction
    return fn.apply(f, alpha, reg, solver_kw)


class SumRegsDenoiseEachFunction(torch.autograd.Function):
    """autograd.Function of sumregs_denoise_each (below); apply(f, alpha, reg, solver_kw)."""
    forward = staticmethod(lambda ctx, f, alpha, reg, solver_kw: _forward(_SUMREGS_EACH, ctx, f, alpha, solver_kw, reg=reg))
    backward = staticmethod(once_differentiable(lambda ctx, gu: _backward(_SUMREGS_EACH, ctx, gu)))


class SumRegsDenoiseEachForwardFunction(SumRegsDenoiseEachFunction):
    """SumRegsDenoiseEachFunction with a jvp (sumregs_denoise_each(..., forward_mode=True))."""
    forward = staticmethod(lambda ctx, f, alpha, reg, solver_kw: _forward(_SUMREGS_EACH, ctx, f, alpha, solver_kw, reg=reg, jvp=True))
    jvp = staticmethod(lambda ctx, df, dalpha, _reg, _solver_kw: _jvp(_SUMREGS_EACH, ctx, df, dalpha))


def sumregs_denoise_each(f, alpha, *, reg=False, forward_mode=False, **solver_kw):
    """u[k] = sumregs_denoise(f[k], alpha[k]) for a batch f of shape (B, H, W) with three weights per image: alpha
    (B, 3), (B, 3, pH, pW) or (B, 3, H, W) on f's device.  One batched solve forward
    (TVSolver.sumregs_denoise_each_device) and one adjoint solve backward (sumregs_vjp_each_device); differentiable in f
    and alpha, alpha.grad[k] being image k's term.  solver_kw and forward_mode: as sumregs_denoise's."""
    fn = SumRegsDenoiseEachForwardFunction if forward_mode else SumRegsDenoiseEachFunction
    return fn.apply(f, alpha, reg, solver_kw)


class SumRegsDenoise(torch.nn.Module):
    """Sum-of-regularisers denoising with a learnable weight: a (3,) vector, or a (3, pH, pW) / (3, H, W) array.  Move
    it to the device of its inputs with .to(device)."""

    def __init__(self, alpha, reg=False, forward_mode=False, **solver_kw):
        super().__init__()
        self.alpha = torch.nn.Parameter(torch.as_tensor(alpha, dtype=torch.float64).clone())
        self.reg = bool(reg)
        self.forward_mode = bool(forward_mode)   # usable under torch.autograd.forward_ad (sumregs_denoise)
        self.solver_kw = dict(solver_kw)

    def forward(self, f):
        return sumregs_denoise(f, self.alpha, reg=self.reg, forward_mode=self.forward_mode, **self.solver_kw)


class TVDenoiseWeightedFunction(torch.autograd.Function):
    """autograd.Function of tv_denoise_weighted (below); apply(f, alpha, w, solver_kw).  No jvp."""
    forward = staticmethod(lambda ctx, f, alpha, w, solver_kw: _forward(_WEIGHTED, ctx, f, alpha, solver_kw, w=w))
    backward = staticmethod(once_differentiable(lambda ctx, gu: _backward(_WEIGHTED, ctx, gu)))


def tv_denoise_weighted(f, alpha, w, **solver_kw):
    """u = argmin 0.5 sum w (u - f)^2 + sum alpha |grad u| (TVSolver.weighted_denoise), differentiable in f, alpha and
    w.  w: float64, (H, W) or f's shape (B, H, W), on f's device; w = 1 everywhere is tv_denoise(f, alpha) bit for bit,
    in value and in f.grad / alpha.grad.  solver_kw: the solver parameters of TVSolver.params (rho, init and order must
    stay 0), used by the forward solve and the adjoint alike."""
    return TVDenoiseWeightedFunction.apply(f, alpha, w, solver_kw)


def _with_checkpoint(solver_kw, checkpoint_every):
    """solver_kw with the unrolled layers' checkpoint_every= in it (_forward says what it does)."""
    return solver_kw if checkpoint_every is None else dict(solver_kw, checkpoint_every=int(checkpoint_every))


class TVDenoiseWeightedUnrolledFunction(torch.autograd.Function):
    """autograd.Function of tv_denoise_weighted_unrolled (below); apply(f, alpha, w, solver_kw).  No jvp."""
    forward = staticmethod(lambda ctx, f, alpha, w, solver_kw: _forward(_WEIGHTED_UNROLLED, ctx, f, alpha, solver_kw, w=w))
    backward = staticmethod(once_differentiable(lambda ctx, gu: _backward(_WEIGHTED_UNROLLED, ctx, gu)))


class TVDenoiseWeightedUnrolledForwardFunction(TVDenoiseWeightedUnrolledFunction):
    """TVDenoiseWeightedUnrolledFunction with a jvp (tv_denoise_weighted_unrolled(..., forward_mode=True)): forward is the
    base class's taped solve, so backward keeps working; the jvp is one tangent sweep through the weighted iterations
    (TVSolver.weighted_unrolled_jvp_device, one direction), which reads no tape."""
    forward = staticmethod(lambda ctx, f, alpha, w, solver_kw: _forward(_WEIGHTED_UNROLLED, ctx, f, alpha, solver_kw, w=w, jvp=True))
    jvp = staticmethod(lambda ctx, df, dalpha, dw, _solver_kw: _jvp(_WEIGHTED_UNROLLED, ctx, df, dalpha, dw))


def tv_denoise_weighted_unrolled(f, alpha, w, maxiter=50, checkpoint_every=None, forward_mode=False, **solver_kw):
    """u = weighted_denoise(f, alpha, w) by exactly maxiter PDHG iterations (TVSolver.weighted_unrolled_denoise_device:
    tv_denoise_weighted's u bit for bit at that maxiter), differentiable in f, alpha and w THROUGH the iterations: backward
    is the exact derivative of the maxiter-step map (TVSolver.weighted_unrolled_vjp_device), with the step table held
    fixed.  w: float64, (H, W) or f's shape (B, H, W), on f's device, >= 0 -- zeros are allowed, so a mask can be trained
    through (inpainting), which tv_denoise_weighted's implicit gradient cannot.  solver_kw: the solver parameters of
    TVSolver.params (rho, init and order must stay 0), used by the forward solve and the sweeps alike.  checkpoint_every: as
    tv_denoise_unrolled's.
    forward_mode: also usable under torch.autograd.forward_ad, with tangents on f, alpha and w (the function then carries a
    jvp, a tangent sweep through the weighted iterations, bpltv_weighted_unrolled_jvp_device, which reads no tape and is
    unaffected by checkpoint_every); without it forward-mode AD raises torch's "not implemented" error, as before."""
    fn = TVDenoiseWeightedUnrolledForwardFunction if forward_mode else TVDenoiseWeightedUnrolledFunction
    return fn.apply(f, alpha, w, _with_checkpoint(dict(solver_kw, maxiter=int(maxiter)), checkpoint_every))


class TVDenoiseUnrolledFunction(torch.autograd.Function):
    """autograd.Function of tv_denoise_unrolled (below); apply(f, alpha, solver_kw).  No jvp."""
    forward = staticmethod(lambda ctx, f, alpha, solver_kw: _forward(_UNROLLED, ctx, f, alpha, solver_kw))
    backward = staticmethod(once_differentiable(lambda ctx, gu: _backward(_UNROLLED, ctx, gu)))


class TVDenoiseUnrolledForwardFunction(TVDenoiseUnrolledFunction):
    """TVDenoiseUnrolledFunction with a jvp (tv_denoise_unrolled(..., forward_mode=True)): forward is the base class's
    taped solve, so backward keeps working; the jvp is one tangent sweep through the iterations
    (TVSolver.unrolled_jvp_device, one direction), which reads no tape."""
    forward = staticmethod(lambda ctx, f, alpha, solver_kw: _forward(_UNROLLED, ctx, f, alpha, solver_kw, jvp=True))
    jvp = staticmethod(lambda ctx, df, dalpha, _solver_kw: _jvp(_UNROLLED, ctx, df, dalpha))


class TVDenoiseUnrolledEachFunction(torch.autograd.Function):
    """autograd.Function of tv_denoise_unrolled_each (below); apply(f, alpha, solver_kw).  No jvp."""
    forward = staticmethod(lambda ctx, f, alpha, solver_kw: _forward(_UNROLLED_EACH, ctx, f, alpha, solver_kw))
    backward = staticmethod(once_differentiable(lambda ctx, gu: _backward(_UNROLLED_EACH, ctx, gu)))


class TVDenoiseUnrolledEachForwardFunction(TVDenoiseUnrolledEachFunction):
    """TVDenoiseUnrolledEachFunction with a jvp (tv_denoise_unrolled_each(..., forward_mode=True)): forward is the base
    class's taped solve, so backward keeps working; the jvp is one tangent sweep through the iterations
    (TVSolver.unrolled_jvp_each_device, one direction), which reads no tape."""
    forward = staticmethod(lambda ctx, f, alpha, solver_kw: _forward(_UNROLLED_EACH, ctx, f, alpha, solver_kw, jvp=True))
    jvp = staticmethod(lambda ctx, df, dalpha, _solver_kw: _jvp(_UNROLLED_EACH, ctx, df, dalpha))


def tv_denoise_unrolled_each(f, alpha, forward_mode=False, checkpoint_every=None, **solver_kw):
    """u[k] = denoise(f[k], alpha[k]) by exactly maxiter PDHG iterations, for a batch f of shape (B, H, W) with one
    parameter per image: alpha (B,), (B, pH, pW) or (B, H, W) on f's device -- tv_denoise_each's u bit for bit,
    differentiable THROUGH the iterations as tv_denoise_unrolled is.  One taped batched solve forward
    (TVSolver.unrolled_denoise_each_device) and one reverse sweep backward (unrolled_vjp_each_device); alpha.grad[k] is
    image k's term alone.  solver_kw, forward_mode and checkpoint_every: as tv_denoise_unrolled's (the jvp is one
    unrolled_jvp_each_device call)."""
    fn = TVDenoiseUnrolledEachForwardFunction if forward_mode else TVDenoiseUnrolledEachFunction
    return fn.apply(f, alpha, _with_checkpoint(solver_kw, checkpoint_every))


def tv_denoise_unrolled(f, alpha, forward_mode=False, checkpoint_every=None, **solver_kw):
    """u = denoise(f, alpha) by exactly maxiter PDHG iterations (TVSolver.unrolled_denoise_device: tv_denoise's u bit for
    bit), differentiable in f and alpha THROUGH the iterations: backward is the exact derivative of the maxiter-step map
    (TVSolver.unrolled_vjp_device), not the implicit gradient of the minimiser.  solver_kw: the solver parameters of
    TVSolver.params (rho, init and order must stay 0), used by the forward solve and the sweeps alike.
    forward_mode: also usable under torch.autograd.forward_ad (the function then carries a jvp, a tangent sweep through
    the iterations, bpltv_unrolled_jvp_device); without it forward-mode AD raises torch's "not implemented" error, as
    before.
    checkpoint_every: None / 0 keeps the full tape (2 * maxiter * B*H*W doubles); C >= 1 keeps the iteration state every C
    iterations instead and lets backward recompute the tape segment by segment -- the same gradients bit for bit for one
    more forward solve, in O(sqrt(maxiter)) memory at C = -1 (TVSolver.auto_checkpoint_every).  The tangent sweep of
    forward_mode reads no tape and is unaffected."""
    fn = TVDenoiseUnrolledForwardFunction if forward_mode else TVDenoiseUnrolledFunction
    return fn.apply(f, alpha, _with_checkpoint(solver_kw, checkpoint_every))


class TVDenoiseUnrolled(torch.nn.Module):
    """TVDenoise with tv_denoise_unrolled's backward: a learnable scalar, patch parameter or pixel map behind a fixed
    number of iterations (solver_kw: maxiter, ...).  Move it to the device of its inputs with .to(device).
    forward_mode, checkpoint_every: as tv_denoise_unrolled's."""

    def __init__(self, alpha, forward_mode=False, checkpoint_every=None, **solver_kw):
        super().__init__()
        self.alpha = torch.nn.Parameter(torch.as_tensor(alpha, dtype=torch.float64).clone())
        self.forward_mode = bool(forward_mode)
        self.solver_kw = _with_checkpoint(dict(solver_kw), checkpoint_every)

    def forward(self, f):
        return tv_denoise_unrolled(f, self.alpha, forward_mode=self.forward_mode, **self.solver_kw)


class SumRegsDenoiseUnrolledFunction(torch.autograd.Function):
    """autograd.Function of sumregs_denoise_unrolled and (each) sumregs_denoise_unrolled_each (below);
    apply(f, alpha, each, solver_kw).  No jvp."""

    @staticmethod
    def forward(ctx, f, alpha, each, solver_kw):
        ctx.each = bool(each)
        return _forward(_SUMREGS_UNROLLED_EACH if each else _SUMREGS_UNROLLED, ctx, f, alpha, solver_kw)

    @staticmethod
    @once_differentiable
    def backward(ctx, gu):
        return _backward(_SUMREGS_UNROLLED_EACH if ctx.each else _SUMREGS_UNROLLED, ctx, gu)


def _no_forward_mode(name, forward_mode, what="the sum-of-regularisers iterations",
                     instead="the implicit sumregs_denoise(..., forward_mode=True)"):
    if forward_mode:
        raise ValueError("%s: forward mode through %s does not exist; %s carries a jvp" % (name, what, instead))


def sumregs_denoise_unrolled(f, alpha, maxiter=50, forward_mode=False, checkpoint_every=None, **solver_kw):
    """u = sumregs_denoise(f, alpha) by exactly maxiter PDHG iterations (TVSolver.sumregs_unrolled_denoise_device: the same
    u bit for bit), differentiable in f and the three weights THROUGH the iterations: backward is the exact derivative of
    the maxiter-step map (one sumregs_unrolled_vjp_device call over a tape of 6 * maxiter * B*H*W doubles the forward pass
    allocates as a torch tensor), with no active-set threshold and no factorisation; zeros in alpha are legal.  alpha:
    (3,), (3, pH, pW) or (3, H, W) on f's device.  solver_kw: the solver parameters of TVSolver.params (rho, init and
    order must stay 0).  forward_mode=True raises: use the implicit sumregs_denoise(..., forward_mode=True).
    checkpoint_every: as tv_denoise_unrolled's (here 7 state planes every C iterations against 6 tape planes per iteration)."""
    _no_forward_mode("sumregs_denoise_unrolled", forward_mode)
    return SumRegsDenoiseUnrolledFunction.apply(f, alpha, False, _with_checkpoint(dict(solver_kw, maxiter=maxiter), checkpoint_every))


def sumregs_denoise_unrolled_each(f, alpha, maxiter=30, forward_mode=False, checkpoint_every=None, **solver_kw):
    """sumregs_denoise_unrolled for a batch f of shape (B, H, W) with three weights per image: alpha (B, 3),
    (B, 3, pH, pW) or (B, 3, H, W) -- sumregs_denoise_each's u bit for bit; alpha.grad[k] is image k's term alone.  What
    a network that predicts the weights per sample in front of a short solve needs.  checkpoint_every: as
    sumregs_denoise_unrolled's."""
    _no_forward_mode("sumregs_denoise_unrolled_each", forward_mode)
    return SumRegsDenoiseUnrolledFunction.apply(f, alpha, True, _with_checkpoint(dict(solver_kw, maxiter=maxiter), checkpoint_every))


class SumRegsDenoiseUnrolled(torch.nn.Module):
    """SumRegsDenoise with sumregs_denoise_unrolled's backward: three learnable weights, patch parameters or pixel maps
    behind a fixed number of iterations (solver_kw: maxiter, ...).  Move it to the device of its inputs with .to(device)."""

    def __init__(self, alpha, forward_mode=False, checkpoint_every=None, **solver_kw):
        super().__init__()
        _no_forward_mode("SumRegsDenoiseUnrolled", forward_mode)
        self.alpha = torch.nn.Parameter(torch.as_tensor(alpha, dtype=torch.float64).clone())
        self.solver_kw = _with_checkpoint(dict(solver_kw), checkpoint_every)

    def forward(self, f):
        return sumregs_denoise_unrolled(f, self.alpha, **self.solver_kw)


# ---- channel-coupled TV for colour images (TVSolver.color_unrolled_*): the planes of a colour image share one projection ----
class TVDenoiseColorUnrolledFunction(torch.autograd.Function):
    """autograd.Function of tv_denoise_color_unrolled (below); apply(f, alpha, solver_kw).  No jvp."""
    forward = staticmethod(lambda ctx, f, alpha, solver_kw: _forward(_COLOR_UNROLLED, ctx, f, alpha, solver_kw))
    backward = staticmethod(once_differentiable(lambda ctx, gu: _backward(_COLOR_UNROLLED, ctx, gu)))


class TVDenoiseColorUnrolledForwardFunction(TVDenoiseColorUnrolledFunction):
    """TVDenoiseColorUnrolledFunction with a jvp (tv_denoise_color_unrolled(..., forward_mode=True)): forward is the base
    class's taped solve, so backward keeps working; the jvp is one tangent sweep through the channel-coupled iterations
    (TVSolver.color_unrolled_jvp_device, one direction), which reads no tape."""
    forward = staticmethod(lambda ctx, f, alpha, solver_kw: _forward(_COLOR_UNROLLED, ctx, f, alpha, solver_kw, jvp=True))
    jvp = staticmethod(lambda ctx, df, dalpha, _solver_kw: _jvp(_COLOR_UNROLLED, ctx, df, dalpha))


def tv_denoise_color_unrolled(f, alpha, maxiter=50, checkpoint_every=None, forward_mode=False, **solver_kw):
    """Vectorial TV of colour images by exactly maxiter PDHG iterations: min_u 1/2 sum_c |u_c - f_c|^2 + sum_pixels alpha *
    sqrt(sum_c |grad u_c|^2) -- the channels of an image share one projection per pixel, so an edge is found in all of them
    at once (TVSolver.color_unrolled_denoise_device).  Differentiable in f and alpha through the iterations
    (TVSolver.color_unrolled_vjp_device), as tv_denoise_unrolled.
    f: (B, C, H, W) or (C, H, W), float64, on a ROCm device, 1 <= C <= 4; alpha, shared by the batch and the channels: 0-dim,
    (pH, pW) or (H, W).  checkpoint_every, solver_kw: as tv_denoise_unrolled's.
    forward_mode: also usable under torch.autograd.forward_ad (the function then carries a jvp, a tangent sweep through the
    coupled iterations, TVSolver.color_unrolled_jvp_device, unaffected by checkpoint_every); without it forward-mode AD raises
    torch's "not implemented" error, as before."""
    fn = TVDenoiseColorUnrolledForwardFunction if forward_mode else TVDenoiseColorUnrolledFunction
    return fn.apply(f, alpha, _with_checkpoint(dict(solver_kw, maxiter=int(maxiter)), checkpoint_every))


class TVDenoiseColorUnrolled(torch.nn.Module):
    """tv_denoise_color_unrolled behind a learnable scalar, patch parameter or pixel map.  Move it to the device of its inputs
    with .to(device).  forward_mode: as tv_denoise_color_unrolled's."""

    def __init__(self, alpha, maxiter=50, checkpoint_every=None, forward_mode=False, **solver_kw):
        super().__init__()
        self.alpha = torch.nn.Parameter(torch.as_tensor(alpha, dtype=torch.float64).clone())
        self.maxiter = int(maxiter)
        self.checkpoint_every = checkpoint_every
        self.forward_mode = bool(forward_mode)
        self.solver_kw = dict(solver_kw)

    def forward(self, f):
        return tv_denoise_color_unrolled(f, self.alpha, maxiter=self.maxiter, checkpoint_every=self.checkpoint_every,
                                         forward_mode=self.forward_mode, **self.solver_kw)


# ---- ... with a per-pixel data-fidelity weight (TVSolver.color_weighted_unrolled_*): colour inpainting, demosaicing ----
class TVDenoiseColorWeightedUnrolledFunction(torch.autograd.Function):
    """autograd.Function of tv_denoise_color_weighted_unrolled (below); apply(f, alpha, w, solver_kw).  No jvp."""
    forward = staticmethod(lambda ctx, f, alpha, w, solver_kw: _forward(_COLOR_WEIGHTED_UNROLLED, ctx, f, alpha, solver_kw, w=w))
    backward = staticmethod(once_differentiable(lambda ctx, gu: _backward(_COLOR_WEIGHTED_UNROLLED, ctx, gu)))


def tv_denoise_color_weighted_unrolled(f, alpha, w, maxiter=50, checkpoint_every=None, forward_mode=False, **solver_kw):
    """Vectorial TV of colour images with a per-pixel fidelity weight, by exactly maxiter PDHG iterations: min_u 1/2 sum_c
    sum_pixels w_c (u_c - f_c)^2 + sum_pixels alpha * sqrt(sum_c |grad u_c|^2) (TVSolver.color_weighted_unrolled_denoise_device).
    The channels keep sharing one projection per pixel, so a masked channel is filled in from the others' edges: colour
    inpainting (one mask), demosaicing (a mask per channel), a noise variance per channel.  Differentiable in f, alpha and w
    through the iterations (TVSolver.color_weighted_unrolled_vjp_device), with the step table (gamma = min w) held fixed.
    f and alpha as tv_denoise_color_unrolled's; w: float64 on f's device, >= 0 with zeros allowed, (H, W) -- one plane for the
    batch and the channels, w.grad then summed over them -- or f's shape, one plane per channel.  A (B, 1, H, W) mask goes in
    as w.expand_as(f).contiguous(); autograd sums its gradient over the channels.  checkpoint_every, solver_kw: as
    tv_denoise_unrolled's.  w = 1 everywhere is tv_denoise_color_unrolled's u bit for bit, C = 1 tv_denoise_weighted_unrolled.
    forward_mode=True raises: the tangent sweep of this model is not built."""
    _no_forward_mode("tv_denoise_color_weighted_unrolled", forward_mode, "the weighted channel-coupled iterations",
                     "tv_denoise_color_unrolled(..., forward_mode=True), without a weight,")
    return TVDenoiseColorWeightedUnrolledFunction.apply(f, alpha, w, _with_checkpoint(dict(solver_kw, maxiter=int(maxiter)),
                                                                                       checkpoint_every))


# ---- TV-L1 (TVSolver.l1_unrolled_*): the data term w |u - f|, for salt-and-pepper noise, outliers and dead pixels ----
class TVL1DenoiseUnrolledFunction(torch.autograd.Function):
    """autograd.Function of tv_l1_denoise_unrolled (below); apply(f, alpha, w, solver_kw).  No jvp."""
    forward = staticmethod(lambda ctx, f, alpha, w, solver_kw: _forward(_L1_UNROLLED, ctx, f, alpha, solver_kw, w=w))
    backward = staticmethod(once_differentiable(lambda ctx, gu: _backward(_L1_UNROLLED, ctx, gu)))


def tv_l1_denoise_unrolled(f, alpha, w, maxiter=50, checkpoint_every=None, forward_mode=False, **solver_kw):
    """TV-L1 denoising by exactly maxiter PDHG iterations: min_u sum_pixels w |u - f| + sum_pixels alpha |grad u|
    (TVSolver.l1_unrolled_denoise_device).  The primal step is a soft threshold around f, so an isolated outlier of any height
    is removed exactly and the rest of the image keeps its contrast.  Differentiable in f, alpha and w through the iterations
    (TVSolver.l1_unrolled_vjp_device); the derivative is exact wherever no pixel sits on the threshold.
    f, alpha, w, checkpoint_every and solver_kw as tv_denoise_weighted_unrolled's: w float64 on f's device, >= 0 with zeros
    allowed, (H, W) -- w.grad then summed over the batch -- or f's shape (B, H, W).  accel changes nothing: the data term has no
    strong convexity and the steps are constant.
    forward_mode=True raises: this function carries no jvp; tv_l1_denoise_unrolled_fwd (below) does."""
    _no_forward_mode("tv_l1_denoise_unrolled", forward_mode, "the TV-L1 iterations", "tv_l1_denoise_unrolled_fwd(f, alpha, w, ...)")
    return TVL1DenoiseUnrolledFunction.apply(f, alpha, w, _with_checkpoint(dict(solver_kw, maxiter=int(maxiter)), checkpoint_every))


class TVL1DenoiseUnrolledForwardFunction(TVL1DenoiseUnrolledFunction):
    """TVL1DenoiseUnrolledFunction with a jvp (tv_l1_denoise_unrolled_fwd): forward is the base class's taped solve, so backward
    keeps working; the jvp is one tangent sweep through the TV-L1 iterations (TVSolver.l1_unrolled_jvp_device, one direction),
    which reads no tape."""
    forward = staticmethod(lambda ctx, f, alpha, w, solver_kw: _forward(_L1_UNROLLED_FWD, ctx, f, alpha, solver_kw, w=w, jvp=True))
    jvp = staticmethod(lambda ctx, df, dalpha, dw, _solver_kw: _jvp(_L1_UNROLLED_FWD, ctx, df, dalpha, dw))


def tv_l1_denoise_unrolled_fwd(f, alpha, w, maxiter=50, checkpoint_every=None, **solver_kw):
    """tv_l1_denoise_unrolled -- the same u and the same backward, bit for bit -- that is also usable under
    torch.autograd.forward_ad, with tangents on f, alpha and w: the function carries a jvp, a tangent sweep through the TV-L1
    iterations (bpltv_lone_unrolled_jvp_device), the exact transpose of backward.  It reads no tape and is unaffected by
    checkpoint_every.  A pixel held at f by the threshold moves with f alone."""
    return TVL1DenoiseUnrolledForwardFunction.apply(f, alpha, w, _with_checkpoint(dict(solver_kw, maxiter=int(maxiter)), checkpoint_every))


class TVL1DenoiseUnrolled(torch.nn.Module):
    """tv_l1_denoise_unrolled behind a learnable scalar, patch parameter or pixel map alpha and a fidelity map w: a buffer, or
    with learn_w=True a Parameter too (keep it >= 0, by clamping after the optimiser's step).  Move it to the device of its
    inputs with .to(device).  forward_mode=True: the module runs tv_l1_denoise_unrolled_fwd, usable under
    torch.autograd.forward_ad as well."""

    def __init__(self, alpha, w, maxiter=50, learn_w=False, checkpoint_every=None, forward_mode=False, **solver_kw):
        super().__init__()
        self.alpha = torch.nn.Parameter(torch.as_tensor(alpha, dtype=torch.float64).clone())
        wt = torch.as_tensor(w, dtype=torch.float64).clone()
        if learn_w:
            self.w = torch.nn.Parameter(wt)
        else:
            self.register_buffer("w", wt)
        self.maxiter = int(maxiter)
        self.checkpoint_every = checkpoint_every
        self.forward_mode = bool(forward_mode)
        self.solver_kw = dict(solver_kw)

    def forward(self, f):
        fn = tv_l1_denoise_unrolled_fwd if self.forward_mode else tv_l1_denoise_unrolled
        return fn(f, self.alpha, self.w, maxiter=self.maxiter, checkpoint_every=self.checkpoint_every, **self.solver_kw)


# ---- TV-KL (TVSolver.kl_unrolled_*): the data term w (u - f log u), for Poisson noise (photon counts) ----
class TVKLDenoiseUnrolledFunction(torch.autograd.Function):
    """autograd.Function of tv_kl_denoise_unrolled (below); apply(f, alpha, w, solver_kw).  No jvp."""
    forward = staticmethod(lambda ctx, f, alpha, w, solver_kw: _forward(_KL_UNROLLED, ctx, f, alpha, solver_kw, w=w))
    backward = staticmethod(once_differentiable(lambda ctx, gu: _backward(_KL_UNROLLED, ctx, gu)))


def tv_kl_denoise_unrolled(f, alpha, w, maxiter=50, checkpoint_every=None, forward_mode=False, **solver_kw):
    """TV-KL denoising by exactly maxiter PDHG iterations: min_{u >= 0} sum_pixels w (u - f log u) + sum_pixels alpha |grad u|
    (TVSolver.kl_unrolled_denoise_device), the model for Poisson noise.  The primal step is the closed-form prox of the
    Kullback-Leibler divergence.  Differentiable in f, alpha and w through the iterations (TVSolver.kl_unrolled_vjp_device); the
    derivative is exact wherever the iterates are > 0, which they are wherever w f > 0; where an iterate is exactly 0 (only where
    w f = 0) the data step passes no gradient.
    f must be finite and >= 0 (zero counts are allowed): a ValueError otherwise.  alpha, w, checkpoint_every and solver_kw as
    tv_l1_denoise_unrolled's: w float64 on f's device, >= 0 with zeros allowed, (H, W) -- w.grad then summed over the batch -- or
    f's shape (B, H, W).  accel changes nothing: the steps are constant.
    forward_mode=True raises: this function carries no jvp; tv_kl_denoise_unrolled_fwd (below) does."""
    _no_forward_mode("tv_kl_denoise_unrolled", forward_mode, "the TV-KL iterations", "tv_kl_denoise_unrolled_fwd(f, alpha, w, ...)")
    return TVKLDenoiseUnrolledFunction.apply(f, alpha, w, _with_checkpoint(dict(solver_kw, maxiter=int(maxiter)), checkpoint_every))


class TVKLDenoiseUnrolledForwardFunction(TVKLDenoiseUnrolledFunction):
    """TVKLDenoiseUnrolledFunction with a jvp (tv_kl_denoise_unrolled_fwd): forward is the base class's taped solve, so backward
    keeps working; the jvp is one tangent sweep through the TV-KL iterations (TVSolver.kl_unrolled_jvp_device, one direction),
    which reads no tape."""
    forward = staticmethod(lambda ctx, f, alpha, w, solver_kw: _forward(_KL_UNROLLED_FWD, ctx, f, alpha, solver_kw, w=w, jvp=True))
    jvp = staticmethod(lambda ctx, df, dalpha, dw, _solver_kw: _jvp(_KL_UNROLLED_FWD, ctx, df, dalpha, dw))


def tv_kl_denoise_unrolled_fwd(f, alpha, w, maxiter=50, checkpoint_every=None, **solver_kw):
    """tv_kl_denoise_unrolled -- the same u and the same backward, bit for bit -- that is also usable under
    torch.autograd.forward_ad, with tangents on f, alpha and w: the function carries a jvp, a tangent sweep through the TV-KL
    iterations (bpltv_kl_unrolled_jvp_device), the exact transpose of backward.  It reads no tape and is unaffected by
    checkpoint_every.  f must be finite and >= 0: a ValueError otherwise.  A pixel clamped at zero passes nothing."""
    return TVKLDenoiseUnrolledForwardFunction.apply(f, alpha, w, _with_checkpoint(dict(solver_kw, maxiter=int(maxiter)), checkpoint_every))


class TVKLDenoiseUnrolled(torch.nn.Module):
    """tv_kl_denoise_unrolled behind a learnable scalar, patch parameter or pixel map alpha and a fidelity map w: a buffer, or
    with learn_w=True a Parameter too (keep it >= 0, by clamping after the optimiser's step).  Move it to the device of its
    inputs with .to(device).  forward_mode=True: the module runs tv_kl_denoise_unrolled_fwd, usable under
    torch.autograd.forward_ad as well."""

    def __init__(self, alpha, w, maxiter=50, learn_w=False, checkpoint_every=None, forward_mode=False, **solver_kw):
        super().__init__()
        self.alpha = torch.nn.Parameter(torch.as_tensor(alpha, dtype=torch.float64).clone())
        wt = torch.as_tensor(w, dtype=torch.float64).clone()
        if learn_w:
            self.w = torch.nn.Parameter(wt)
        else:
            self.register_buffer("w", wt)
        self.maxiter = int(maxiter)
        self.checkpoint_every = checkpoint_every
        self.forward_mode = bool(forward_mode)
        self.solver_kw = dict(solver_kw)

    def forward(self, f):
        fn = tv_kl_denoise_unrolled_fwd if self.forward_mode else tv_kl_denoise_unrolled
        return fn(f, self.alpha, self.w, maxiter=self.maxiter, checkpoint_every=self.checkpoint_every, **self.solver_kw)
