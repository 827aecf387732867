"""What the sixteen autograd Functions of bpldenoising_amd/torch_layer.py ask of the library, call by call: for each of the
eleven models the sequence of TVSolver calls of a forward pass, of backward with every gradient, of backward with
alpha.grad alone and (where a jvp exists) of one forward_ad pass with a tangent on f, against lists written out here -- the
order within a call, which output and tangent pointers are None, when f is installed again, which keywords travel.  The
values are the other test_gpu_*torch_layer*.py files' business.

torch_layer._solver is replaced by a wrapper that returns a recording proxy around the real TVSolver: every method call is
logged as (name, positional arguments, keyword arguments) and forwarded.  A count, flag or None is logged as itself, anything
else among the positional arguments -- a device address -- as P, and so are the keywords tape_ptr and u_ptr."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

P = "set"
B, C, H, W = 2, 3, 9, 12
KW = {"maxiter": 5}
CK = {"maxiter": 5, "checkpoint_every": 2}
SDD = ("set_data_device", (P, P), {})
COPY = ("copy_u_device", (P,), {})


class Recorder:
    def __init__(self, solver, log):
        self._solver, self._log = solver, log

    def __getattr__(self, name):
        attr = getattr(self._solver, name)
        if not callable(attr):
            return attr

        def call(*args, **kw):
            small = lambda v: v if v is None or (isinstance(v, (bool, int)) and abs(v) < 4096) else P   # data_ptr() is an int too
            self._log.append((name, tuple(small(a) for a in args),
                              {k: small(v) if k in ("tape_ptr", "u_ptr") else v for k, v in kw.items()}))
            return attr(*args, **kw)
        return call


@pytest.fixture
def calls(gpu_solver_cls, monkeypatch):
    from bpldenoising_amd import torch_layer
    log, real = [], torch_layer._solver
    monkeypatch.setattr(torch_layer, "_solver", lambda *key: Recorder(real(*key), log))
    return log


def implicit(solve, vjp, jvp, am, an):
    """forward, backward (all), backward (alpha.grad alone), the jvp call(s) behind a forward pass: reg travels as a keyword."""
    kw = dict(reg=False, **KW)
    return ([SDD, (solve, (P, am, an), KW), COPY],
            [(vjp, (P, P, am, an, P, P, P), kw)],
            [(vjp, (P, P, am, an, P, None, P), kw)],
            jvp and [(jvp, (P, P, am, an, P, None, P), dict(ndir=1, **kw))])


def unrolled(tape, solve, vjp, jvp, am, an, kw=KW, lead=()):
    """The same four for a taped model; lead: the channel count in front of every argument list.  A checkpointed backward
    installs f again; the tangent sweep installs f, reads no tape and gets no checkpoint_every."""
    again = [SDD] if "checkpoint_every" in kw else []
    return ([(tape, (), kw), SDD, (solve, lead + (P, am, an), dict(tape_ptr=P, **kw)), COPY],
            again + [(vjp, lead + (P, P, am, an, P, P, P), kw)],
            again + [(vjp, lead + (P, P, am, an, P, None, P), kw)],
            jvp and [SDD, (jvp, lead + (P, am, an, P, None, P, None), dict(ndir=1, **KW))])


def weighted(am, an, wo):
    return ([SDD, ("weighted_denoise_device", (P, wo, P, am, an), KW), COPY],
            [("weighted_vjp_device", (P, P, P, wo, P, am, an, P, P, P, P), KW)],
            [("weighted_vjp_device", (P, None, P, wo, P, am, an, P, None, P, None), KW)],   # f's pointer only for w.grad
            None)


def weighted_unrolled(am, an, wo, kw=KW):
    again = [SDD] if "checkpoint_every" in kw else []
    return ([("weighted_unrolled_tape_doubles", (), kw), SDD,
             ("weighted_unrolled_denoise_device", (P, wo, P, am, an), dict(tape_ptr=P, **kw)), COPY],
            [SDD, ("weighted_unrolled_vjp_device", (P, P, wo, P, am, an, P, P, P, P), kw)],   # w.grad reads the dataset
            again + [("weighted_unrolled_vjp_device", (P, P, wo, P, am, an, P, None, P, None), kw)],
            [SDD, ("weighted_unrolled_jvp_device", (P, wo, P, am, an, P, None, None, P, None), dict(ndir=1, **KW))])


def _rows(am, an, wo):
    """name -> (function, base class, forward-mode class or None, alpha's leading shape, solver keywords, the four lists)."""
    from bpldenoising_amd import torch_layer as tl
    T, SR = "unrolled_tape_doubles", "sumregs_unrolled_tape_doubles"
    return {
        "tv": (tl.tv_denoise, "TVDenoiseFunction", "TVDenoiseFunction", (), KW,
               implicit("denoise_device", "vjp_device", "jvp_device", am, an)),
        "tv-each": (tl.tv_denoise_each, "TVDenoiseEachFunction", "TVDenoiseEachFunction", (B,), KW,
                    implicit("denoise_each_device", "vjp_each_device", "jvp_each_device", am, an)),
        "sumregs": (tl.sumregs_denoise, "SumRegsDenoiseFunction", "SumRegsDenoiseForwardFunction", (3,), KW,
                    implicit("sumregs_denoise_device", "sumregs_vjp_device", "sumregs_jvp_device", am, an)),
        "sumregs-each": (tl.sumregs_denoise_each, "SumRegsDenoiseEachFunction", "SumRegsDenoiseEachForwardFunction", (B, 3), KW,
                         implicit("sumregs_denoise_each_device", "sumregs_vjp_each_device", "sumregs_jvp_each_device", am, an)),
        "weighted": (tl.tv_denoise_weighted, "TVDenoiseWeightedFunction", None, (), KW, weighted(am, an, wo)),
        "unrolled": (tl.tv_denoise_unrolled, "TVDenoiseUnrolledFunction", "TVDenoiseUnrolledForwardFunction", (), KW,
                     unrolled(T, "unrolled_denoise_device", "unrolled_vjp_device", "unrolled_jvp_device", am, an)),
        "unrolled-ck": (tl.tv_denoise_unrolled, "TVDenoiseUnrolledFunction", "TVDenoiseUnrolledForwardFunction", (), CK,
                        unrolled(T, "unrolled_denoise_device", "unrolled_vjp_device", "unrolled_jvp_device", am, an, CK)),
        "unrolled-each": (tl.tv_denoise_unrolled_each, "TVDenoiseUnrolledEachFunction", "TVDenoiseUnrolledEachForwardFunction",
                          (B,), KW, unrolled(T, "unrolled_denoise_each_device", "unrolled_vjp_each_device",
                                             "unrolled_jvp_each_device", am, an)),
        "weighted-unrolled": (tl.tv_denoise_weighted_unrolled, "TVDenoiseWeightedUnrolledFunction",
                              "TVDenoiseWeightedUnrolledForwardFunction", (), KW, weighted_unrolled(am, an, wo)),
        "weighted-unrolled-ck": (tl.tv_denoise_weighted_unrolled, "TVDenoiseWeightedUnrolledFunction",
                                 "TVDenoiseWeightedUnrolledForwardFunction", (), CK, weighted_unrolled(am, an, wo, CK)),
        "sumregs-unrolled": (tl.sumregs_denoise_unrolled, "SumRegsDenoiseUnrolledFunction", None, (3,), KW,
                             unrolled(SR, "sumregs_unrolled_denoise_device", "sumregs_unrolled_vjp_device", None, am, an)),
        "sumregs-unrolled-each": (tl.sumregs_denoise_unrolled_each, "SumRegsDenoiseUnrolledFunction", None, (B, 3), KW,
                                  unrolled(SR, "sumregs_unrolled_denoise_each_device", "sumregs_unrolled_vjp_each_device", None,
                                           am, an)),
        "color-unrolled": (tl.tv_denoise_color_unrolled, "TVDenoiseColorUnrolledFunction", "TVDenoiseColorUnrolledForwardFunction",
                           (), KW, unrolled(T, "color_unrolled_denoise_device", "color_unrolled_vjp_device",
                                            "color_unrolled_jvp_device", am, an, lead=(C,))),
    }


ROWS = ["tv", "tv-each", "sumregs", "sumregs-each", "weighted", "unrolled", "unrolled-ck", "unrolled-each", "weighted-unrolled",
        "weighted-unrolled-ck", "sumregs-unrolled", "sumregs-unrolled-each", "color-unrolled"]
NO_JVP = ["sumregs", "sumregs-each", "weighted", "unrolled", "unrolled-each", "weighted-unrolled", "sumregs-unrolled",
          "sumregs-unrolled-each", "color-unrolled"]


def _inputs(name, lead, patch):
    """(f, alpha[, w]) on the GPU: alpha a scalar / vector or a (2, 3) patch behind its leading shape; w one plane with the
    former, one per image with the latter, > 0 everywhere."""
    rng = np.random.default_rng(11)
    f = rng.random((B, C, H, W) if name.startswith("color") else (B, H, W))
    alpha = 0.05 + 0.05 * rng.random(lead + ((2, 3) if patch else ()))
    extra = (0.5 + rng.random((B, H, W) if patch else (H, W)),) if name.startswith("weighted") else ()
    return [torch.tensor(np.asarray(x), dtype=torch.float64, device="cuda") for x in (f, alpha) + extra]


@pytest.mark.parametrize("patch", [False, True], ids=["scalar", "patch"])
@pytest.mark.parametrize("name", ROWS)
def test_the_library_sees_these_calls_in_this_order(calls, name, patch):
    import torch.autograd.forward_ad as fwAD
    am, an = (3, 2) if patch else (1, 1)                      # a (2, 3) patch is an = 2 rows of am = 3
    fn, base, fwd_cls, lead, kw, (forward, backward, backward_alpha, jvp) = _rows(am, an, B if patch else 1)[name]

    t = [x.clone().requires_grad_(True) for x in _inputs(name, lead, patch)]
    u = fn(*t, **kw)
    assert u.grad_fn.name() == base + "Backward"
    u.sum().backward()
    assert all(x.grad is not None and x.grad.shape == x.shape for x in t)
    assert calls == forward + backward
    del calls[:]

    t = _inputs(name, lead, patch)
    t[1].requires_grad_(True)
    fn(*t, **kw).sum().backward()
    assert t[1].grad.shape == t[1].shape and t[0].grad is None
    assert calls == forward + backward_alpha
    del calls[:]

    if jvp:
        t = _inputs(name, lead, patch)
        t[1].requires_grad_(True)                             # (so that the output has a grad_fn to name)
        with fwAD.dual_level():
            t[0] = fwAD.make_dual(t[0], torch.ones_like(t[0]))
            out = fn(*t, **({} if fwd_cls == base else {"forward_mode": True}), **kw)
            du = fwAD.unpack_dual(out).tangent
            assert out.grad_fn.name() == fwd_cls + "Backward"
            assert du.shape == out.shape and bool(torch.isfinite(du).all())
        assert calls == forward + jvp


@pytest.mark.parametrize("name", NO_JVP)
def test_a_base_without_a_jvp_raises_torch_s_error_under_forward_ad(calls, name):
    import torch.autograd.forward_ad as fwAD
    fn, _, _, lead, kw, (forward, _, _, _) = _rows(1, 1, 1)[name]
    t = _inputs(name, lead, False)
    with fwAD.dual_level():
        t[0] = fwAD.make_dual(t[0], torch.ones_like(t[0]))
        with pytest.raises((NotImplementedError, RuntimeError), match="jvp"):
            fn(*t, **kw)
    assert calls == forward                                   # torch asks for the jvp behind the forward pass
