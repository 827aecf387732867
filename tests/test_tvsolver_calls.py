"""TVSolver, call for call, on a machine without a GPU: what every public method hands the C ABI and what it makes of the answer.

A TVSolver built with __new__ gets a fake library that forwards the two default-params entries to the real one, records every
other call and answers it with a fixed pattern in every output.  _cases() drives every public method through its parameter forms,
weights, want_* subsets, tangents, null pointers, checkpoint spacings, a failing entry, every rejected argument and every pair of
them.  tests/golden/tvsolver_calls.json, which `python tests/test_tvsolver_calls.py --record` wrote from the revision before
TVSolver's bodies were folded into cores, keeps per method the number of cases and the SHA-1 of their logs, per public name the
signature and the SHA-1 of the docstring, and _lib.SYMBOLS with a letter per type; `--dump FILE` writes every log in full, to
compare two revisions when a digest differs.

Encoding of one logged value: ints and bools as they are; "f:<hex>" a float; "p:<value>" a c_void_p; "b:<text>" bytes;
"a:<dtype>:<shape>:<C|N>:<sha1 of the bytes>" a host array read by the entry; "o:<dtype>:<shape>:<C|N>" one it writes (the
header's non-const pointers); "P:<sha1 of the fields>" byref(params); "r:<type>" any other byref output; null is None."""
import ctypes as C
import functools
import hashlib
import inspect
import itertools
import json
import os
import re
import sys

import numpy as np
import pytest
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "tvsolver_calls.json")
M, N, O, CHANNELS, K = 5, 7, 6, 3, 2
# the entries of SYMBOLS no recorded call reaches, and why
NOT_RECORDED = {"bpltv_version": "no method of TVSolver wraps it (the ABI tests read it from the library)",
                "bpltv_create": "__init__, which a solver made with __new__ skips", "bpltv_create_multi": "__init__",
                "bpltv_create_sharded": "__init__", "bpltv_default_params": "forwarded to the library by every params()",
                "bpltv_sumregs_default_params": "forwarded to the library by every sum-of-regularisers params()"}
KW = {"maxiter": 5}


def _arr(shape, k):
    """Exact binary fractions, different for every k."""
    n = int(np.prod(shape, dtype=int))
    return ((np.arange(n) * 7 + k) % 61 + 1.0).reshape(shape) / 64.0


def _sha(b):
    return hashlib.sha1(b).hexdigest()[:12]


def _header_outputs():
    """entry -> indices of the arguments the header declares as written (a pointer to non-const double)."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpltv.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(bpltv_\w+)\s*\(([^)]*)\)", text):
        out[m.group(1)] = {i for i, a in enumerate(m.group(2).split(",")) if "double *" in a and "const" not in a}
    return out


class _Token:
    """What the patched learning_function._ptr hands the fake library: the array itself."""
    def __init__(self, a):
        self.a = a


def _enc(v):
    """A returned value."""
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, np.ndarray):
        return "a:%s:%s:%s:%s" % (v.dtype, v.shape, "C" if v.flags.c_contiguous else "N", _sha(np.ascontiguousarray(v).tobytes()))
    if isinstance(v, float):
        return ("f:" if type(v) is float else "nf:") + float(v).hex()
    if isinstance(v, (tuple, list)):
        return [_enc(x) for x in v]
    if isinstance(v, dict):
        return {k: _enc(x) for k, x in v.items()}
    if isinstance(v, C.Structure):
        return "P:" + _params_sha(v)
    return "?:" + type(v).__name__


def _params_sha(p):
    return _sha(repr([(k, list(getattr(p, k)) if k == "reserved" else (getattr(p, k).hex() if isinstance(getattr(p, k), float)
                                                                            else getattr(p, k))) for k, _ in p._fields_]).encode())


class FakeLib:
    def __init__(self, real, log, outputs, fail):
        self._real, self._log, self._outputs, self._fail = real, log, outputs, fail

    def __getattr__(self, name):
        from bpldenoising_amd import _lib
        if name in ("bpltv_default_params", "bpltv_sumregs_default_params"):
            return getattr(self._real, name)
        if name not in _lib.SYMBOLS:
            raise AttributeError(name)
        return functools.partial(self._call, name)

    def _call(self, name, *args):
        from bpldenoising_amd import _lib
        outs, enc = self._outputs[name], []
        for i, a in enumerate(args):
            if isinstance(a, _Token):
                a = a.a
                assert isinstance(a, np.ndarray)
                flags = "C" if a.flags.c_contiguous else "N"
                if i in outs:
                    enc.append("o:%s:%s:%s" % (a.dtype, a.shape, flags))
                    a.reshape(-1)[:] = (np.arange(a.size) % 251 + 1.0) / 8.0
                else:
                    enc.append("a:%s:%s:%s:%s" % (a.dtype, a.shape, flags, _sha(a.tobytes())))
            elif isinstance(a, C.c_void_p):
                enc.append("p:%s" % a.value)
            elif isinstance(a, bytes):
                enc.append("b:" + a.decode())
            elif isinstance(a, float):
                enc.append("f:" + a.hex())
            elif a is None or isinstance(a, int):
                enc.append(a)
            elif hasattr(a, "_obj"):   # byref(...)
                obj = a._obj
                if isinstance(obj, _lib.BpltvParams):
                    enc.append("P:" + _params_sha(obj))
                else:
                    enc.append("r:" + type(obj).__name__)
                    if isinstance(obj, C.c_double):
                        obj.value = 7.5
                    elif isinstance(obj, C.c_ulonglong):
                        obj.value = 12345
                    elif isinstance(obj, C.c_void_p):
                        obj.value = 0x7000
            else:
                enc.append("?:" + type(a).__name__)
        self._log.append([name] + enc)
        if name == "bpltv_last_error":
            return b"recorded failure"
        return 3 if self._fail and name not in ("bpltv_set_option", "bpltv_destroy") else 0


# ---- the values a parameter name stands for ---------------------------------------------------------------------------------
def _kind(method):
    return ("sr" if "sumregs" in method else "tv") + ("_each" if "each" in method.split("_") else "")


PARAMS = {"tv": [0.3, _arr((2, 3), 1)], "sr": [_arr((3,), 2), _arr((3, 2, 3), 3)],
          "tv_each": [_arr((O,), 4), _arr((O, 2, 3), 5)], "sr_each": [_arr((O, 3), 6), _arr((O, 3, 2, 3), 7)]}
BAD_PARAMS = {"tv": [np.zeros((2, 2, 2))], "sr": [np.zeros(4), np.zeros((2, 2, 3))],
              "tv_each": [np.zeros((O, 2)), np.zeros(O + 1)], "sr_each": [np.zeros((O, 2)), np.zeros((O + 1, 3))]}
BATCH = (O, N, M)
IMAGES = {"u": 10, "f": 11, "gu": 12, "ubar": 13}
WEIGHTS = [_arr((N, M), 20), _arr((O, N, M), 21)]
SWEEPS = {"sweep": [_arr((4,), 30), _arr((4, 2, 3), 31)], "sumregs_sweep": [_arr((4, 3), 32), _arr((4, 3, 2, 3), 33)]}
BAD_SWEEPS = {"sweep": [np.zeros((4, 2))], "sumregs_sweep": [np.zeros((4, 2))]}
KWS = [{}, {"maxiter": 7, "rho": 0.0, "variant": 2, "chains": 1, "adjoint_method": "bcr", "Δt": 1e-5, "verbose_iter": 9}]
SPACINGS = [2, -1, 0]


def _values(method, name, x):
    """(baseline, [other valid values], [rejected values]) of parameter `name` of `method`; x: the parameter of this call."""
    kind = _kind(method)
    if name in ("x", "alphas"):
        if method in SWEEPS:
            return SWEEPS[method][0], SWEEPS[method][1:], BAD_SWEEPS[method]
        if method == "grad_fwd":
            return _arr((N, M), 40), [], []
        return PARAMS[kind][0], PARAMS[kind][1:], BAD_PARAMS[kind]
    if name in IMAGES:
        good = _arr(BATCH, IMAGES[name])
        return good, [], [np.zeros((O, N, M + 1))]
    if name == "w":
        return WEIGHTS[0], WEIGHTS[1:], [np.zeros((M, N)), np.zeros((O + 1, N, M))]
    if name in ("y1", "y2"):
        return _arr((N, M), 41 + (name == "y2")), [], []
    if name == "df":
        return None, [_arr(BATCH, 50), _arr((K,) + BATCH, 51)], [np.zeros((O, N, M + 1)), np.zeros((K, O + 1, N, M))]
    if name in ("dalpha", "dalphas"):
        s = np.shape(x)
        if kind == "tv" and len(s) == 1:
            s = (1,) + s
        return None, [_arr(s, 52), _arr((K,) + s, 53)], [np.zeros(s + (2, 2)), np.zeros((K,) + s + (2,))]
    if name == "dw":
        return None, None, None   # follows w: see _tangent_cases
    if name in ("fetch", "fetch_u", "want_f", "want_alpha", "want_w"):
        return True, [False], []
    if name in ("want_u", "reg"):
        return False, [True], []
    if name == "channels":
        return CHANNELS, [1], []
    if name == "delta":
        return 1e-4, [], []
    if name.endswith("_ptr"):
        return 0x1000 + 0x100 * (sum(map(ord, name)) % 97), [0, None], []
    if name in ("am", "an"):
        return (3 if name == "am" else 2), [], []
    if name == "wo":
        return 1, [O], []
    if name == "ndir":
        return 1, [K], []
    if name == "name":
        return "adjoint_budget_mb", [], []
    if name == "value":
        return 40, [], []
    if name == "maxiter":
        return 50, [1, 7, 1000], [0]
    if name == "model":
        return "tv", ["weighted", "sumregs"], []
    if name == "_sumregs":
        return False, [True], []
    raise KeyError((method, name))


def _public():
    from bpldenoising_amd.learning_function import TVSolver
    return sorted(n for n in vars(TVSolver) if not n.startswith("_"))


def _cases():
    """[(case id, method, kwargs by name, solver keywords, the fake entry fails)]."""
    from bpldenoising_amd.learning_function import TVSolver
    out = []
    for method in _public():
        sig = inspect.signature(getattr(TVSolver, method))
        names = [n for n, p in sig.parameters.items() if n != "self" and p.kind is not p.VAR_KEYWORD]
        has_kw = any(p.kind is p.VAR_KEYWORD for p in sig.parameters.values())
        pname = next((n for n in names if n in ("x", "alphas")), None)
        xs = [None]
        if pname is not None:
            b, others, _ = _values(method, pname, None)
            xs = [b] + others
        for xi, x in enumerate(xs):
            base, alts, bads = {}, {}, {}
            for n in names:
                if n == "dw":
                    continue
                b, others, bad = _values(method, n, x)
                base[n], alts[n], bads[n] = (x if n == pname else b), ([] if n == pname else others), bad
            kw = dict(KW) if has_kw and method != "params" else {}

            def add(tag, args, kw=kw, fail=False):
                out.append(("%s[%d]%s" % (method, xi, tag), method, args, kw, fail))
            add("", base)
            for n in names:   # one valid alternative at a time
                for j, v in enumerate(alts.get(n, [])):
                    add(" %s=%d" % (n, j), dict(base, **{n: v}))
            for n in names:   # defaults left out
                if sig.parameters[n].default is not inspect.Parameter.empty and n not in ("df", "dalpha", "dalphas", "dw"):
                    add(" -%s" % n, {k: v for k, v in base.items() if k != n})
            wants = [n for n in names if n.startswith("want_") and n != "want_u"]
            for combo in itertools.product([True, False], repeat=len(wants)):
                if wants and not all(combo):
                    add(" wants=%s" % "".join("ft"[c] for c in combo), dict(base, **dict(zip(wants, combo))))
            if "w" in names and len(wants) == 3:   # grad_w has the shape of w
                add(" w=1 wants", dict(base, w=WEIGHTS[1]))
            if "f" in names and "want_w" in names:   # weighted_vjp: f may be None unless grad_w is wanted
                add(" f=None", dict(base, f=None))
                add(" f=None want_w=f", dict(base, f=None, want_w=False))
            tnames = [n for n in names if n in ("df", "dalpha", "dalphas")] + (["dw"] if "dw" in names else [])
            if tnames:
                for w in (WEIGHTS if "w" in names else [None]):
                    tb = dict(base, w=w) if w is not None else dict(base)
                    tv = {n: _values(method, n, x) for n in tnames if n != "dw"}
                    if "dw" in tnames:
                        tv["dw"] = (None, [_arr(w.shape, 54), _arr((K,) + w.shape, 55)], [np.zeros(w.shape + (2,))])
                    wt = "" if w is None else " w=%s" % ("NM" if w.ndim == 2 else "ONM")
                    for lead in (0, 1):
                        for r in range(1, len(tnames) + 1):
                            for sub in itertools.combinations(tnames, r):
                                add("%s tangents %s K=%d" % (wt, "+".join(sub), lead), dict(tb, **{n: tv[n][1][lead] for n in sub}))
                    if len(tnames) >= 2:   # a single tangent beside a stack, and two stacks of different heights
                        add("%s tangents mixed" % wt, dict(tb, **{tnames[0]: tv[tnames[0]][1][1], tnames[1]: tv[tnames[1]][1][0]}))
                        add("%s tangents K 2 and 3" % wt, dict(tb, **{tnames[0]: tv[tnames[0]][1][1],
                                                                       tnames[1]: np.concatenate([tv[tnames[1]][1][1]] * 2)[:3]}))
                    if "dw" in tnames:
                        add("%s tangents df K 2 and dw K 3" % wt, dict(tb, df=tv["df"][1][1], dw=np.concatenate([tv["dw"][1][1]] * 2)[:3]))
                    for n in tnames:
                        for j, v in enumerate(tv[n][2]):
                            add("%s tangent bad %s=%d" % (wt, n, j), dict(tb, **{n: v}))
                        if "want_u" in names:
                            add("%s tangent %s want_u" % (wt, n), dict(tb, want_u=True, **{n: tv[n][1][1]}))
                bads = dict(bads, **{n: (_values(method, n, x)[2] if n != "dw" else [np.zeros(WEIGHTS[0].shape + (2,))]) for n in tnames})
                first = {tnames[0]: _values(method, tnames[0], x)[1][0]}   # the rejections below need one tangent to get that far
                base = dict(base, **first)
            # rejected arguments: one at a time, then two at a time (which error wins)
            rejected = [(n, j, v) for n in names for j, v in enumerate(bads.get(n, []))]
            if has_kw and method != "params":
                rejected.append(("kw", 0, None))
            if wants:
                rejected.append(("wants", 0, None))

            def reject(args, kw2, item):
                n, _, v = item
                if n == "kw":
                    kw2["bogus"] = 1
                elif n == "wants":
                    args.update({k: False for k in wants})
                else:
                    args[n] = v
            for item in rejected:
                args, kw2 = dict(base), dict(kw)
                reject(args, kw2, item)
                add(" bad %s=%d" % item[:2], args, kw2)
            for a, b in itertools.combinations(rejected, 2):
                if a[0] == b[0]:
                    continue
                args, kw2 = dict(base), dict(kw)
                reject(args, kw2, a)
                reject(args, kw2, b)
                add(" bad %s=%d %s=%d" % (a[:2] + b[:2]), args, kw2)
            if has_kw and method != "params":
                for j, other in enumerate(KWS):
                    add(" kw=%d" % j, base, other)
                for c in SPACINGS:   # a method without a tape rejects the keyword
                    add(" checkpoint_every=%d" % c, base, dict(kw, checkpoint_every=c))
                add(" checkpoint_every=2 fails", base, dict(kw, checkpoint_every=2), True)
                gu_bad = bads.get("gu")
                if gu_bad:   # rejected after the spacing was set
                    add(" checkpoint_every=2 bad gu", dict(base, gu=gu_bad[0]), dict(kw, checkpoint_every=2))
            if method not in ("params", "auto_checkpoint_every"):
                add(" fails", base, kw, True)
    return out


def _run(case):
    """The log of one case: the ABI calls in order, then what the method returned or raised."""
    from bpldenoising_amd import _lib, learning_function as lf
    _, method, args, kw, fail = case
    log = []
    s = lf.TVSolver.__new__(lf.TVSolver)
    s.M, s.N, s.O, s.dtype = M, N, O, 64
    s._h = C.c_void_p(0xBEEF)
    s._lib = FakeLib(_lib.load(), log, _OUTPUTS, fail)
    if method == "per_image":   # rows of the last evaluate
        s._lib._fail = False
        s.evaluate(PARAMS["tv"][1], 1e-4)
        s._lib._fail = fail
    args = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in args.items()}
    try:
        log.append(["return", _enc(getattr(s, method)(**args, **kw))])
    except Exception as e:   # noqa: BLE001 -- the type and the text are what is recorded
        log.append(["raise", type(e).__name__, str(e)])
    s._h = None   # nothing for __del__ to destroy
    return log


def _symbols():
    """entry -> "<restype>:<argtypes>", one letter per type."""
    from bpldenoising_amd import _lib
    letter = {C.c_int: "i", C.c_double: "f", C.c_void_p: "v", C.c_char_p: "s", C.POINTER(C.c_double): "d", _lib._PP: "P",
              C.POINTER(C.c_void_p): "V", C.POINTER(C.c_int): "I", C.POINTER(C.c_ulonglong): "U", C.POINTER(_lib.BpltvStats): "S"}
    return {k: letter[r] + ":" + "".join(letter[a] for a in args) for k, (r, args) in _lib.SYMBOLS.items()}


def _introspection():
    """public name -> [signature, sha1 of the docstring, kind of attribute]."""
    from bpldenoising_amd.learning_function import TVSolver
    return {n: [str(inspect.signature(getattr(TVSolver, n))), _sha((getattr(TVSolver, n).__doc__ or "").encode()),
                type(inspect.getattr_static(TVSolver, n)).__name__] for n in _public()}


def _digests(logs):
    """method -> [number of cases, sha1 of their ids and logs in order of id]: what the golden file keeps of the logs."""
    out = {}
    for method in _public():
        mine = sorted((k, v) for k, v in logs.items() if k.startswith(method + "["))
        out[method] = [len(mine), _sha(json.dumps(mine).encode())]
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def _all_logs():
    """case id -> log, every case run once with learning_function._ptr handing over the array."""
    from bpldenoising_amd import learning_function as lf
    global _OUTPUTS
    _OUTPUTS = _header_outputs()
    saved, lf._ptr = lf._ptr, _Token
    try:
        cases = _cases()
        logs = {c[0]: _run(c) for c in cases}
        assert len(logs) == len(cases)
        return logs
    finally:
        lf._ptr = saved


@pytest.fixture(scope="module")
def logs():
    return _all_logs()


_OUTPUTS = None


def test_every_case_makes_the_recorded_calls_and_returns_the_recorded_value(golden, logs):
    """Per method, the number of cases and the digest of their logs.  To see what differs, dump the logs of both revisions
    (`python tests/test_tvsolver_calls.py --dump FILE`) and compare the two files."""
    now = _digests(logs)
    assert sorted(now) == sorted(golden["calls"]), set(now) ^ set(golden["calls"])
    bad = [m for m in sorted(now) if now[m] != golden["calls"][m]]
    for m in bad[:3]:
        print("%s: recorded %s, now %s; its first case now:\n  %s" % (m, golden["calls"][m], now[m], json.dumps(logs[m + "[0]"])))
    assert not bad, "%d of %d methods differ: %s" % (len(bad), len(now), bad)


def test_the_cases_cover_what_the_issue_lists(logs):
    """Every public method is driven; every taped one with the spacings 2, -1 and 0 and with a failing entry, and the option is
    back at 0 after each; no other method sets it."""
    taped = 0
    for method in _public():
        mine = {k: v for k, v in logs.items() if k.startswith(method + "[")}
        assert mine, method
        options = [c for v in mine.values() for c in v if c[0] == "bpltv_set_option" and c[2] == "b:tape_checkpoint"]
        if not re.search(r"unrolled_(tape_doubles|denoise|vjp)", method):
            assert not options, method
            continue
        taped += 1
        for k, v in mine.items():
            sets = [c[3] for c in v if c[0] == "bpltv_set_option"]
            m = re.search(r"checkpoint_every=(-?\d+)", k)
            c = float(m.group(1)) if m else 0.0
            reached = bool(sets)   # a call rejected before the params sets nothing
            assert sets == ([("f:" + c.hex())] + (["f:" + 0.0.hex()] if c else []) if reached else []), (k, v)
            if "fails" in k:
                assert v[-1][:2] == ["raise", "BpltvError"], (k, v)
    assert taped == 39


def test_signatures_docstrings_and_names_are_the_recorded_ones(golden):
    now = _introspection()
    assert sorted(now) == sorted(golden["public"])
    for n in now:
        assert now[n] == golden["public"][n], n


def test_symbols_are_the_recorded_ones(golden):
    now = _symbols()
    assert sorted(now) == sorted(golden["symbols"])
    for k in now:
        assert now[k] == golden["symbols"][k], k


def test_every_symbol_is_reached_or_listed(logs):
    from bpldenoising_amd import _lib
    reached = {c[0] for v in logs.values() for c in v if c[0].startswith("bpltv_")}
    assert set(_lib.SYMBOLS) - reached == set(NOT_RECORDED), (set(_lib.SYMBOLS) - reached) ^ set(NOT_RECORDED)


def record(path=GOLDEN, full=False):
    """The golden file, or with full=True every case's whole log for comparing two revisions by hand."""
    logs = _all_logs()
    doc = logs if full else {"calls": _digests(logs), "public": _introspection(), "symbols": _symbols()}
    with open(path, "w") as fh:   # one line per case, method, name or entry
        if full:
            fh.write("{\n%s\n}\n" % ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in doc.items()))
        else:
            fh.write("{\n%s\n}\n" % ",\n".join("%s: {\n%s\n}" % (json.dumps(sec), ",\n".join(
                " %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(d.items()))) for sec, d in doc.items()))
    print("%d cases, %d bytes" % (len(logs), os.path.getsize(path)))


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        record()
    else:
        assert len(sys.argv) == 3 and sys.argv[1] == "--dump", "usage: --record | --dump FILE"
        record(sys.argv[2], full=True)
