"""ctypes binding of libebfi_hip.so (the C ABI declared in include/ebfi_hip.h).

This is the only place the host code touches the native library.  The header is the single description
of the ABI: at import ``parse_header`` reads it (text only, no library) into ``SIGNATURES``
{name: (restype, [argtypes])}, ``PARAMS`` {name: [parameter declarations]} and ``CONSTANTS`` (enumerators
and ``#define EBFI_*`` integers), and refuses whatever its type rules do not cover.  A new entry point is
declared in the header and defined in csrc/; nothing is written here.  Loading is lazy and LOUD: if the
shared object is missing, cannot be loaded or lacks a declared symbol, the first use of any op
raises ``EbfiNativeError`` -- there is no CPU or PyTorch fallback anywhere in this package.
"""
import ctypes
import os
import re
import subprocess
import threading

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # .../ebfi-be_amd
REPO_ROOT = os.path.dirname(PKG_ROOT)
# Development variables (EBFI_LIB_PATH below): honoured only in a process started with
# EBFI_DEV=1, so that a stray variable cannot change what a production run, one of its ranks or one of its graph captures
# computes.  No variable selects a kernel: an A/B comparison builds the other tree into a second library (csrc/build.sh with
# EBFI_LIB_OUT / EBFI_OBJ_DIR) and loads it here, or runs two trees.
_DEV = os.environ.get("EBFI_DEV") == "1"


def dev_env(name, default=None):
    return os.environ.get(name, default) if _DEV else default


# EBFI_LIB_PATH: a second build of the library for same-box A/B runs (tools/ab_bench.sh).  The ABI version of whatever is
# loaded must match in every case -- an older build whose entry points changed signature would be called with shifted
# arguments (round-3 advisory).
LIB_PATH = dev_env("EBFI_LIB_PATH") or os.path.join(PKG_ROOT, "lib", "libebfi_hip.so")
HEADER = os.path.join(REPO_ROOT, "include", "ebfi_hip.h")
BUILD_SCRIPT = os.path.join(PKG_ROOT, "csrc", "build.sh")


class EbfiNativeError(RuntimeError):
    pass


_lock = threading.Lock()
_lib = None

_c = ctypes
_vp, _i, _i64 = _c.c_void_p, _c.c_int, _c.c_int64
_SCALARS = {"int": _i, "int64_t": _i64, "size_t": _c.c_size_t, "float": _c.c_float, "double": _c.c_double,
            "uint64_t": _c.c_uint64}
_RETURNS = dict(_SCALARS, **{"void": None, "const char *": _c.c_char_p})
_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"


def _argtype(func, decl):
    """ctypes type of one parameter declaration.  Pointers of any depth travel as c_void_p (the ebfi_prof_*
    out-parameters too: byref() converts to it), `const int64_t name[n]` as POINTER(c_int64); anything else is refused."""
    m = re.fullmatch(r"([\w\s*]*?)(\w+)\s*(\[\d*\])?", decl)
    if not m:
        raise EbfiNativeError("include/ebfi_hip.h: %s: cannot bind parameter `%s`" % (func, decl))
    base = " ".join(t for t in m.group(1).replace("*", " * ").split() if t != "const")
    if m.group(3):
        ctype = _c.POINTER(_i64) if base == "int64_t" else None
    else:
        ctype = _vp if "*" in base else _SCALARS.get(base)
    if ctype is None:
        raise EbfiNativeError("include/ebfi_hip.h: %s: parameter `%s` has no binding rule (`%s`)" % (func, m.group(2), decl))
    return ctype


def parse_header(text):
    """(signatures, params, constants) of a C header text: {name: (restype, [argtypes])}, {name: [parameter declarations]}
    and {NAME: int} of the enumerators and the `#define EBFI_* <integer>` lines.  A pure function of the text; whatever
    it cannot bind by the rules above raises EbfiNativeError -- it never guesses and never skips a declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {k: int(v, 0) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(EBFI_\w+)[ \t]+(%s)[ \t]*$" % _INT, text, flags=re.M)}
    text = re.sub(r"^[ \t]*#ifdef __cplusplus.*?^[ \t]*#endif", " ", text, flags=re.S | re.M)      # extern "C" { ... }
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def enum(m):
        nxt = 0
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            name, _, val = (s.strip() for s in item.partition("="))
            if val and not re.fullmatch(_INT, val):
                raise EbfiNativeError("include/ebfi_hip.h: enumerator %s: `%s` is not an integer literal" % (name, val))
            nxt = constants[name] = int(val, 0) if val else nxt
            nxt += 1
        return " "
    text = re.sub(r"(?:typedef\s+)?enum\s*\w*\s*\{([^}]*)\}\s*\w*\s*;", enum, text)

    signatures, params = {}, {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = re.fullmatch(r"([\w\s*]+?)\s*\b(\w+)\s*\((.*)\)", stmt)
        if not m:
            raise EbfiNativeError("include/ebfi_hip.h: cannot split `%s` into `ret name(params)`" % stmt)
        ret, name, plist = " ".join(m.group(1).replace("*", " * ").split()), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise EbfiNativeError("include/ebfi_hip.h: %s: return type `%s` has no binding rule" % (name, ret))
        decls = [] if plist == "void" else [p.strip() for p in plist.split(",")]
        signatures[name] = (_RETURNS[ret], [_argtype(name, d) for d in decls])
        params[name] = decls
    return signatures, params, constants


try:
    with open(HEADER) as _f:
        SIGNATURES, PARAMS, CONSTANTS = parse_header(_f.read())
except OSError as e:
    raise EbfiNativeError("cannot read the C header %s: %s" % (HEADER, e)) from e

ABI_VERSION = CONSTANTS["EBFI_ABI_VERSION"]
EBFI_F32, EBFI_F32_BF16MMA, EBFI_F32_BF16X3MMA = (CONSTANTS[k] for k in ("EBFI_F32", "EBFI_F32_BF16MMA", "EBFI_F32_BF16X3MMA"))
EBFI_ERR_UNSUPPORTED = CONSTANTS["EBFI_ERR_UNSUPPORTED"]


def declared_symbols():
    """Function names declared in include/ebfi_hip.h: a crude name scan, deliberately independent of parse_header
    (the tests hold the two against each other)."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ebfi_[a-z0-9_]+)\s*\(", text)))


def build(verbose=False):
    """Compile libebfi_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["bash", BUILD_SCRIPT], stdout=out)
    return LIB_PATH


def _counted(fn, name, n):
    def call(*a):
        if len(a) != n:
            raise TypeError("%s takes %d arguments (%s), %d given" % (name, n, ", ".join(PARAMS[name]) or "void", len(a)))
        return fn(*a)
    call.__name__ = name
    return call


def lib():
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise EbfiNativeError(
                "native library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or ebfi-be_amd/csrc/build.sh).  There is no CPU fallback." % LIB_PATH)
        try:
            h = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise EbfiNativeError("cannot load %s: %s" % (LIB_PATH, e)) from e
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(h, name)
            except AttributeError as e:
                raise EbfiNativeError("%s does not export %s" % (LIB_PATH, name)) from e
            fn.restype = res
            fn.argtypes = args
            # ctypes accepts EXTRA positional arguments silently (they are passed after the declared ones and ignored by the
            # callee): a stray argument in front of the stream pointer put every image-reading data gradient on the NULL
            # stream for two hours of round 4.  Every entry point is therefore called through a wrapper that checks the count.
            setattr(h, name, _counted(fn, name, len(args)))
        if h.ebfi_abi_version() != ABI_VERSION:
            raise EbfiNativeError("ABI version mismatch: library %d, binding %d" % (h.ebfi_abi_version(), ABI_VERSION))
        _lib = h
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().ebfi_last_error()
        raise EbfiNativeError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def i64x4(vals):
    return (_c.c_int64 * 4)(*[int(v) for v in vals])


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return _vp(t.data_ptr()) if t is not None else _vp(0)


def stream_ptr(device=None):
    import torch
    return _vp(torch.cuda.current_stream(device).cuda_stream)


def dtype_code(t):
    import torch
    if t.dtype == torch.float32:
        return EBFI_F32
    raise EbfiNativeError("unsupported dtype %s (the ops take float32 tensors, like the reference's)" % t.dtype)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NotImplementedError(
                "ebfi_amd ops run on an MI355X through libebfi_hip.so only; got a %s tensor "
                "(the reference's FAC has no CPU path either: KernelConv2D.py:38-39)" % t.device)


# ------------------------------------------------------------------ profiler helpers
def prof_enable(on=True):
    lib().ebfi_prof_enable(1 if on else 0)


def prof_reset():
    lib().ebfi_prof_reset()


def prof_fold():
    """Fold the pending event pairs into the per-kernel totals (call after torch.cuda.synchronize(), e.g. once per
    step, so that the bounded pending list never overflows).  Returns the number of launches dropped so far."""
    dropped = _i(0)
    lib().ebfi_prof_collect(ctypes.byref(dropped))
    return dropped.value


def prof_collect(strict=True):
    """{label: (launches, total_ms, algorithmic flops, algorithmic bytes)}; call after torch.cuda.synchronize().
    Raises when launches were dropped (pending list full): totals would be silently truncated otherwise."""
    h = lib()
    dropped = _i(0)
    h.ebfi_prof_collect(ctypes.byref(dropped))
    if strict and dropped.value:
        raise EbfiNativeError("profiler dropped %d launches (pending capacity exceeded): fold once per step with "
                              "prof_fold() or raise ebfi_prof_set_capacity" % dropped.value)
    out = {}
    for k in range(h.ebfi_prof_num_kernels()):
        name, n, ms = _c.c_char_p(), _i64(0), _c.c_double(0)
        fl, by = _c.c_double(0), _c.c_double(0)
        h.ebfi_prof_get(k, ctypes.byref(name), ctypes.byref(n), ctypes.byref(ms))
        h.ebfi_prof_get_work(k, ctypes.byref(fl), ctypes.byref(by))
        out[name.value.decode()] = (n.value, ms.value, fl.value, by.value)
    out["__dropped__"] = (dropped.value, 0.0, 0.0, 0.0)
    return out
