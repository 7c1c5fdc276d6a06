"""ctypes binding of liblidog_amd.so (the C ABI declared in include/lidog_amd.h).

There is NO fallback: if the HIP library is missing or a call fails, this raises."""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# LIDOG_SO: another build of the same library (kernel A/B runs); there is still no fallback behind it
SO_PATH = os.environ.get("LIDOG_SO") or os.path.join(_HERE, "_C", "liblidog_amd.so")

_i32, _i64, _p, _f, _d = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double

HEADER_PATH = os.path.join(_HERE, "..", "include", "lidog_amd.h")
_SCALARS = {"int": ctypes.c_int, "int32_t": _i32, "int64_t": _i64, "uint32_t": ctypes.c_uint32, "float": _f,
            "double": _d}
_POINTEES = set(_SCALARS) | {"void", "char", "uint8_t", "uint16_t", "uint64_t"}
_RETURNS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": _i64, "const char *": ctypes.c_char_p}


def parse_header(text):
    """(argtypes, restypes, abi_version) from the text of include/lidog_amd.h: name -> list of ctypes types, name ->
    ctypes type, LIDOG_ABI_VERSION.  Strict: anything outside the grammar that the header's opening comment states
    raises, so a header this cannot read never yields a shorter table."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    abi = re.search(r"^[ \t]*#[ \t]*define[ \t]+LIDOG_ABI_VERSION[ \t]+(\d+)[ \t]*$", text, re.M)
    if abi is None:
        raise RuntimeError("lidog_amd.h: no `#define LIDOG_ABI_VERSION <number>`")
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{|\}', " ", text, flags=re.M)
    argtypes, restypes = {}, {}
    for stmt in filter(None, (" ".join(re.findall(r"\w+|\S", s)) for s in text.split(";"))):
        m = re.fullmatch(r"(.+?) (lidog_[a-z0-9_]+) \( (.*) \)", stmt)
        if m is None or m.group(1) not in _RETURNS:
            raise RuntimeError(f"lidog_amd.h: not a prototype the binding can read: `{stmt}`")
        ret, name, params = m.groups()
        if name in argtypes:
            raise RuntimeError(f"lidog_amd.h: {name} is declared twice")
        if "(" in params:
            fp = re.search(r"\( \* (\w+)", params)
            raise RuntimeError(f"lidog_amd.h: {name}: function-pointer parameter `{fp.group(1) if fp else params}`")
        args = []
        for param in [] if params == "void" else params.split(" , "):
            kind, _, pname = param.rpartition(" ")
            if not kind or not re.fullmatch(r"[A-Za-z_]\w*", pname) or pname in _POINTEES or pname == "const":
                raise RuntimeError(f"lidog_amd.h: {name}: parameter `{param}` has no name")
            t = re.fullmatch(r"(?:const )?(\w+)((?: \*(?: const)?)*)", kind)
            if t is None or t.group(1) not in (_POINTEES if t.group(2) else _SCALARS):
                raise RuntimeError(f"lidog_amd.h: {name}: parameter `{pname}` has the unknown type `{kind}`")
            args.append(ctypes.POINTER(_p) if kind == "void * *" else _p if t.group(2) else _SCALARS[kind])
        argtypes[name], restypes[name] = args, _RETURNS[ret]
    if len(argtypes) != len(re.findall(r"\blidog_[a-z0-9_]+\s*\(", text)):
        raise RuntimeError("lidog_amd.h: a lidog_ name is followed by `(` outside a prototype")
    return argtypes, restypes, int(abi.group(1))


# Derived once, at import: hipcc holds every definition in csrc/ to its declaration in the header, and this holds the
# binding to the same declarations.  SIGNATURES: name -> argtypes of every entry point but lidog_last_error;
# _RESTYPES: name -> restype.  ABI_VERSION: what load() demands of lidog_abi_version() -- a stale .so would take
# mis-sized arguments without any diagnostic.
if not os.path.exists(HEADER_PATH):
    raise RuntimeError(f"{HEADER_PATH} is missing: the ctypes binding is derived from it")
with open(HEADER_PATH) as _header:
    _ARGTYPES, _RESTYPES, ABI_VERSION = parse_header(_header.read())
SIGNATURES = {name: args for name, args in _ARGTYPES.items() if name != "lidog_last_error"}

_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                f"{SO_PATH} is missing: build it with `python -m lidog_amd.build` (hipcc, gfx950). "
                "lidog_amd has no CPU or torch fallback.")
        L = ctypes.CDLL(SO_PATH)
        have = L.lidog_abi_version()
        if have != ABI_VERSION:
            raise RuntimeError(f"{SO_PATH} is ABI version {have}, this package expects {ABI_VERSION}: rebuild it with "
                               "`python -m lidog_amd.build --force`")
        for name, args in _ARGTYPES.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = _RESTYPES[name]
        _lib = L
    return _lib


def ptr(t):
    """device pointer of a contiguous tensor (None -> NULL)"""
    if t is None:
        return None
    assert t.is_contiguous(), "lidog_amd kernels need contiguous tensors"
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """hipStream_t of torch's current stream on the current device (the raw C query: the python Stream object costs
    ~9 us per call, 2 ms per training step over ~230 launches per pass)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


_fns = {}


def call(name, *args):
    """call a status-returning entry point on the current torch stream; raise on failure"""
    fn = _fns.get(name)
    if fn is None:
        fn = _fns[name] = getattr(load(), name)
    rc = fn(*args, stream())
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {load().lidog_last_error().decode()}")


def call_on(raw_stream, name, *args):
    """the same on an explicit hipStream_t (a stream's .cuda_stream): no switch of torch's current stream"""
    fn = _fns.get(name)
    if fn is None:
        fn = _fns[name] = getattr(load(), name)
    rc = fn(*args, raw_stream)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {load().lidog_last_error().decode()}")


def require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"lidog_amd: {what} must live on the GPU (got {t.device}); there is no CPU path")
