"""ctypes binding of the two C-ABI shared objects, derived at import from include/lpformer_hip.h: the header is the only
place an entry point or an ABI constant is written.

There is no fallback: if ``liblpformer_hip.so`` is missing or a call fails, the caller gets an exception.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
INSTALLED_HIP_LIB_PATH = os.path.join(_HERE, "liblpformer_hip.so")
# LPF_HIP_LIB, read once here: a tuning build of the kernel library (tools/variant.sh) to load instead of the installed
# one.  Whatever it names is what is loaded -- a missing file is an error, never a reason to take the installed library.
HIP_LIB_PATH = os.environ.get("LPF_HIP_LIB") or INSTALLED_HIP_LIB_PATH
HOST_LIB_PATH = os.path.join(_HERE, "liblpformer_host.so")

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lpformer_hip.h")
HOST_NAMES = ("lpf_ppr_push_cpu", "lpf_ppr_push_cpu_sources", "lpf_host_free", "lpf_host_abi_version")  # liblpformer_host.so


class LpfError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p, "void": None}
_DECL = re.compile(r"([\w\s*]+?)\b(lpf_\w+)\s*\(([^()]*)\)\s*;")
_PARAM = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*)*)(?:\b\w+)?")


def _argtype(param, where):
    m = _PARAM.fullmatch(param.strip())
    base, stars = (m.group(1), m.group(2).count("*")) if m else (None, 0)
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1:
        return {"int": C.POINTER(C.c_int), "char": C.c_char_p}.get(base, C.c_void_p)
    if stars == 2:
        return C.POINTER(C.c_void_p)
    raise LpfError(f"{where}: no ctypes type for the parameter {param.strip()!r}")


def _const_value(expr, where):
    """An integer expression of decimal literals (optional u suffix), parentheses, unary minus and <<."""
    toks = re.findall(r"\d+[uU]?|<<|[()-]|\S", expr)
    bad = LpfError(f"{where}: {expr.strip()!r} is not an integer expression")

    def unary():
        t = toks.pop(0) if toks else ""
        if t == "-":
            return -unary()
        if t == "(":
            v = shift()
            if not toks or toks.pop(0) != ")":
                raise bad
            return v
        if not t[:1].isdigit():
            raise bad
        return int(t.rstrip("uU"))

    def shift():
        v = unary()
        while toks and toks[0] == "<<":
            toks.pop(0)
            v <<= unary()
        return v

    v = shift()
    if toks:
        raise bad
    return v


def parse_header(text):
    """``(prototypes, constants)`` of a C header in the form of include/lpformer_hip.h: every ``ret lpf_name(params);``
    as name -> (restype, [argtypes]) and every ``#define LPF_NAME value`` as name -> int.  Whatever it cannot read is an
    LpfError, never skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, code = {}, []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = re.match(r"\s*#\s*define\s+(LPF_\w+)(.*)", line)
        if m:
            if m.group(1) in constants:
                raise LpfError(f"{m.group(1)} is defined twice")
            constants[m.group(1)] = _const_value(m.group(2), m.group(1))
    code = "\n".join(code)
    prototypes = {}
    for ret, name, params in _DECL.findall(code):
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in _RETURNS:
            raise LpfError(f"{name}: no ctypes type for the return type {ret!r}")
        if name in prototypes:
            raise LpfError(f"{name} is declared twice")
        params = [] if params.strip() == "void" else params.split(",")
        prototypes[name] = (_RETURNS[ret], [_argtype(p, name) for p in params])
    rest = _DECL.sub(" ", code)
    if not re.fullmatch(r'\s*(extern\s*"C"\s*\{\s*\}\s*)?', rest):
        raise LpfError(f"cannot read this part of the header: {' '.join(rest.split())[:200]!r}")
    return prototypes, constants


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise LpfError(f"the C header was looked for at {HEADER_PATH} "
                       f"(lpformer_amd runs from its source tree): {e}") from None


# The header is the one place an entry point or an ABI constant is written: name -> (restype, [argtypes]) of every
# declaration, LPF_NAME -> int of every #define.
PROTOTYPES, CONST = _read_header()
HOST_PROTOTYPES = {name: PROTOTYPES[name][1] for name in HOST_NAMES}
HIP_PROTOTYPES = {name: args for name, (_, args) in PROTOTYPES.items() if name not in HOST_NAMES}

ABI_VERSION = CONST["LPF_ABI_VERSION"]
FLAG_RELU = CONST["LPF_FLAG_RELU"]
SELECT_ERR_NODE_RANGE = CONST["LPF_SELECT_ERR_NODE_RANGE"]
SELECT_ERR_ITEM_CAP = CONST["LPF_SELECT_ERR_ITEM_CAP"]
SELECT_ERR_ENTRY_CAP = CONST["LPF_SELECT_ERR_ENTRY_CAP"]
ROWS_PERM_LB_WORDS = CONST["LPF_ROWS_PERM_LB_WORDS"]
SELECT4_BLOCK = CONST["LPF_SELECT4_BLOCK"]

_hip = None
_host = None
_recorder = None   # set by `recording(...)`: the launches, pointers and stream hand-overs of the calls made meanwhile
_recorder_thread = None   # ... by THIS thread only: a concurrent sweep or PPR producer on another thread is not captured


def _recording():
    return _recorder if (_recorder is not None and _recorder_thread == threading.get_ident()) else None


class recording:
    """``with recording(rec):`` every entry point fetched through ``hip()`` is handed to ``rec.launch(name, fn)`` (which
    returns what the caller calls instead), every tensor whose address ``ptr()`` hands out to ``rec.keep(t)``, every
    ``stream_wait(a, b)`` to ``rec.wait(a, b)``.  ``lpformer_amd.PlannedScorer`` records one scoring step this way.  One
    recording at a time, from one thread (the hooks are module state)."""

    def __init__(self, rec):
        self.rec = rec

    def __enter__(self):
        global _recorder, _recorder_thread
        if _recorder is not None:
            raise LpfError("a recording is already in progress")
        _recorder, _recorder_thread = self.rec, threading.get_ident()
        return self.rec

    def __exit__(self, *exc):
        global _recorder, _recorder_thread
        _recorder = _recorder_thread = None
        return False


class _RecordingLib:
    def __init__(self, lib, rec):
        self._lib, self._rec = lib, rec

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        return self._rec.launch(name, fn) if name.startswith("lpf_") else fn


def _bind(lib, protos):
    for name in protos:
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = PROTOTYPES[name]
    return lib


def hip():
    """The gfx950 kernel library.  Raises if it has not been built (python __graft_entry__.py build)."""
    global _hip
    if _hip is None:
        if HIP_LIB_PATH != INSTALLED_HIP_LIB_PATH and not os.path.exists(HIP_LIB_PATH):
            raise LpfError(f"LPF_HIP_LIB names {HIP_LIB_PATH}, which does not exist (tools/variant.sh builds and names "
                           "tuning libraries); the installed library is not loaded in its place")
        if not os.path.exists(HIP_LIB_PATH):
            raise LpfError(f"{HIP_LIB_PATH} not found: build it with `make -C lpformer_amd/csrc` "
                           "(or __graft_entry__.build()); lpformer_amd has no non-HIP fallback")
        lib = _bind(C.CDLL(HIP_LIB_PATH), HIP_PROTOTYPES)
        if lib.lpf_abi_version() != ABI_VERSION:
            raise LpfError("liblpformer_hip.so ABI version mismatch; rebuild")
        _hip = lib
    rec = _recording()
    return _hip if rec is None else _RecordingLib(_hip, rec)


def host():
    """The host-side library (PPR producer)."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise LpfError(f"{HOST_LIB_PATH} not found: build it with `make -C lpformer_amd/csrc`")
        lib = _bind(C.CDLL(HOST_LIB_PATH), HOST_PROTOTYPES)
        if lib.lpf_host_abi_version() != ABI_VERSION:
            raise LpfError("liblpformer_host.so ABI version mismatch; rebuild")
        _host = lib
    return _host


def check(rc: int, what: str = ""):
    if rc != 0:
        lib = _hip if _hip is not None else hip()
        msg = lib.lpf_strerror(rc).decode()
        extra = lib.lpf_last_hip_error().decode()
        raise LpfError(f"{what or 'lpformer_hip call'} failed: {msg}" + (f" [{extra}]" if extra else ""))


def ptr(t):
    """Device/host pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    rec = _recording()
    if rec is not None:
        rec.keep(t)
    return t.data_ptr()


def stream_wait(waiter, waited):
    """``waiter.wait_stream(waited)`` -- the one way the scoring path hands work from one stream to another, so that a
    recording sees it."""
    rec = _recording()
    if rec is not None:
        rec.wait(waiter, waited)
    waiter.wait_stream(waited)


def device_info():
    cu, lds, wave = C.c_int(), C.c_int(), C.c_int()
    name = C.create_string_buffer(64)
    check(hip().lpf_device_info(C.byref(cu), C.byref(lds), C.byref(wave), name, 64), "lpf_device_info")
    return {"cu_count": cu.value, "lds_bytes_per_cu": lds.value, "wave_size": wave.value, "arch": name.value.decode()}
