"""ctypes binding of libmft_hip.so (C-ABI declared in include/mft_hip.h).

The product path has no CPU fallback: ``lib()`` raises if the shared library is
missing, and every wrapper raises ``RuntimeError`` on a non-zero return code.
"""
import ctypes
import os
import re

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libmft_hip.so")

_P = ctypes.c_void_p
_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float}


def _ctype(decl, where):
    """ctypes class of one C declaration ``TYPE name``: any pointer is a c_void_p, a scalar must be one of _SCALARS."""
    if "*" in decl:
        return _P
    ctype = _SCALARS.get(" ".join(w for w in decl.split()[:-1] if w != "const"))
    if ctype is None:
        raise RuntimeError("%s: cannot bind `%s` (scalars the binding knows: %s)" % (where, decl, ", ".join(_SCALARS)))
    return ctype


def parse_header(text):
    """C header text -> ({function: (argtypes, restype)}, {struct typedef: _fields_}).  Every statement that is left after the
    comments, preprocessor lines, enums and struct typedefs are taken out must be a prototype ``RET mft_name(ARGS);`` over
    pointers and the _SCALARS; anything else raises -- the binding never guesses."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r'^\s*#.*$|extern\s+"C"\s*\{|enum\s*\w*\s*\{[^}]*\}\s*;', " ", text, flags=re.M)
    protos, structs = {}, {}

    def take_struct(m):
        name, fields = m.group(2), []
        for decl in filter(None, (" ".join(d.split()) for d in m.group(1).split(";"))):
            first, *more = [d.strip() for d in decl.split(",")]
            if "*" in decl and more:
                raise RuntimeError("struct %s: one pointer per declaration, got `%s`" % (name, decl))
            ctype = _ctype(first, "struct " + name)
            fields += [(n, ctype) for n in [re.split(r"[\s*]+", first)[-1]] + more]
        if name in structs:
            raise RuntimeError("struct %s is declared twice" % name)
        structs[name] = fields
        return " "

    text = re.sub(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", take_struct, text, flags=re.S)
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        if stmt == "}":                                    # closes extern "C"
            continue
        m = re.fullmatch(r"([^()]+?)\b(mft_\w+) ?\(([^()]*)\)", stmt)
        if m is None:
            raise RuntimeError("not a prototype the binding understands: `%s`" % stmt)
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if name in protos:
            raise RuntimeError("%s is declared twice" % name)
        argtypes = [] if args in ("", "void") else [_ctype(a, name) for a in args.split(",")]
        protos[name] = (argtypes, None if ret == "void" else _ctype(ret + " " + name, name))
    if not protos:
        raise RuntimeError("no prototype found in the header")
    return protos, structs


def _load_header(name):
    with open(os.path.join(os.path.dirname(PKG), "include", name)) as f:
        return parse_header(f.read())


# include/mft_hip.h is the one copy of the ABI.  SIGNATURES: launcher -> argtypes; RESTYPES: launcher or hook -> restype (None = void)
_protos, _STRUCT_FIELDS = _load_header("mft_hip.h")
# test / A-B hooks (include/mft_hip_testing.h): form selection for tests/ and tools/, never called by the product path
_hooks = _load_header("mft_hip_testing.h")[0]
if set(_protos) & set(_hooks):
    raise RuntimeError("declared in both headers: %s" % sorted(set(_protos) & set(_hooks)))
SIGNATURES = {n: a for n, (a, _) in _protos.items()}
TESTING_SIGNATURES = {n: a for n, (a, _) in _hooks.items()}
RESTYPES = {n: r for n, (_, r) in list(_protos.items()) + list(_hooks.items())}
_structs = {}


def struct(name):
    """The ctypes.Structure of a ``typedef struct`` of include/mft_hip.h (e.g. "MftBnFwdJob"): same field names, order and layout."""
    if name not in _structs:
        _structs[name] = type(name, (ctypes.Structure,), {"_fields_": _STRUCT_FIELDS[name]})
    return _structs[name]


_lib = None


def lib():
    """Load libmft_hip.so; raise loudly if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libmft_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'`; "
                "this package has no CPU or PyTorch fallback" % LIB_PATH)
        # Load order matters on this stack: the library's static initialisers register its code objects with the HIP runtime
        # (the one PyTorch already loaded, same SONAME); if that happens before PyTorch has initialised the device, every
        # later launch from this library fails with hipErrorNoDevice.  So bring the device up through PyTorch first.
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
            torch.empty(1, device="cuda")
        h = ctypes.CDLL(LIB_PATH)
        for name, argtypes in list(SIGNATURES.items()) + list(TESTING_SIGNATURES.items()):
            fn = getattr(h, name)          # AttributeError if the .so lacks a declared symbol
            fn.argtypes = argtypes
            fn.restype = RESTYPES[name]
        _lib = h
    return _lib


MFT_EINVAL = -22


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed with code %d (hipError_t / MFT_EINVAL=-22)" % (what, rc))


def call(name, *args):
    """Run launcher ``name`` of ``lib()`` (a running LaunchTimer stands in); a non-zero status raises."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        check(rc, name)


def try_call(name, *args):
    """``call`` for a launcher with a fallback: False on MFT_EINVAL (outside its domain, nothing ran: the caller takes the other
    route), True on success; any other status raises."""
    rc = getattr(lib(), name)(*args)
    if rc == MFT_EINVAL:
        return False
    check(rc, name)
    return True


class LaunchTimer:
    """Measurement aid: ``with LaunchTimer() as t: ...`` brackets EVERY launcher call made through ``lib()`` inside the block with
    a pair of HIP events recorded on the stream the launcher enqueues on (its last argument), whichever stream that is -- the
    engine's raw priority / CU-masked streams included, which torch.cuda.Event (current stream only) cannot see.
    ``t.collect()`` -> {launcher name: [milliseconds per call, ...]} (synchronises).  A launcher that enqueues several kernels
    is timed as one unit.  Not for use under stream capture (an event record would become a graph node); eager phases only."""

    _SKIP = ("mft_event_", "mft_stream_", "mft_debug_", "mft_version", "mft_device_info", "mft_has_experiments",
             "mft_wgrad_fwd_set_", "mft_probe_placement")

    def __init__(self, only=None, keep_args=False):
        self.only = only                       # optional predicate(name) -> bool
        self.keep_args = keep_args             # also keep each call's C-ABI arguments (shapes: callers derive bytes / flops from them)
        self._pairs = []                       # (name, start, stop, args | None)
        self._free = []
        self._real = None

    def _event(self):
        if self._free:
            return self._free.pop()
        e = ctypes.c_void_p()
        check(self._real.mft_event_create(ctypes.byref(e)), "mft_event_create")
        return e

    def __getattr__(self, name):               # stands in for the CDLL while the block runs
        real = self.__dict__["_real"]
        fn = getattr(real, name)
        sig = SIGNATURES.get(name)
        if (sig is None or not sig or sig[-1] is not _P or name.endswith("_ws_floats") or name.startswith(self._SKIP)
                or (self.only is not None and not self.only(name))):
            return fn

        def timed(*args):
            stream = args[-1]
            a, b = self._event(), self._event()
            real.mft_event_record(a, stream)
            rc = fn(*args)
            if rc != 0:                        # refused (MFT_EINVAL: outside the launcher's domain, the host falls back) -- nothing ran
                self._free += [a, b]
                return rc
            real.mft_event_record(b, stream)
            self._pairs.append((name, a, b, args if self.keep_args else None))
            return rc
        return timed

    def __enter__(self):
        global _lib
        self._real = lib()
        assert not isinstance(self._real, LaunchTimer), "LaunchTimer blocks do not nest"
        _lib = self
        return self

    def __exit__(self, *exc):
        global _lib
        _lib = self._real
        if exc and exc[0] is not None:         # the block raised: nobody will collect() -- do not leave the event pairs behind
            for _, a, b, _ in self._pairs:
                self._free += [a, b]
            self._pairs = []
            self.close()
        return False

    def collect(self, calls=False):
        """-> {launcher: [ms per call, ...]}; ``calls=True``: the flat list [(launcher, ms, args | None), ...] in call order."""
        out, flat = {}, []
        ms = ctypes.c_float()
        for name, a, b, args in self._pairs:
            check(self._real.mft_event_elapsed_ms(a, b, ctypes.byref(ms)), "mft_event_elapsed_ms")
            out.setdefault(name, []).append(float(ms.value))
            flat.append((name, float(ms.value), args))
            self._free += [a, b]
        self._pairs = []
        return flat if calls else out

    def close(self):
        for e in self._free:
            self._real.mft_event_destroy(e)
        self._free = []
