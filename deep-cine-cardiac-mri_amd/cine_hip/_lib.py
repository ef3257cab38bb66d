"""ctypes binding of libcine_hip.so (C ABI: include/cine_hip.h).

The library is looked up next to this file (built in-tree by
``make -C deep-cine-cardiac-mri_amd/csrc`` or ``__graft_entry__.build()``).
Loading is lazy so host-only helpers (synth, metrics) import without it, but
every compute call goes through ``lib()`` and raises ``CineHipError`` if the
library is missing -- there is no CPU fallback.

The header is the only place a signature is written down: ``_SIGS``
(``{name: (restype, [argtypes])}``) is parsed from it at import by
``parse_header``, which refuses any type outside the header's convention
instead of guessing.  A missing or unparsable header is reported by ``lib()``.
"""
import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CINE_HIP_LIB") or os.path.join(_HERE, "libcine_hip.so")   # override: A/B builds of the library
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "cine_hip.h"))


class CineHipError(RuntimeError):
    pass


_SCALARS = {"int": c_int, "long": c_long, "float": c_float, "double": c_double, "size_t": c_size_t}
_PROTO = re.compile(r"(const char ?\*|\w+) ?\b(cine_[a-z0-9_]+) ?\((.*)\)")
_PARAM = re.compile(r"(?:const )?(\w+) ?((?:\*(?: ?const\b)? ?)*)\w*")          # base type, the stars (`const void* const* w`), a name


def _argtype(param: str):
    m = _PARAM.fullmatch(param)
    base, stars = m.groups() if m else (None, None)
    if stars:
        return c_void_p if base != "char" else None       # a string argument would need c_char_p: not part of the convention
    return _SCALARS.get(base)


def parse_header(text: str) -> dict:
    """{name: (restype, [argtypes])} of every prototype in the text of a header written like include/cine_hip.h.

    by-value int / long / float / double / size_t (a leading const ignored) map to their ctypes twins, every pointer argument to
    c_void_p (None, tensor.data_ptr() and ctypes arrays all pass), a ``const char*`` return to c_char_p.  Anything else -- another
    by-value type, a ``char*`` argument, a function pointer, an array, ``...``, another pointer return, a statement that is no
    prototype -- raises ValueError naming the statement: a signature is never guessed.
    """
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)                        # comments
    text = re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", " ", text, flags=re.M)                    # preprocessor lines
    text = re.sub(r'extern\s*"C"\s*\{|^\s*\}\s*$', " ", text, flags=re.M)              # the extern "C" { ... } wrapper
    sigs = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = _PROTO.fullmatch(stmt)
        if not m:
            raise ValueError(f"not a prototype this binding understands: `{stmt}`")
        ret, name, params = m.groups()
        res = c_char_p if "*" in ret else _SCALARS.get(ret)
        args = [_argtype(p.strip()) for p in params.split(",")] if params.strip() not in ("", "void") else []
        if res is None or None in args:
            raise ValueError(f"{name}: a type outside int, long, float, double, size_t, pointer argument, const char* return: `{stmt}`")
        if name in sigs:
            raise ValueError(f"{name}: declared twice")
        sigs[name] = (res, args)
    return sigs


def _load_sigs():
    """The table of HEADER_PATH, parsed once at import; a failure is kept for lib() so that the package imports without the header."""
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read()), None
    except (OSError, ValueError) as e:
        return {}, f"{HEADER_PATH}: cannot derive the ctypes signatures from the C header: {e}"


_SIGS, _SIGS_ERROR = _load_sigs()
_lib = None


def declared_symbols(header_path: str = HEADER_PATH):
    """Every function name include/cine_hip.h declares (used by the symbol-export test)."""
    text = open(header_path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cine_[a-z0-9_]+)\s*\(", text)))


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if _SIGS_ERROR:
            raise CineHipError(_SIGS_ERROR)
        if not os.path.exists(LIB_PATH):
            raise CineHipError(
                f"{LIB_PATH} not found: build it with `make -C deep-cine-cardiac-mri_amd/csrc` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(code: int, what: str = "") -> None:
    if code != 0:
        msg = lib().cine_last_error().decode(errors="replace")
        raise CineHipError(f"{what or 'cine_hip'} failed ({code}): {msg}")
