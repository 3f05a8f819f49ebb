"""The C signatures of the ctypes bindings, read from include/*.h: the headers are the ABI contract and already state every type.

`signatures(header, types)` parses every `pmhip_* / sgmhip_* / mvsf_* / dmap_* / dimap_*` prototype of a header into `{name: (restype, [argtypes])}`;
`declare(lib, sigs)` sets them on a loaded library.  A type spelling the table below does not know raises, naming the function and the parameter."""
from __future__ import annotations

import ctypes as C
import functools
import os
import re

import numpy as np

_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
_PROTOTYPE = re.compile(r"(?<=[;{}])\s*([\w\s*]+?)\b((?:pmhip|sgmhip|mvsf|dmap|dimap)_\w+)\s*\(([^()]*)\)\s*;")
_PARAMETER = re.compile(r"(.+?)\b\w+\s*(\[\d*\])?")          # type, name, [N]
_SCALARS = {"void": None, "char": C.c_char, "unsigned char": C.c_ubyte, "int": C.c_int, "unsigned": C.c_uint, "unsigned long long": C.c_ulonglong,
            "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int16_t": C.c_int16, "int32_t": C.c_int32,
            "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
_HANDLES = ("pmhip_engine", "sgmhip_engine", "mvsf_scene")   # opaque: the pointer is the value
_BYREF = type(C.byref(C.c_int()))


class _Pointer:
    """Argument class of a `T*` parameter.  Takes None, a C-contiguous numpy array of exactly that element type (writeable unless T is const), a ctypes
    array or pointer of T or `byref` of a T, and a `c_void_p` or integer address (device pointers travel through `const float*`).  `void*` takes any of them."""
    ctype, dtype, const = None, None, True

    @classmethod
    def from_param(cls, a):
        if a is None or isinstance(a, C.c_void_p):
            return a
        if isinstance(a, (int, np.integer)):
            return C.c_void_p(int(a))
        if isinstance(a, np.ndarray):
            if a.flags.c_contiguous and (cls.const or a.flags.writeable) and (cls.dtype is None or a.dtype == cls.dtype):
                return C.c_void_p(a.ctypes.data)
            raise TypeError("expected a C-contiguous%s array of %s, got %s%s%s" % ("" if cls.const else " writeable", cls.dtype or "any type", a.dtype,
                                                                                 "" if a.flags.c_contiguous else ", strided", "" if a.flags.writeable else ", read-only"))
        obj = a._obj if isinstance(a, _BYREF) else a
        if isinstance(a, (C.Array, C._Pointer, _BYREF)) and (cls.dtype is None or isinstance(obj, cls.ctype) or getattr(obj, "_type_", None) is cls.ctype):
            return a
        raise TypeError("expected %s, got %s" % (cls.__name__, type(a).__name__))


@functools.lru_cache(maxsize=None)
def _pointer(elem, const):
    """The argument class of `elem*`: elem a ctypes scalar, a numpy dtype (a table of structs) or None (void)."""
    if isinstance(elem, np.dtype):
        ctype, dtype, name = (), elem, "table"                # no ctypes object is a row of such a table
    else:
        ctype, dtype, name = elem, elem and np.dtype(elem), elem.__name__[2:] if elem else "void"
    return type(("const_" if const else "") + name + "_p", (_Pointer,), dict(ctype=ctype, dtype=dtype, const=const))


def _ctype(spelling, types):
    """One C type -> its ctypes type.  `types`: the binding module's struct mirrors by C name, C.Structure classes or numpy dtypes.  KeyError: unknown spelling."""
    const = spelling.startswith("const ")
    stars = spelling.count("*")
    base = " ".join(re.sub(r"\bconst\b|\*", " ", spelling).split())
    if base in _HANDLES and stars:
        t, stars = C.c_void_p, stars - 1
    elif base == "char" and const and stars:
        t, stars = C.c_char_p, stars - 1
    else:
        t = types[base] if base in types else _SCALARS[base]
    if stars == 1 and isinstance(t, type) and issubclass(t, C.Structure):
        return C.POINTER(t)
    if stars == 1 and t is not C.c_void_p and t is not C.c_char_p:
        return _pointer(t, const)
    for _ in range(stars):                                   # X** of a handle, const char**, const T* const*
        t = C.POINTER(t)
    return t


def signatures(header, types=None):
    """{name: (restype, [argtypes])} of every prototype in include/<header>, in the header's order."""
    types = types or {}
    with open(os.path.join(_INCLUDE, header)) as f:
        src = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    src = re.sub(r"^\s*#.*$", ";", src, flags=re.M)          # preprocessor lines end a statement
    out = {}
    for ret, name, params in _PROTOTYPE.findall(src):
        try:
            what = "return type"
            res = _ctype(ret.strip(), types)
            res = C.c_void_p if isinstance(res, type) and issubclass(res, _Pointer) else res
            args = []
            for what in ([] if params.strip() == "void" else params.split(",")):
                spelling, array = _PARAMETER.fullmatch(what.strip()).groups()
                args.append(_ctype(spelling.strip() + ("*" if array else ""), types))
        except (KeyError, AttributeError):
            raise TypeError("include/%s: %s: no ctypes type for '%s'" % (header, name, " ".join(what.split()))) from None
        out[name] = (res, args)
    return out


def declare(lib, sigs, allow_missing=False):
    """Set restype and argtypes of every function of `sigs` on `lib`.  A symbol the library lacks is an AttributeError unless `allow_missing`."""
    for name, (res, args) in sigs.items():
        if hasattr(lib, name) or not allow_missing:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib
