"""ctypes binding of libroma_hip.so / libroma_hip_f16.so (C ABI declared in include/roma_hip.h).

The 16-bit storage format is a build-time property of the library (csrc/common.h): `load("bf16")` (the default) binds
libroma_hip.so, `load("f16")` binds libroma_hip_f16.so - the same sources compiled for IEEE binary16, the reference's
default amp_dtype.  Both export the same symbols; f32-only operators live in either.

The signatures are not restated here: `SIGNATURES` is read from include/roma_hip.h at import (`parse_header`), the
declarations that the compiler holds every definition in csrc/ to; `EXTENSIONS` likewise from the header of the registration
operators (include/roma_hip_registration.h) and `TSDF` from that of the volumetric ones (include/roma_hip_tsdf.h).

There is deliberately NO fallback: if the HIP library is missing or does not export a symbol
the import fails loudly (the product path never routes through the CPU oracle).
"""
from __future__ import annotations

import ctypes as C
import os
import re

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# ROMA_LIB_DIR: A/B runs of tools/ against another BUILD of the same two libraries (e.g. the previous commit's); the product
# default is the in-tree build next to this file.  There is still no fallback: a missing library raises.
_HERE = os.environ.get("ROMA_LIB_DIR", _PKG)
LIB_PATH = os.path.join(_HERE, "libroma_hip.so")
LIB_PATHS = {"bf16": LIB_PATH, "f16": os.path.join(_HERE, "libroma_hip_f16.so")}

ROMA_F32, ROMA_BF16, ROMA_F16, ROMA_MIXED = 0, 1, 2, 3
H16_CODE = {"bf16": ROMA_BF16, "f16": ROMA_F16}


class RomaConfig(C.Structure):
    _fields_ = [("coarse_h", C.c_int), ("coarse_w", C.c_int), ("upsample_h", C.c_int), ("upsample_w", C.c_int),
                ("symmetric", C.c_int), ("upsample_preds", C.c_int), ("attenuate_cert", C.c_int),
                ("precision", C.c_int), ("max_batch", C.c_int), ("device", C.c_int)]


class RomaForwardArgs(C.Structure):
    """roma_forward_args_t (include/roma_hip.h)"""
    _fields_ = [("upsample", C.c_int), ("symmetric", C.c_int), ("scale_factor", C.c_double),
                ("seed_flow", C.c_void_p), ("seed_cert", C.c_void_p), ("seed_h", C.c_int), ("seed_w", C.c_int),
                ("flow", C.c_void_p * 5), ("cert", C.c_void_p * 5), ("feat", C.c_void_p * 5)]


# C type -> ctypes.  `char*` / `const char*` are c_char_p and every other pointer c_void_p (_ctype); nothing else is known.
_CTYPES = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong,
           "unsigned long long": C.c_ulonglong, "roma_handle_t": C.c_void_p}


def _ctype(text, named, decl):
    """One return type (named = False) or one parameter with its name of the declaration `decl` as a ctypes type."""
    words = re.findall(r"\w+|\*", text) if re.fullmatch(r"[\w\s*]+", text) else []  # no function pointer, no array
    if "*" in words:
        return C.c_char_p if [w for w in words[:words.index("*")] if w != "const"] == ["char"] else C.c_void_p
    key = " ".join(w for w in (words[:-1] if named else words) if w != "const")
    if key not in _CTYPES:
        raise ImportError(f"roma_hip.h: no ctypes type for `{' '.join(text.split())}` in `{decl}`")
    return _CTYPES[key]


def parse_header(text):
    """symbol -> (restype, argtypes) of every function that the C header `text` declares.  It reads the narrow subset of C
    that include/roma_hip.h is written in and raises on anything else: it never guesses a type."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r"\b(typedef\s+struct|enum)\s*\{[^}]*\}[^;]*;|\btypedef\b[^;{]*;", " ", text)
    text = re.sub(r'extern\s+"C"\s*\{|\}', " ", text)
    sigs = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"([\w\s*]+?)\s*\b(\w+)\s*\((.*)\)", decl)
        if not m:
            raise ImportError(f"roma_hip.h: `{decl}` is not a function declaration")
        ret, name, params = m.groups()
        sigs[name] = (_ctype(ret, False, decl), [_ctype(p, True, decl) for p in params.split(",") if params.strip() != "void"])
    return sigs


# symbol -> (restype, argtypes), read from the one declaration of the C ABI.  The header travels with the package (it is looked
# up next to it, whatever ROMA_LIB_DIR says); without it there is no binding.
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "roma_hip.h")
if not os.path.exists(HEADER_PATH):
    raise ImportError(f"{HEADER_PATH} not found - roma_amd reads the signatures of the C ABI from it")
with open(HEADER_PATH) as _f:
    SIGNATURES = parse_header(_f.read())
# the operator families declared in headers of their own (include/roma_hip_registration.h): a second table, bound by load()
# like the first.  SIGNATURES stays the table of roma_hip.h alone, the one ROMA_ABI_VERSION counts.
EXTENSION_HEADERS = [os.path.join(os.path.dirname(_PKG), "include", "roma_hip_registration.h")]
EXTENSIONS = {}
for _path in EXTENSION_HEADERS:
    if not os.path.exists(_path):
        raise ImportError(f"{_path} not found - roma_amd reads the signatures of the C ABI from it")
    with open(_path) as _f:
        _sigs = parse_header(_f.read())
    _twice = sorted(set(_sigs) & (set(SIGNATURES) | set(EXTENSIONS)))
    if _twice:
        raise ImportError(f"{_path} declares {_twice} a second time")
    EXTENSIONS.update(_sigs)
# the volumetric operators (include/roma_hip_tsdf.h): a third table.  EXTENSIONS stays the registration one, entry by entry.
TSDF_HEADER = os.path.join(os.path.dirname(_PKG), "include", "roma_hip_tsdf.h")
if not os.path.exists(TSDF_HEADER):
    raise ImportError(f"{TSDF_HEADER} not found - roma_amd reads the signatures of the C ABI from it")
with open(TSDF_HEADER) as _f:
    TSDF = parse_header(_f.read())
_twice = sorted(set(TSDF) & (set(SIGNATURES) | set(EXTENSIONS)))
if _twice:
    raise ImportError(f"{TSDF_HEADER} declares {_twice} a second time")

_libs = {}


class RomaHipError(RuntimeError):
    pass


def load(fmt: str = "bf16"):
    """dlopen the library that stores `fmt` ("bf16" | "f16") and bind every declared symbol (raises if anything is missing)."""
    if fmt in _libs:
        return _libs[fmt]
    path = LIB_PATHS[fmt]
    if not os.path.exists(path):
        raise ImportError(f"{path} not found - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(roma_amd has no CPU fallback)")
    lib = C.CDLL(path)
    for name, (res, args) in {**SIGNATURES, **EXTENSIONS, **TSDF}.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.roma_h16_format() != H16_CODE[fmt]:
        raise ImportError(f"{path} does not store {fmt} (roma_h16_format() = {lib.roma_h16_format()})")
    lib.h16 = fmt
    _libs[fmt] = lib
    return lib


def fmt_of(dtype) -> str:
    """library format for a torch dtype: float16 -> "f16", everything else (bfloat16, float32) -> "bf16"."""
    return "f16" if str(dtype) == "torch.float16" else "bf16"


def last_error(lib=None) -> str:
    return (lib or load()).roma_last_error().decode("utf-8", "replace")


def check(rc: int, exc=RomaHipError, lib=None):
    if rc != 0:
        raise exc(last_error(lib))
    return rc


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _device_tensor(x, name, module):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RomaHipError(f"roma_amd.{module}: {name} must be a tensor on a HIP device; there is no CPU fallback")
    return x.detach()
