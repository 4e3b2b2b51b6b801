"""The C ABI is written twice - the declaration in include/roma_hip.h and the definition in the operator's source, which the
compiler holds to each other - and roma_amd/_lib.py reads its ctypes signatures from the header.  No GPU needed:
  * the table read from the header is tests/golden/abi_signatures.json, which tools/make_goldens.py abi_signatures wrote from the
    hand-kept table the parser replaced: an ABI change has to rewrite that file on purpose, next to ROMA_ABI_VERSION;
  * the parser reads only the narrow C subset of the header and raises on everything else;
  * the two ctypes structures have the layout a C compiler gives the header's structs (tests/abi_layout.c);
  * both libraries export every declared name."""
import ctypes
import glob
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_goldens import abi_classes  # noqa: E402
from roma_amd import _lib  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_signatures.json")))


def test_signatures_read_from_the_header_are_the_golden_table():
    assert len(GOLDEN) == 120
    got = abi_classes(_lib.SIGNATURES)
    assert sorted(got) == sorted(GOLDEN)
    for name in GOLDEN:
        assert got[name] == GOLDEN[name], name
    used = {c for row in GOLDEN.values() for c in [row["ret"]] + row["args"]}
    assert used <= {"int", "long", "float", "double", "longlong", "ulonglong", "cstr", "ptr"}, used


def test_parser_reads_the_subset_the_header_is_written_in():
    C = ctypes
    text = """
    /* a comment with a declaration inside: int no(int x); */
    #ifdef __cplusplus
    extern "C" {
    #endif
    typedef struct roma_model* roma_handle_t;
    enum { A = 0, B = 1 };
    typedef struct {
      int a, b;  // int nor(int y);
      const float *p, *q;
    } args_t;
    #define VERSION 6
    int three_lines(roma_handle_t h, const float* in, unsigned char* mask,
                    long n, unsigned long long seed, long long m,
                    const char* name, char* buf, const args_t* a, float f, double d, void* stream);
    long nothing(void);
    const char* text(void);
    #ifdef __cplusplus
    }
    #endif
    """
    vp = C.c_void_p
    assert _lib.parse_header(text) == {
        "three_lines": (C.c_int, [vp, vp, vp, C.c_long, C.c_ulonglong, C.c_longlong, C.c_char_p, C.c_char_p, vp, C.c_float,
                                  C.c_double, vp]),
        "nothing": (C.c_long, []),
        "text": (C.c_char_p, []),
    }


@pytest.mark.parametrize("decl", ["int f(short x);", "int f(int (*cb)(int));", "int f(float v[3]);", "short f(int x);",
                                  "int f(unsigned x);", "int f();", "int f(int);", "int f(int x) { return x; }", "int x;"])
def test_parser_never_guesses(decl):
    with pytest.raises(ImportError) as e:
        _lib.parse_header("int ok(int a);\n" + decl)
    assert decl.split(";")[0].split("{")[0].strip() in str(e.value)  # the message names the declaration


def _rocm_cc():
    for pat in ("/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang", "/opt/rocm*/llvm/bin/clang", "/opt/rocm*/lib/llvm/bin/clang"):
        for cc in sorted(glob.glob(pat)):
            if os.access(cc, os.X_OK):
                return cc
    return None


def test_ctypes_structures_have_the_layout_of_the_header(tmp_path):
    cc = _rocm_cc()
    if cc is None:
        pytest.skip("no C compiler (llvm/bin/clang) found under /opt/rocm")
    exe = str(tmp_path / "abi_layout")
    build = subprocess.run([cc, "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "abi_layout.c"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=30)
    assert out.returncode == 0, out.stderr
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out.stdout.splitlines()}
    want = {}
    for cname, st in (("roma_config_t", _lib.RomaConfig), ("roma_forward_args_t", _lib.RomaForwardArgs)):
        want[(cname, "sizeof")] = ctypes.sizeof(st)
        for field, _ in st._fields_:
            want[(cname, field)] = getattr(st, field).offset
    assert got == want


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_both_libraries_export_every_declared_name(fmt):
    lib = _lib.load(fmt)  # binds every name of SIGNATURES, AttributeError on a missing one
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
