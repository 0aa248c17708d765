"""CPU: the binding read from include/xpretrain_hip.h has the compiler's layouts and values, the library exports exactly what the
header declares, and the reader refuses a header it does not understand."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")      # hipcc's own clang and llvm-nm


def _built():
    from xpretrain_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_layouts_and_constants_are_the_compilers(tmp_path):
    """sizeof of every struct, offsetof and size of every field and the value of every constant, as the binding has them, asserted
    by a C compiler over the header itself: what a text reader cannot derive (padding, alignment)"""
    from xpretrain_amd import _lib
    abi = _lib.parse_header(open(_lib.HEADER_PATH).read())
    assert len(abi.structs) >= 16 and len(abi.constants) >= 62 and all(getattr(_lib, n) == v for n, v in abi.constants.items())
    lines = ["#include <stddef.h>", '#include "xpretrain_hip.h"']
    for name in abi.structs:
        cls = getattr(_lib, name)                   # the classes the package uses, not this test's second reading
        lines.append(f'_Static_assert(sizeof({name}) == {C.sizeof(cls)}, "sizeof {name}");')
        for field, _ in cls._fields_:
            f, c = getattr(cls, field), field.rstrip("_")
            lines.append(f'_Static_assert(offsetof({name}, {c}) == {f.offset} && sizeof((({name}*)0)->{c}) == {f.size}, "{name}.{c}");')
    lines += [f'_Static_assert({n} == {v}, "{n}");' for n, v in abi.constants.items()]
    assert len(lines) > 16 + 300 + 62
    src = tmp_path / "abi_layout.c"
    src.write_text("\n".join(lines) + "\n")
    cc = next((c for c in (os.path.join(LLVM_BIN, "clang"), shutil.which("cc")) if c and os.path.exists(c)), None)
    assert cc, "no C compiler: neither the clang beside hipcc nor cc"
    r = subprocess.run([cc, "-fsyntax-only", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_library_exports_every_declared_symbol():
    _lib = _built()
    lib = _lib.lib()          # raises if any symbol is missing
    assert lib.xp_abi_version() == _lib.XP_ABI_VERSION == 1
    assert lib.xp_last_error() is not None


def test_every_exported_symbol_is_declared():
    """the reverse direction: an extern "C" function that no header line declares is an ABI nobody reviews"""
    _lib = _built()
    nm = next((n for n in (os.path.join(LLVM_BIN, "llvm-nm"), shutil.which("llvm-nm"), shutil.which("nm")) if n and os.path.exists(n)), None)
    assert nm, "no llvm-nm beside hipcc"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("xp_")}
    assert exported == set(_lib.SIGNATURES), sorted(exported ^ set(_lib.SIGNATURES))


@pytest.mark.parametrize("text, names", [
    ("int xp_f(const double* x);", "unknown type 'double'"),
    ("int xp_f(void);\n} trailing", "cannot parse: '} trailing'"),
    ("int xp_f(void);\nint64_t xp_f(int32_t a);", "duplicate name 'xp_f'"),
    ("int xp_f(const XpLate* p);\ntypedef struct { int32_t a; } XpLate;", "unknown type 'XpLate' (a struct must be defined before it is used)"),
], ids=["unknown type", "trailing text", "duplicate prototype", "struct used before its definition"])
def test_the_reader_refuses_what_it_does_not_understand(text, names):
    from xpretrain_amd import _lib
    ok = _lib.parse_header("#define XP_N 3\nenum { XP_A, XP_B = 5, XP_C };\ntypedef struct { const float* in; int32_t n[2], m; } XpS;\n"
                           "size_t xp_g(const XpS* s, const void* const* t);\n")
    assert ok.constants == {"XP_N": 3, "XP_A": 0, "XP_B": 5, "XP_C": 6} and [f for f, _ in ok.structs["XpS"]._fields_] == ["in_", "n", "m"]
    assert ok.signatures == {"xp_g": (C.c_size_t, [C.POINTER(ok.structs["XpS"]), C.c_void_p])}
    with pytest.raises(RuntimeError, match=re.escape(names)):
        _lib.parse_header(text)


def test_cpu_tensors_are_rejected():
    import torch
    from xpretrain_amd import hip_ops as H
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.gemm(torch.zeros(8, 8), torch.zeros(8, 8), 8, 8, 8)
