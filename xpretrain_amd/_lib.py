"""ctypes binding of libxpretrain_hip.so, read from the C ABI's one description: include/xpretrain_hip.h.

Importing this module parses the header (``parse_header``) and publishes every ``Xp*`` structure as a ``ctypes.Structure`` class,
every ``#define`` / enum constant under its header name, and ``SIGNATURES``: name -> (restype, argtypes).  A new entry point is
header + implementation + ``hip_ops`` wrapper; nothing is written here.

How C types become ctypes:
  * scalars: int / int32_t -> c_int32, int64_t, uint8_t, uint32_t, size_t, float;
  * structure fields: every pointer is c_void_p, ``T name[n]`` is ``T * n``, a nested struct is its class, a field named with a
    Python keyword gets a trailing underscore (``XpReduceSeg.in_``);
  * parameters: a pointer to an ABI struct is ``POINTER(struct)`` -- except a struct of ``_DEVICE_TABLES``, whose arrays live in
    device memory and are passed as integer addresses -- and every other pointer is c_void_p;
  * a ``const char*`` return is c_char_p.
The reader is strict: text it does not consume, an unknown type, a duplicate name or a struct used before its definition raises
RuntimeError naming the text.  Padding and alignment are the compiler's to confirm (tests/test_abi.py).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C xpretrain_amd/csrc``.
Loading fails loudly if it is missing -- there is no fallback path.
"""
import ctypes as C
import keyword
import os
import re
import sys
from types import SimpleNamespace

# PyTorch must be imported BEFORE the library is dlopen'ed: torch bundles its own HIP runtime
# (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  Loaded first, it satisfies our DT_NEEDED by soname and
# the process has ONE runtime / one set of streams; loaded second, torch would bring a second runtime whose
# streams are not ordered with ours.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libxpretrain_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "xpretrain_hip.h")

i32, i64, f32, vp, sz = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_size_t

_SCALARS = {"int": i32, "int32_t": i32, "int64_t": i64, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32, "size_t": sz, "float": f32}
_DEVICE_TABLES = ("XpAdamTensor",)
_FRAME = ("#ifndef XPRETRAIN_HIP_H\n#define XPRETRAIN_HIP_H", "#include <stddef.h>", "#include <stdint.h>",
          '#ifdef __cplusplus\nextern "C" {\n#endif', "#ifdef __cplusplus\n}\n#endif", "#endif")
_SPACE = re.compile(r"\s*")
_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
_DEFINE = re.compile(rf"#define[ \t]+(\w+)[ \t]+({_INT})[ \t]*$", re.M)
_ENUM = re.compile(r"enum\s*(\w*)\s*\{([^{}]*)\}\s*;")
_ENUMERATOR = re.compile(rf"(\w+)\s*(?:=\s*({_INT}))?")
_STRUCT = re.compile(r"typedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"([^;(){}#]+)\(([^;(){}#]*)\)\s*;")
_DECLARATOR = re.compile(r"(\w+)\s*(?:\[\s*(\d+)\s*\])?")
_DECL = re.compile(r"(?:const\s+)?(\w+)\b((?:\s*\*(?:\s*const\b)?)*)\s*\b" + _DECLARATOR.pattern)     # base type, stars, name, [n]


def parse_header(text, origin="<header>"):
    """structs (name -> class, in order of definition), signatures (name -> (restype, argtypes)) and constants (name -> int) of a
    header in the dialect of include/xpretrain_hip.h; RuntimeError naming the text for anything else."""
    structs, signatures, constants = {}, {}, {}

    def fail(why, what):
        raise RuntimeError(f"{origin}: {why}: {' '.join(what.split())!r}")

    def define(table, name, value, what):
        if name in structs or name in signatures or name in constants:
            fail(f"duplicate name {name!r}", what)
        table[name] = value

    def declaration(text, what):
        d = _DECL.fullmatch(text.strip())
        return d.groups() if d else fail("cannot parse the declaration", what)

    def ctype(base, stars, what, param):
        t = _SCALARS.get(base) or structs.get(base)
        if t is None and not (stars and base in ("void", "char")):
            fail(f"unknown type {base!r} (a struct must be defined before it is used)", what)
        if not stars:
            return t
        return C.POINTER(t) if param and stars.count("*") == 1 and base in structs and base not in _DEVICE_TABLES else vp

    text, pos = re.sub(r"/\*.*?\*/", " ", text, flags=re.S), 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            return SimpleNamespace(structs=structs, signatures=signatures, constants=constants)
        frame = next((f for f in _FRAME if text.startswith(f, pos)), None)
        if frame:
            pos += len(frame)
            continue
        for kind in (_DEFINE, _ENUM, _STRUCT, _PROTO):
            m = kind.match(text, pos)
            if m:
                break
        else:
            fail("cannot parse", text[pos:].split("\n", 1)[0])
        pos = m.end()
        if kind is _DEFINE:
            define(constants, m[1], int(m[2], 0), m[0])
        elif kind is _ENUM:
            value = -1
            for item in m[2].split(","):
                e = _ENUMERATOR.fullmatch(item.strip()) or fail(f"cannot parse the enumerator {item.strip()!r}", m[0])
                value = int(e[2], 0) if e[2] else value + 1
                define(constants, e[1], value, m[0])
        elif kind is _STRUCT:
            *decls, rest = m[2].split(";")
            if rest.strip() or m[1] not in ("", m[3]):
                fail("cannot parse the struct", m[0])
            fields = []
            for decl in decls:
                first, *more = decl.split(",")
                base, stars, name, n = declaration(first, decl)
                if stars and more:
                    fail("one pointer field per declaration", decl)
                t = ctype(base, stars, decl, param=False)
                for name, n in [(name, n)] + [(_DECLARATOR.fullmatch(d.strip()) or fail("cannot parse the field", decl)).groups() for d in more]:
                    fields.append((name + "_" * keyword.iskeyword(name), t * int(n) if n else t))
            define(structs, m[3], type(m[3], (C.Structure,), {"_fields_": fields}), m[0])
        else:
            base, stars, name, n = declaration(m[1], m[0])
            args = []
            for p in ([] if m[2].strip() == "void" else m[2].split(",")):
                pbase, pstars, _, pn = declaration(p, m[0])
                if pn:
                    fail("array parameter", m[0])
                args.append(ctype(pbase, pstars, m[0], param=True))
            if n:
                fail("cannot parse the prototype", m[0])
            res = C.c_char_p if (base, stars.count("*")) == ("char", 1) else ctype(base, stars, m[0], param=False)
            define(signatures, name, (res, args), m[0])


if not os.path.isfile(HEADER_PATH):
    raise RuntimeError(f"{HEADER_PATH} not found: the binding is read from the C header, which lives beside the xpretrain_amd package "
                       "in the repository tree.  xpretrain_amd has no CPU / eager fallback.")
with open(HEADER_PATH) as _f:
    _abi = parse_header(_f.read(), HEADER_PATH)
SIGNATURES, _constants = _abi.signatures, _abi.constants
globals().update(_abi.structs)
globals().update(_constants)
# the unprefixed spellings the host side uses
globals().update({k[3:]: v for k, v in _constants.items()
                  if k.startswith(("XP_EPI_", "XP_ACT_", "XP_ATTN_PROXY", "XP_ATTN_CAUSAL", "XP_GEMM_FAMILY_", "XP_GEMM_EPI_"))})

# XpLayerDims.act (XP_ACT_*) by config.hidden_act, and the fc1 / dpre epilogue kinds of each
ACTS = {"quick_gelu": _constants["XP_ACT_QUICK_GELU"], "gelu": _constants["XP_ACT_GELU"]}
EPI_ACT_FWD = (_constants["XP_EPI_BIAS_GELU"], _constants["XP_EPI_BIAS_GELU_ERF"])
EPI_ACT_BWD = (_constants["XP_EPI_GELU_BWD"], _constants["XP_EPI_GELU_ERF_BWD"])


def _names(prefix):
    return {v: k[len(prefix):].lower() for k, v in _constants.items() if k.startswith(prefix)}


ATTN_KERNELS = tuple(_names("XP_ATTN_KERNEL_")[v] for v in range(len(_names("XP_ATTN_KERNEL_"))))
# kernels only an opt-in switch plans (xp_set_attn_bwd_wide)
ATTN_OPTIN_KERNELS = _names("XP_ATTN_OPTIN_")

_lib = None


def lib():
    """The loaded library (raises RuntimeError if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C xpretrain_amd/csrc`.  xpretrain_amd has no CPU / eager fallback.")
        l = C.CDLL(LIB_PATH)
        missing = [n for n in SIGNATURES if not hasattr(l, n)]
        if missing:
            raise RuntimeError(f"{LIB_PATH} is missing C-ABI symbols: {missing}")
        for n, (res, args) in SIGNATURES.items():
            fn = getattr(l, n)
            fn.restype, fn.argtypes = res, args
        if l.xp_abi_version() != _constants["XP_ABI_VERSION"]:
            raise RuntimeError(f"ABI version mismatch: library {l.xp_abi_version()} != header {_constants['XP_ABI_VERSION']}")
        _lib = l
    return _lib


# XPRETRAIN_DEBUG=flag[,flag...]: the debug / test facilities (csrc/common.cpp lists the library's flags).  Python side:
#   sync      synchronise and check the device after every library call (errors then surface at the call that caused them)
#   op_by_op  encoder layers as separate operator calls instead of one C-ABI call per pass (the fingerprinting / calibration tools)
#   no_comm   GradBucketReducer packs and tracks its buckets but skips the all-reduce calls (cost attribution on one GPU)
DEBUG = frozenset(f for f in os.environ.get("XPRETRAIN_DEBUG", "").split(",") if f)
DEBUG_SYNC = "sync" in DEBUG


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {lib().xp_last_error().decode()}")
    if DEBUG_SYNC:      # debugging aid: localise an asynchronous fault to the call that caused it
        sys.stderr.write(f"[xp] {what} ... "); sys.stderr.flush()
        torch.cuda.synchronize()
        sys.stderr.write("ok\n"); sys.stderr.flush()
