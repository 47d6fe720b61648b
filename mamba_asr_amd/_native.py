"""ctypes binding of libconmamba_hip.so, derived from the C ABI's header include/conmamba_hip.h.

At import this module parses the header and creates from it every argument structure (``cm_foo_bar_args`` ->
``FooBarArgs``), the ``SYMBOLS`` table of prototypes, the ``CM_*`` constants and ``ABI_VERSION``: the header is the only
description of the boundary.  The parser takes the small subset of C the header's opening comment lists and raises
ValueError on anything else, so a declaration it only half understands never yields a layout.

The library is built in-tree (``mamba_asr_amd/lib/libconmamba_hip.so``) by
``__graft_entry__.build()`` / ``make -C mamba_asr_amd/csrc``.  There is no CPU fallback:
if the library is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import collections
import ctypes as C
import keyword
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CM_LIB_PATH") or os.path.join(_HERE, "lib", "libconmamba_hip.so")    # CM_LIB_PATH: A/B builds of the same ABI
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "conmamba_hip.h")

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_POINTEES = set(_SCALARS) | {"void", "char", "int8_t", "uint8_t", "int16_t", "uint16_t"}    # T * is a c_void_p for these and for structs
_RETURNS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "const char *": C.c_char_p}
_CLASS_NAMES = {"cm_layernorm_args": "LayerNormArgs"}      # the one name that is not the camel-cased C name

Header = collections.namedtuple("Header", "structs protos consts ablate_protos")


def class_name(c_name: str) -> str:
    """cm_scan_cl_dir -> ScanClDir."""
    stem = c_name[3:] if c_name.startswith("cm_") else c_name
    return _CLASS_NAMES.get(c_name) or "".join(p[:1].upper() + p[1:] for p in stem.split("_"))


def _bad(what: str, decl: str):
    return ValueError(f"conmamba_hip.h: {what}: `{' '.join(decl.split())}`")


def _integer(text: str, decl: str) -> int:
    t = text.strip()
    while t.startswith("(") and t.endswith(")"):
        t = t[1:-1].strip()
    m = re.fullmatch(r"([+-]?)\s*(0[xX][0-9a-fA-F]+|[1-9][0-9]*|0)[uUlL]*", t)
    if not m:
        raise _bad("not an integer constant", decl)
    return int(m.group(1) + m.group(2), 0)


def _preprocess(text: str):
    """Comments out, directives handled: (product declarations, CM_ABLATE-only declarations, #define constants)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out, consts, stack, guard, guard_open = {"keep": [], "ablate": []}, {}, [], None, False
    for line in text.split("\n"):
        s = line.strip()
        if not s.startswith("#"):
            mode = stack[-1] if stack else "keep"
            if mode != "skip":
                out[mode].append(line)
            continue
        if s.endswith("\\"):
            raise _bad("continued directive", s)
        d = s[1:].split(None, 2)
        op, name, rest = (d + ["", "", ""])[:3]
        if op in ("ifdef", "ifndef") and stack:
            raise _bad("nested conditional", s)
        if op == "ifndef" and guard is None and not rest and not "".join(out["keep"]).strip() and not consts:
            guard, guard_open = name, True                      # the include guard: #ifndef X / #define X ... #endif
        elif op == "ifdef" and not rest and name in ("__cplusplus", "CM_ABLATE"):
            stack.append("skip" if name == "__cplusplus" else "ablate")
        elif op == "endif" and stack:
            stack.pop()
        elif op == "endif" and guard_open:
            guard_open = False
        elif stack and stack[-1] == "skip":
            continue
        elif op == "include" and name in ("<stdint.h>", "<stddef.h>") and not rest:
            continue
        elif op == "define" and name == guard and not rest:
            continue
        elif op == "define" and re.fullmatch(r"[A-Za-z_]\w*", name) and rest:
            consts[name] = _integer(rest, s)
        else:
            raise _bad("unsupported directive", s)
    if stack or guard_open:
        raise _bad("unterminated conditional", "#ifdef" if stack else f"#ifndef {guard}")
    return "\n".join(out["keep"]), "\n".join(out["ablate"]), consts


def _fields(body: str, structs: dict, owner: str):
    fields = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        m = re.fullmatch(r"\s*(?:const\s+)?([A-Za-z_]\w*)\b\s*(.*?)\s*", decl, flags=re.S)
        if not m or ":" in decl or "(" in decl:       # bit-fields, function pointers
            raise _bad(f"unsupported field of {owner}", decl)
        base = m.group(1)
        for item in m.group(2).split(","):
            dm = re.fullmatch(r"\s*((?:\*\s*)*)([A-Za-z_]\w*)\s*(?:\[\s*([0-9]+)\s*\])?\s*", item)
            if not dm:
                raise _bad(f"unsupported declarator in {owner}", decl)
            if dm.group(1):
                if base not in _POINTEES and base not in structs:
                    raise _bad(f"unknown type `{base}` in {owner}", decl)
                ctype = C.c_void_p
            elif base in _SCALARS or base in structs:
                ctype = _SCALARS.get(base) or structs[base]
            else:
                raise _bad(f"unknown type `{base}` in {owner}", decl)
            if dm.group(3) is not None:
                if int(dm.group(3)) < 1:
                    raise _bad(f"empty array in {owner}", decl)
                ctype = ctype * int(dm.group(3))
            name = dm.group(2)
            fields.append((name + "_" if keyword.iskeyword(name) else name, ctype))      # the C field `in` is `in_` here
    return fields


def _prototype(decl: str, structs: dict):
    m = re.fullmatch(r"\s*(const\s+char\s*\*|[A-Za-z_]\w*)\s*([A-Za-z_]\w*)\s*\((.*)\)\s*", decl, flags=re.S)
    ret = " ".join(m.group(1).replace("*", " * ").split()) if m else None
    if ret not in _RETURNS:
        raise _bad("unsupported declaration", decl)
    args = []
    if m.group(3).strip() != "void":
        for item in m.group(3).split(","):
            am = re.fullmatch(r"\s*(?:const\s+)?([A-Za-z_]\w*)\b\s*((?:\*\s*)*)([A-Za-z_]\w*)?\s*", item)
            if not am:
                raise _bad("unsupported argument", decl)
            base, stars = am.group(1), am.group(2).replace(" ", "")
            if stars == "*" and base in structs:
                args.append(C.POINTER(structs[base]))
            elif stars and (base in _POINTEES or base in structs):
                args.append(C.c_void_p)
            elif not stars and base in _SCALARS:
                args.append(_SCALARS[base])
            else:
                raise _bad(f"unknown type `{base}`", decl)
    return m.group(2), (_RETURNS[ret], args)


def _declarations(text: str, structs: dict, protos: dict, consts: dict, prototypes_only: bool = False):
    pos = 0
    while text[pos:].strip():
        rest = text[pos:]
        end = rest.find(";")
        m = re.match(r"\s*typedef\s+(struct\s+([A-Za-z_]\w*)|enum)\s*\{", rest)
        if m and not prototypes_only:
            close = rest.find("}", m.end())
            end = rest.find(";", close) if close >= 0 else -1
            body, tail = rest[m.end():close], rest[close + 1:end].strip()
            if end < 0 or "{" in body or not re.fullmatch(r"[A-Za-z_]\w*", tail):       # nested / anonymous struct or union
                raise _bad("unsupported declaration", rest[:end + 1] if end >= 0 else rest)
            if m.group(2):
                if tail != m.group(2) or tail in structs:
                    raise _bad("struct tag and typedef name differ, or the struct is declared twice", rest[:m.end()] + " ... } " + tail)
                structs[tail] = type(class_name(tail), (C.Structure,),
                                     {"__slots__": (), "_fields_": _fields(body, structs, tail), "__module__": __name__})
            else:
                for item in body.split(","):
                    em = re.fullmatch(r"\s*([A-Za-z_]\w*)\s*=(.*)", item, flags=re.S)
                    if not em:
                        raise _bad(f"enumerator of {tail} without an explicit value", item)
                    consts[em.group(1)] = _integer(em.group(2), item)
        elif end < 0:
            raise _bad("unterminated declaration", rest)
        else:
            name, sig = _prototype(rest[:end], structs)
            if name in protos:
                raise _bad("declared twice", rest[:end])
            protos[name] = sig
        pos += end + 1


def parse_header(text: str) -> Header:
    """The structs (C name -> ctypes.Structure class with empty __slots__: a store to a name that is no field raises
    AttributeError), the prototypes (name -> (restype, argtypes)) and the integer constants (#define and enum) a header
    in the supported subset declares; ablate_protos holds the prototypes inside #ifdef CM_ABLATE, which the product
    library does not export.  Raises ValueError, quoting the declaration, on anything outside the subset."""
    keep, ablate, consts = _preprocess(text)
    structs, protos, ablate_protos = {}, {}, {}
    _declarations(keep, structs, protos, consts)
    _declarations(ablate, structs, ablate_protos, consts, prototypes_only=True)
    return Header(structs, protos, consts, ablate_protos)


with open(HEADER_PATH) as _f:
    HEADER = parse_header(_f.read())
globals().update({cls.__name__: cls for cls in HEADER.structs.values()})      # ScanFwdArgs, ScanClDir, ... FfnArgs
globals().update(HEADER.consts)                                               # CM_F32, CM_SCAN_CHUNK, CM_SEED_EPOCH_MUL, ...
ABI_VERSION = HEADER.consts["CM_ABI_VERSION"]
# every symbol include/conmamba_hip.h declares: (name, restype, argtypes)
SYMBOLS = [(name, res, args) for name, (res, args) in HEADER.protos.items()]

_lib = None


def lib():
    """dlopen the HIP library (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C mamba_asr_amd/csrc` (hipcc, --offload-arch=gfx950). There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(handle, name)      # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        got = handle.cm_abi_version()
        if got != ABI_VERSION:
            raise RuntimeError(f"libconmamba_hip ABI {got} != binding {ABI_VERSION}: rebuild the library")
        if hasattr(handle, "cm_debug_set"):  # the ablation build (make ablate; CM_LIB_PATH): timing-only kernel variants
            for name, (res, args) in HEADER.ablate_protos.items():
                fn = getattr(handle, name)
                fn.restype, fn.argtypes = res, args
            if os.environ.get("CM_DEBUG"):
                handle.cm_debug_set(int(os.environ["CM_DEBUG"]))
        _lib = handle
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().cm_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")
