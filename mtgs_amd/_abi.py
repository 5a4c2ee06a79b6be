"""include/mtgs_rast.h as the Python layer sees it: the header is the one description of the C ABI, and this module reads it.

    prototypes()        {name: (restype, [argtypes])} of every mtgs_* function the header declares (ctypes)
    signatures()        {name: (result letter, argument letters)}: the same, as tests/golden/abi_signatures.txt spells it
    struct_dtype(name)  numpy record dtype of `typedef struct name { ... } name;` with C's natural alignment
    constant(name)      value of a #define (an integer or a float) or of an enumerator of an anonymous enum
    included_headers()  the names on the #include "mtgs_*.h" lines of mtgs_rast.h, in order: one group of entry points each
    header_abi(name)    the whole Abi tuple (prototypes, signatures, structs, constants) of ONE named header that mtgs_rast.h includes

A few regular expressions over a header this project owns, not a C parser: anything they do not recognise raises with the line
number and the text of the declaration -- nothing is skipped or guessed.  If a new header line resists, write it in the plain form
the others have.  The header is read once; the three functions answer from the cached result.
"""
from __future__ import annotations

import ctypes as C
import re
from functools import lru_cache
from pathlib import Path
from typing import NamedTuple

import numpy as np

HEADER = Path(__file__).resolve().parent.parent / "include" / "mtgs_rast.h"

# by-value scalars: C type -> (ctypes type, numpy format, letter of tests/golden/abi_signatures.txt)
_SCALARS = {"int": (C.c_int, "<i4", "i"), "int32_t": (C.c_int, "<i4", "i"), "int64_t": (C.c_int64, "<i8", "l"),
            "float": (C.c_float, "<f4", "f"), "double": (C.c_double, "<f8", "d"), "size_t": (C.c_size_t, "<u8", "z"),
            "uint64_t": (C.c_uint64, "<u8", "Q"), "unsigned": (C.c_uint, "<u4", "I"), "uint32_t": (C.c_uint, "<u4", "I")}
_POINTEES = set(_SCALARS) | {"void", "char", "uint8_t"}   # + the structs declared so far; every pointer is c_void_p / <u8 / p

_TOP = re.compile(r"""\s*(?:
      (?P<linkage>\#\s*ifdef\s+__cplusplus\s+(?:extern\s+"C"\s*\{|\})\s+\#\s*endif\b)
    | (?P<pp>\#[^\n]*)
    | typedef\s+struct\s+(?P<struct>\w+)\s*\{(?P<members>[^{}]*)\}\s*(?P=struct)\s*;
    | enum\s*\{(?P<enum>[^{}]*)\}\s*;
    | (?P<decl>[^;{}\#]+);
    )""", re.X)
_DEFINE = re.compile(r"#\s*define\s+(\w+)(\(?)(.*)")
_IGNORED_PP = re.compile(r"#\s*(ifndef|ifdef|endif|include)\b")
_PROTOTYPE = re.compile(r"(?P<ret>[\w\s*]+?)\b(?P<name>mtgs_\w+)\s*\((?P<args>.*)\)", re.S)
_TYPE = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)")
_PARAMETER = re.compile(r"(?:const\s+)?(\w+)(?:\s*(\*)\s*|\s+)\w+")
_MEMBER = re.compile(r"(?:const\s+)?(\w+)\s+(.+)", re.S)
_DECLARATOR = re.compile(r"(\*?)\s*(\w+)\s*(?:\[([^\[\]]+)\])?")
_NAME = re.compile(r"(?<![\w.])[A-Za-z_]\w*")
_FLOAT = re.compile(r"(?:\d+\.\d*|\.\d+|\d+(?=e))(?:e[+-]?\d+)?")


class Abi(NamedTuple):
    prototypes: dict    # name -> (restype, [argtypes])
    signatures: dict    # name -> (letter of the result, letters of the arguments)
    structs: dict       # name -> np.dtype
    constants: dict     # name -> int or float


def parse(text: str) -> Abi:
    """The ABI a header `text` declares.  Raises ValueError naming the first line it does not recognise."""
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n") + " ", text, flags=re.S)   # line numbers survive
    abi = Abi({}, {}, {}, {})
    pos, end = 0, len(text.rstrip())

    def fail(what, where, at=None):       # `at`: offset of the offending text, the current declaration's by default
        at = pos if at is None else at
        line = text.count("\n", 0, len(text) - len(text[at:].lstrip())) + 1
        raise ValueError(f"header line {line}: {what}: {' '.join(where.split())!r}")

    def number(expr, at=None, integer=False):   # a constant expression over literals and the #defines / enumerators seen so far
        try:
            plain = _NAME.sub(lambda m: repr(abi.constants[m.group()]), re.sub(r"(?<=[\d.])f\b", "", expr))
        except KeyError as e:
            fail(f"unknown constant {e.args[0]}", expr, at)
        if re.fullmatch(r"[\d\s+*()-]+", plain):
            return int(eval(plain, {"__builtins__": {}}))
        if integer or not re.fullmatch(r"[\s+*/()-]*", _FLOAT.sub("", plain)):       # 0x10, 16u, 1 << 2, 7 / 2
            fail("not an integer constant expression" if integer else "neither an integer nor a float constant expression", expr, at)
        return float(eval(plain, {"__builtins__": {}}))

    def kind(base, star, where, at=None):   # (ctypes type, numpy format, letter)
        if star:
            if base not in _POINTEES and base not in abi.structs:
                fail(f"pointer to unknown type {base!r}", where, at)
            return C.c_void_p, "<u8", "p"
        if base not in _SCALARS:
            fail(f"unknown type {base!r}", where, at)
        return _SCALARS[base]

    while pos < end:
        m = _TOP.match(text, pos)
        if m is None:
            fail("unrecognised declaration", text[pos:].lstrip().split("\n")[0])
        if m["linkage"]:          # #ifdef __cplusplus / extern "C" { or } / #endif, as a whole: a brace anywhere else is an error
            pass
        elif m["pp"]:
            d = _DEFINE.fullmatch(m["pp"].strip())
            if d and d[2]:
                fail("function-like macro", m["pp"])
            if d and d[3].strip():                       # a #define without a value (the include guard) is no constant
                abi.constants[d[1]] = number(d[3])
            elif not d and not _IGNORED_PP.match(m["pp"]):
                fail("unrecognised preprocessor line", m["pp"])
        elif m["struct"]:
            fields = []
            for member in re.finditer(r"[^;]*[^;\s][^;]*", m["members"]):
                decl, at = member.group().strip(), m.start("members") + member.start()
                mm = _MEMBER.fullmatch(decl)
                parts = [_DECLARATOR.fullmatch(part.strip()) for part in mm[2].split(",")] if mm else [None]
                if None in parts:
                    fail(f"unrecognised member of {m['struct']}", decl, at)
                for dd in parts:
                    fmt = kind(mm[1], dd[1], decl, at)[1]
                    fields.append((dd[2], fmt) if dd[3] is None else (dd[2], fmt, (number(dd[3], at, integer=True),)))
            abi.structs[m["struct"]] = np.dtype(fields, align=True)
        elif m["enum"] is not None:
            for part in filter(None, (s.strip() for s in m["enum"].split(","))):
                e = re.fullmatch(r"(\w+)\s*=\s*(.+)", part)
                if e is None:
                    fail("enumerator without an explicit value", part)
                abi.constants[e[1]] = number(e[2], integer=True)
        else:
            p = _PROTOTYPE.fullmatch(m["decl"].strip())
            t = p and _TYPE.fullmatch(p["ret"].strip())
            if not t:
                fail("unrecognised declaration", m["decl"])
            result = (C.c_char_p, None, "s") if (t[1], t[2]) == ("char", "*") else kind(t[1], t[2], m["decl"])
            args = []
            for arg in ([] if p["args"].strip() == "void" else p["args"].split(",")):
                a = _PARAMETER.fullmatch(arg.strip())
                if a is None:
                    fail(f"unrecognised parameter {' '.join(arg.split())!r} of", m["decl"])
                args.append(kind(a[1], a[2], m["decl"]))
            abi.prototypes[p["name"]] = (result[0], [a[0] for a in args])
            abi.signatures[p["name"]] = (result[2], "".join(a[2] for a in args))
        pos = m.end()
    return abi


@lru_cache(maxsize=None)
def _header() -> Abi:
    return parse(HEADER.read_text())


@lru_cache(maxsize=None)
def included_headers() -> tuple:
    """The additive blocks that are headers of their own, in the order mtgs_rast.h includes them.  Each is read by the same
    parser (header_abi), bound by _lib.load() and keeps a reviewed record of its own, tests/golden/abi_signatures_<x>.txt."""
    return tuple(re.findall(r'^#\s*include\s+"(mtgs_\w+\.h)"', HEADER.read_text(), re.M))


@lru_cache(maxsize=None)
def header_abi(name: str) -> Abi:
    """What the included header include/`name` declares by itself: the same Abi tuple as for mtgs_rast.h, structs and constants
    included."""
    if name not in included_headers():
        raise ValueError(f"{HEADER.name} does not include {name!r}")
    return parse((HEADER.parent / name).read_text())


def prototypes() -> dict:
    return _header().prototypes


def signatures() -> dict:
    return _header().signatures


def struct_dtype(name: str) -> np.dtype:
    return _header().structs[name]


def constant(name: str):
    return _header().constants[name]
