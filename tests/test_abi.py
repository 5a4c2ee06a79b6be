"""The C-ABI shared library: loads without a GPU, exports every symbol include/mtgs_rast.h declares,
and validates arguments on the host before any launch (no compute calls here)."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def header_symbols():
    text = (ROOT / "include" / "mtgs_rast.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mtgs_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_operator_table():
    syms = header_symbols()
    for must in ("mtgs_sh_fwd", "mtgs_sh_bwd", "mtgs_project_fwd", "mtgs_project_bwd", "mtgs_isect_count",
                 "mtgs_isect_scan", "mtgs_isect_emit", "mtgs_sort_pairs", "mtgs_isect_offsets", "mtgs_blend_fwd",
                 "mtgs_blend_bwd", "mtgs_tile_schedule", "mtgs_bin_compact", "mtgs_bin_emit", "mtgs_sort_pairs_u32", "mtgs_bin_sort_tiles", "mtgs_bin_build", "mtgs_dp_pack", "mtgs_dp_accumulate", "mtgs_dp_pack_ordered", "mtgs_node_fwd", "mtgs_node_bwd", "mtgs_node_fwd_batch", "mtgs_node_bwd_batch", "mtgs_densify_stats", "mtgs_densify_stats_batch", "mtgs_normals_fwd", "mtgs_normals_bwd", "mtgs_head_fwd", "mtgs_head_bwd", "mtgs_oob_fwd", "mtgs_oob_bwd", "mtgs_ncc_fwd", "mtgs_ncc_bwd", "mtgs_tv_fwd", "mtgs_tv_bwd", "mtgs_ssim_workspace_floats", "mtgs_ssim_fwd", "mtgs_ssim_bwd", "mtgs_l1_workspace_floats", "mtgs_l1_fwd", "mtgs_l1_bwd", "mtgs_dp_reduce", "mtgs_rast_version", "mtgs_rast_last_error"):
        assert must in syms


def header_define(name):
    """An integer #define of the header, by this file's own regex (not through mtgs_amd._abi)."""
    return int(re.search(r"^#define %s (\d+)\b" % name, (ROOT / "include" / "mtgs_rast.h").read_text(), re.M).group(1))


def test_library_exports_every_declared_symbol(hip_lib):
    from mtgs_amd import _lib
    syms = header_symbols()
    assert sorted(_lib.EXPORTS) == syms, "python binding table and header disagree"
    raw = C.CDLL(str(_lib.LIB_PATH))
    for s in syms:
        assert hasattr(raw, s), f"{s} not exported by libmtgs_rast.so"
    assert hip_lib.mtgs_rast_version() == _lib.ABI_VERSION == header_define("MTGS_RAST_ABI_VERSION")
    assert hip_lib.mtgs_rast_hot_version() == _lib.HOT_ABI_VERSION == header_define("MTGS_RAST_HOT_ABI_VERSION")


LETTERS = {"i": C.c_int, "l": C.c_int64, "f": C.c_float, "d": C.c_double, "z": C.c_size_t, "Q": C.c_uint64, "I": C.c_uint,
           "p": C.c_void_p, "s": C.c_char_p}


def test_prototypes_match_the_frozen_signatures():
    """The header reader renders to exactly the reviewed record tests/golden/abi_signatures.txt (first written from the
    hand-typed table the reader replaced): `name(arguments) result` per entry point, sorted, one letter per argument by the
    width and kind of its C type (i int32, l int64, f, d, z size_t, Q uint64, I uint32, p pointer; s the string result).
    And what ctypes is told, prototypes(), is those letters as ctypes types.  A new entry point adds its line to the file."""
    from mtgs_amd import _abi
    frozen = (ROOT / "tests" / "golden" / "abi_signatures.txt").read_text()
    signatures = _abi.signatures()
    assert "".join(f"{name}({args}) {res}\n" for name, (res, args) in sorted(signatures.items())) == frozen
    assert sorted(signatures) == header_symbols()
    assert _abi.prototypes() == {name: (LETTERS[res], [LETTERS[a] for a in args]) for name, (res, args) in signatures.items()}
    for name in ("mtgs_rast_version", "mtgs_rast_hot_version"):
        assert signatures[name] == ("i", "")
    assert signatures["mtgs_rast_last_error"] == ("s", "")


def included_headers():
    from mtgs_amd import _abi
    return _abi.included_headers()


@pytest.mark.parametrize("header", included_headers())
def test_an_included_header_is_declared_bound_and_exported(hip_lib, header):
    """Every header that mtgs_rast.h includes is a group of entry points of its own: read by mtgs_amd._abi.header_abi, bound by
    mtgs_amd._lib (GROUPS), exported by the library, with a reviewed record tests/golden/abi_signatures_<x>.txt in the spelling of
    abi_signatures.txt.  The groups are additive: the ABI versions stay 29 and 7."""
    from mtgs_amd import _abi, _lib
    abi = _abi.header_abi(header)
    frozen = (ROOT / "tests" / "golden" / f"abi_signatures_{header[len('mtgs_'):-len('.h')]}.txt").read_text()
    assert "".join(f"{name}({args}) {res}\n" for name, (res, args) in sorted(abi.signatures.items())) == frozen
    assert re.search(r'^#include "%s"' % re.escape(header), (ROOT / "include" / "mtgs_rast.h").read_text(), re.M)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mtgs_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(abi.signatures) == sorted(_lib.GROUPS[header]) and names
    raw = C.CDLL(str(_lib.LIB_PATH))
    for name, (restype, argtypes) in abi.prototypes.items():
        assert hasattr(raw, name), f"{name} not exported by libmtgs_rast.so"
        fn = getattr(hip_lib, name)
        assert fn.restype is C.c_int is restype and list(fn.argtypes) == argtypes
    assert abi.prototypes == {name: (LETTERS[res], [LETTERS[a] for a in args]) for name, (res, args) in abi.signatures.items()}
    assert _abi.constant("MTGS_RAST_ABI_VERSION") == 29 == header_define("MTGS_RAST_ABI_VERSION")
    assert _abi.constant("MTGS_RAST_HOT_ABI_VERSION") == 7 == header_define("MTGS_RAST_HOT_ABI_VERSION")
    assert hip_lib.mtgs_rast_version() == 29 and hip_lib.mtgs_rast_hot_version() == 7


def test_the_groups_are_the_headers_the_records_and_disjoint():
    """One table: the header files, the #include lines and the reviewed records name the same groups; no entry point belongs to two
    groups, the main header's own declarations included; a header that is not included is refused by name."""
    from mtgs_amd import _abi, _lib
    files = {p.name for p in (ROOT / "include").glob("mtgs_*.h")} - {"mtgs_rast.h"}
    records = {"mtgs_" + p.stem[len("abi_signatures_"):] + ".h" for p in (ROOT / "tests" / "golden").glob("abi_signatures_*.txt")}
    included = _abi.included_headers()
    assert files == set(included) == records and len(set(included)) == len(included)
    assert list(_lib.GROUPS) == ["mtgs_rast.h", *included] and _lib.GROUPS["mtgs_rast.h"] is _lib.EXPORTS
    assert sorted(_lib.EXPORTS) == sorted(_abi.signatures()) == header_symbols()
    groups = list(_lib.GROUPS.items())
    for i, (a, names_a) in enumerate(groups):
        assert len(set(names_a)) == len(names_a), a
        for b, names_b in groups[i + 1:]:
            assert not set(names_a) & set(names_b), (a, b)
    with pytest.raises(ValueError, match="does not include"):
        _abi.header_abi("mtgs_nothing.h")


@pytest.mark.parametrize("text, names", [
    ("int mtgs_ok(int n);\nint mtgs_bad(long n, void *stream);\n", r"line 2.*'long'.*mtgs_bad"),                # an unknown type
    ("typedef struct mtgs_s {\n    int64_t n;\n\n    int flag : 3;\n} mtgs_s;\n", r"line 4.*mtgs_s.*'int flag : 3'"),   # a bit-field
    ("/* c\n */\nint mtgs_bad(int n, void (*done)(int), void *stream);\n", r"line 3.*\(\*done\).*mtgs_bad"),      # a function pointer
    ("int mtgs_bad(const mtgs_unknown *table);\n", r"'mtgs_unknown'.*mtgs_bad"),
    ("typedef struct mtgs_s {\n    int n;\n    float x[MTGS_N];\n} mtgs_s;\n", r"line 3.*MTGS_N"),
    ("#define MTGS_N 2.0f\ntypedef struct mtgs_s { float x[MTGS_N]; } mtgs_s;\n", r"not an integer.*MTGS_N"),
    ("int mtgs_ok(void);\n#define MTGS_BITS 0x10\n", r"line 2.*'0x10'"),                                           # #define values
    ("#define MTGS_BITS (1 << 2)\n", r"'\(1 << 2\)'"),
    ("#define MTGS_N 16u\n", r"'16u'"),
    ("#define MTGS_A 7\n#define MTGS_HALF (MTGS_A / 2)\n", r"line 2.*'\(MTGS_A / 2\)'"),
    ("#define MTGS_B (MTGS_A + 1)\n", r"unknown constant MTGS_A"),
    ("int mtgs_f(void);\n}\n", r"line 2.*unrecognised.*'}'"),                                                                # a stray brace
    ("extern \"C\" {\nint mtgs_f(void);\n}\n", r"line 1.*unrecognised.*extern"),
    ("int mtgs_bad(int, void *stream);\n", r"parameter 'int' of.*mtgs_bad"),                                        # no name
    ("#define MTGS_F(x) (x)\n", r"MTGS_F"),
    ("int mtgs_a(void)\nint mtgs_b(void);\n", r"mtgs_a.*mtgs_b"),                                                # a lost semicolon
])
def test_header_reader_fails_loudly(text, names):
    """Anything the reader does not recognise raises and names the declaration; nothing is skipped or guessed."""
    from mtgs_amd import _abi
    with pytest.raises(ValueError, match=names):
        _abi.parse(text)


def test_header_reader_on_a_small_header():
    from mtgs_amd import _abi
    abi = _abi.parse("#ifndef H\n#define H\n#include <stdint.h>\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
                     "#define MTGS_N 3 /* three */\n#define MTGS_X 0.5f\n#define MTGS_Y (1.0f / 4.0f)\nenum { MTGS_A = 0, MTGS_B = MTGS_N + 1 };\n"
                     "typedef struct mtgs_s {\n    int n; /* pad follows */\n    const float *p, *q;\n    int64_t a[MTGS_N + 1], b;\n"
                     "    float x[3];\n} mtgs_s;\n"
                     "const char *mtgs_name(void);\nint mtgs_f(int64_t n, const mtgs_s *s, unsigned m, uint64_t seed,\n"
                     "           size_t bytes, double eps, float *out, uint32_t k, int32_t j);\n#ifdef __cplusplus\n}\n#endif\n#endif\n")
    assert abi.constants == {"MTGS_N": 3, "MTGS_X": 0.5, "MTGS_Y": 0.25, "MTGS_A": 0, "MTGS_B": 4}
    assert [type(abi.constants[k]) for k in ("MTGS_N", "MTGS_X", "MTGS_B")] == [int, float, int]
    assert abi.signatures == {"mtgs_name": ("s", ""), "mtgs_f": ("i", "lpIQzdpIi")}
    assert abi.prototypes == {"mtgs_name": (C.c_char_p, []),
                              "mtgs_f": (C.c_int, [C.c_int64, C.c_void_p, C.c_uint, C.c_uint64, C.c_size_t, C.c_double, C.c_void_p,
                                                   C.c_uint, C.c_int])}
    d = abi.structs["mtgs_s"]
    assert d.names == ("n", "p", "q", "a", "b", "x") and d.itemsize == 80
    assert [d.fields[k][1] for k in d.names] == [0, 8, 16, 24, 56, 64] and d["a"].shape == (4,) and d["x"].base == "<f4"


def test_host_side_argument_validation(hip_lib):
    """Bad arguments are rejected before anything is launched, with a message."""
    from mtgs_amd import _lib
    n = C.c_size_t(0)
    assert hip_lib.mtgs_sort_workspace_bytes(-1, C.byref(n)) == 1
    assert b"mtgs_sort_workspace_bytes" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_scan_workspace_bytes(1 << 20, C.byref(n)) == 0 and n.value >= 8 * (1 << 20) // 2048
    # SH degree 5 / K too small
    assert hip_lib.mtgs_sh_fwd(10, 16, 5, None, None, None, None, None) == 1
    assert hip_lib.mtgs_sh_fwd(10, 4, 3, None, None, None, None, None) == 1
    with pytest.raises(RuntimeError, match="degree"):
        _lib.call("mtgs_sh_fwd", 10, 4, 3, None, None, None, None, None)
    # null pointers
    assert hip_lib.mtgs_project_fwd(1, 10, None, None, None, None, None, 64, 64, 0.3, 0.01, 1e10, 0.0,
                                    None, None, None, None, None, None, None, 0, 0, 0, None, None) == 1
    # tile size other than 16 and unsupported channel counts are refused by name
    assert hip_lib.mtgs_blend_fwd(1, 10, 3, None, None, None, None, None, None, 0, 64, 64, 8, 8, 8, None, None, 0,
                                  None, None, None, None, None) == 4
    assert b"tile_size" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_blend_fwd(1, 10, 9, None, None, None, None, None, None, 0, 64, 64, 16, 4, 4, None, None, 0,
                                  None, None, None, None, None) == 4
    # empty problems are a no-op success
    assert hip_lib.mtgs_sh_fwd(0, 16, 3, None, None, None, None, None) == 0
    assert hip_lib.mtgs_sort_pairs(0, 46, None, None, None, None, None, 0, None) == 0


STRUCTS = {"mtgs_node_desc": 320, "mtgs_stats_desc": 48, "mtgs_oob_desc": 64, "mtgs_adam_group": 232, "mtgs_dp_group": 48,
           "mtgs_dp_chunks": 400}


def c_fields(name):
    """[(field, is an array)] of a struct of the header, in declaration order, by this file's own regexes."""
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mtgs_rast.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        for part in decl.split(","):
            out.append((re.sub(r"[^A-Za-z0-9_]", " ", re.sub(r"\[.*?\]", "", part)).split()[-1], "[" in part))
    return out


def test_descriptor_tables_match_the_c_structs(hip_lib):
    """The record layouts the Python layer fills (mtgs_amd.nodes._DESC, mtgs_amd.densify._STATS_DESC, ...) are the header's
    structs (include/mtgs_rast.h) and have the size the LOADED library reports; the layouts themselves are checked against the
    C compiler in test_header_is_plain_c_and_struct_sizes_match."""
    from mtgs_amd import _abi, densify, dist, loss, nodes, optim
    assert hip_lib.mtgs_node_desc_bytes() == nodes._DESC.itemsize == 320
    assert hip_lib.mtgs_stats_desc_bytes() == densify._STATS_DESC.itemsize == 48
    assert hip_lib.mtgs_oob_desc_bytes() == loss._OOB_DESC.itemsize == 64
    assert hip_lib.mtgs_adam_group_bytes() == optim._GROUP.itemsize == 232
    tables = {"mtgs_node_desc": nodes._DESC, "mtgs_stats_desc": densify._STATS_DESC, "mtgs_oob_desc": loss._OOB_DESC,
              "mtgs_adam_group": optim._GROUP, "mtgs_dp_group": dist._DP_GROUP, "mtgs_dp_chunks": dist._DP_CHUNKS}
    assert set(tables) == set(STRUCTS)
    for name, dtype in tables.items():
        assert dtype == _abi.struct_dtype(name) and dtype.itemsize == STRUCTS[name], name


def test_header_is_plain_c_and_struct_sizes_match(tmp_path):
    """include/mtgs_rast.h compiles as C99 (no C++-isms, no torch types), and the C compiler's layout of the six descriptor
    structs -- sizeof the struct; offsetof and sizeof of EVERY field, and of one element of every array field -- is the layout
    of the record dtypes the header reader derives (mtgs_amd._abi.struct_dtype) and the Python layer uploads byte for byte."""
    import shutil
    import subprocess
    from mtgs_amd import _abi
    if shutil.which("gcc") is None:
        pytest.skip("gcc not installed")
    prints = []
    for name in STRUCTS:
        prints.append(f'printf("{name} . %zu 0 0\\n", sizeof({name}));')
        for field, is_array in c_fields(name):
            member = f"(({name} *)0)->{field}"
            prints.append(f'printf("{name} {field} %zu %zu %zu\\n", sizeof({member}), offsetof({name}, {field}), '
                          f'sizeof({member + "[0]" if is_array else member}));')
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mtgs_rast.h"\nint main(void) {\n' + "\n".join(prints) + "\nreturn 0; }\n")
    exe = tmp_path / "h"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)])
    by_c = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        name, field, size, offset, element = line.split()
        by_c.setdefault(name, []).append((field, int(size), int(offset), int(element)))
    assert set(by_c) == set(STRUCTS)
    arrays = set()
    for name, rows in by_c.items():
        dtype = _abi.struct_dtype(name)
        assert rows[0] == (".", dtype.itemsize, 0, 0) and dtype.itemsize == STRUCTS[name], name
        assert [r[0] for r in rows[1:]] == list(dtype.names), name
        for field, size, offset, element in rows[1:]:
            sub, at = dtype.fields[field][:2]
            assert (sub.itemsize, at, sub.base.itemsize) == (size, offset, element), (name, field)
            assert sub.shape == (() if size == element else (size // element,)), (name, field)
            arrays |= {field} if sub.shape else set()
    assert arrays == {"begin", "rows", "cap", "limit"}
