"""(no GPU) The ctypes binding is read from include/esn_hip.h (esn_ofdm_mimo_amd/_lib.py): the parser on a synthetic
header with every form the real one uses, its refusal of a type it does not know, and on the real header the argument
counts, the pointer / scalar kind of every position, struct esn_shape, the ABI version and the enum constants -- each
counted here on its own, not through the parser."""
import ctypes as C
import os
import re

import pytest

from esn_ofdm_mimo_amd import _lib
from esn_ofdm_mimo_amd._lib import Shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "esn_hip.h")).read()
BARE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)                   # the real header has block comments only
SCALARS = (C.c_int, C.c_uint, C.c_double, C.c_uint64, C.c_size_t, C.c_longlong, C.c_ulonglong)
POINTERS = (C.c_void_p, C.c_char_p, C.POINTER(Shape), C.POINTER(C.c_int))

SYNTHETIC = r'''
#ifndef T_H
#define T_H
#define LONG_MACRO(a) \
    esn_not_a_function(a);
#ifdef __cplusplus
extern "C" {
#endif
enum esn_kind { ESN_A = 0, ESN_B = 1 };   // a line comment; with esn_ghost(int x);
typedef struct esn_shape { int n_res; double leak_rate; } esn_shape_t;
const char* esn_text(void);
/* a comment holding (parentheses), a semicolon; and int esn_hidden(int a); between declarations */
size_t esn_bytes(int precision, const esn_shape_t* shape);
int esn_many(int precision, const esn_shape_t* shape,
             const double* U, const float *V, uint8_t* bits, long long* count,
             double noise, uint64_t seed,
             size_t workspace_bytes, void* stream);
int esn_enum_arg(enum esn_kind kind, unsigned flags, unsigned long long big, long long n);
int esn_unnamed(int, double, const char*, void*);
void* esn_alloc(size_t bytes);
#ifdef __cplusplus
}
#endif
#endif
'''
PS, VP = C.POINTER(Shape), C.c_void_p


def test_parser_reads_every_form_the_header_uses():
    assert _lib.parse_signatures(SYNTHETIC) == {
        "esn_text": (C.c_char_p, []),
        "esn_bytes": (C.c_size_t, [C.c_int, PS]),
        "esn_many": (C.c_int, [C.c_int, PS, VP, VP, VP, VP, C.c_double, C.c_uint64, C.c_size_t, VP]),
        "esn_enum_arg": (C.c_int, [C.c_int, C.c_uint, C.c_ulonglong, C.c_longlong]),
        "esn_unnamed": (C.c_int, [C.c_int, C.c_double, C.c_char_p, VP]),
        "esn_alloc": (VP, [C.c_size_t]),
    }
    assert _lib.parse_enums(SYNTHETIC) == {"esn_kind": {"ESN_A": 0, "ESN_B": 1}}
    assert _lib.parse_enums("enum esn_e { ESN_X, ESN_Y = 4, ESN_Z };") == {"esn_e": {"ESN_X": 0, "ESN_Y": 4, "ESN_Z": 5}}
    assert _lib.parse_define(SYNTHETIC + "#define ESN_N 0x10  /* sixteen */\n", "ESN_N") == 16


@pytest.mark.parametrize("decl", ["int esn_odd(int n, float _Complex x);", "float esn_odd(int n);",
                                  "void esn_odd(int n);", "int esn_odd(int n, double 2x);", "int esn_odd(int a b);"])
def test_parser_refuses_a_type_it_does_not_know(decl):
    with pytest.raises(_lib.EsnHipError, match="esn_odd"):
        _lib.parse_signatures("int esn_fine(int n);\n" + decl)


def test_parser_refuses_a_declaration_it_cannot_read():
    with pytest.raises(_lib.EsnHipError, match="esn_callback"):
        _lib.parse_signatures("int esn_fine(int n);\nint esn_callback(int (*fn)(int), void* stream);")
    with pytest.raises(_lib.EsnHipError, match="ESN_NOPE"):
        _lib.parse_define(SYNTHETIC, "ESN_NOPE")


def declarations():
    """{name: [parameter text, ...]} of the real header, split on commas here."""
    found = re.findall(r"\b(esn_\w+)\s*\(([^()]*)\)\s*;", BARE)
    return {name: [] if args.strip() == "void" else args.split(",") for name, args in found}


def test_every_entry_has_the_argument_count_of_its_declaration():
    decls = declarations()
    assert sorted(decls) == sorted(_lib.SIGNATURES) and len(decls) >= 80
    for name, params in decls.items():
        assert len(_lib.SIGNATURES[name][1]) == len(params), name


def test_pointer_positions_are_pointer_ctypes_and_the_rest_scalars():
    for name, params in declarations().items():
        for i, (param, ctype) in enumerate(zip(params, _lib.SIGNATURES[name][1])):
            assert ctype in (POINTERS if "*" in param else SCALARS), (name, i, param, ctype)
        ret = re.search(r"([\w \t*]+?)\b%s\s*\(" % name, BARE).group(1)
        assert _lib.SIGNATURES[name][0] in (POINTERS if "*" in ret else SCALARS), (name, ret)
    # the two pointees that are not plain addresses, and the one override
    assert _lib.SIGNATURES["esn_last_error"] == (C.c_char_p, [])
    assert _lib.SIGNATURES["esn_debug_set"] == (C.c_int, [C.c_char_p, C.c_char_p])
    assert _lib.SIGNATURES["esn_tile_frames"] == (C.c_int, [C.c_int, PS])
    assert _lib.SIGNATURES["esn_device_alloc"] == (VP, [C.c_size_t])
    assert _lib.SIGNATURES["esn_device_info"] == (C.c_int, [C.POINTER(C.c_int)] * 3 + [C.c_char_p, C.c_int])
    assert [n for n, (_, a) in _lib.SIGNATURES.items() if C.POINTER(C.c_int) in a] == ["esn_device_info"]


def test_shape_fields_are_the_header_struct():
    body = re.search(r"typedef\s+struct\s+esn_shape\s*\{(.*?)\}\s*esn_shape_t\s*;", BARE, flags=re.S).group(1)
    members = [m.split() for m in body.split(";") if m.strip()]
    ctypes_of = {"int": C.c_int, "double": C.c_double}
    assert Shape._fields_ == [(name, ctypes_of[ctype]) for ctype, name in members]
    assert len(members) == 6 and C.sizeof(Shape) == 5 * 4 + 4 + 8      # five ints, padding, one double


def test_abi_version_is_stated_once():
    from esn_ofdm_mimo_amd import build
    build.build_library(verbose=False)
    assert re.findall(r"^#define ESN_ABI_VERSION (\d+)$", BARE, flags=re.M) == [str(_lib.ABI_VERSION)]
    assert _lib.load().esn_abi_version() == _lib.ABI_VERSION == 10


def header_enum(tag):
    body = re.search(r"enum\s+%s\s*\{(.*?)\}" % tag, BARE, flags=re.S).group(1)
    return {k: int(v) for k, v in re.findall(r"(\w+)\s*=\s*(\d+)", body)}


def test_enum_constants_are_the_header_values():
    prec, noise, mem = header_enum("esn_precision"), header_enum("esn_noise_mode"), header_enum("esn_mem_kind")
    assert (_lib.F64, _lib.F32, _lib.F16, _lib.BF16) == (prec["ESN_F64"], prec["ESN_F32"], prec["ESN_F16"],
                                                         prec["ESN_BF16"]) == (0, 1, 2, 3)
    assert _lib.PRECISIONS == {k[len("ESN_"):].lower(): v for k, v in prec.items()}
    assert (_lib.NOISE_NONE, _lib.NOISE_TENSOR, _lib.NOISE_COUNTER) == (
        noise["ESN_NOISE_NONE"], noise["ESN_NOISE_TENSOR"], noise["ESN_NOISE_COUNTER"]) and len(noise) == 3
    assert (_lib.MEM_DEVICE, _lib.MEM_HOST) == (mem["ESN_MEM_DEVICE"], mem["ESN_MEM_HOST"]) and len(mem) == 2
    paths = header_enum("esn_path")
    assert len(paths) == len(_lib.PATHS) == 8
    for name, value in paths.items():
        assert _lib.PATHS[value] == name[len("ESN_PATH_"):].lower(), name
