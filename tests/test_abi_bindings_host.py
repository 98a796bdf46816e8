"""CPU-only: the ctypes bindings and the ABI constants are derived from include/lpformer_hip.h (lpformer_amd/_lib.py
parse_header) -- the parser on synthetic header text, the real header as the loaded libraries carry it, and a few
prototypes written out by hand."""
import ctypes as C

import pytest

from lpformer_amd import _lib
from lpformer_amd._lib import LpfError, parse_header

i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p

SYNTHETIC = """
/* a block comment with a declaration: int lpf_fake(int x);
 * over two lines */
#ifndef SYNTHETIC_H
#define SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define LPF_PLAIN 16
#define LPF_NEGATIVE (-1)   /* a trailing comment */
#define LPF_UNSIGNED 1u
#define LPF_SHIFTED (1 << 30)
// int lpf_fake(int x);
int lpf_scalars(int a, int32_t b, int64_t c, uint32_t d, uint64_t e, float f, double g);
int lpf_pointers(void **out, const float **rows, int *count, char *name, const char *label, const int64_t *rowptr,
                 float *y, const void *blob, int8_t *types, void *stream);
int64_t lpf_three_lines(int64_t n,
                        const int32_t *col,   // int lpf_fake(int x);
                        void *stream);
int lpf_no_arguments(void);
const char *lpf_text(int code);
void lpf_nothing(void *p);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_types():
    protos, _ = parse_header(SYNTHETIC)
    assert set(protos) == {"lpf_scalars", "lpf_pointers", "lpf_three_lines", "lpf_no_arguments", "lpf_text",
                           "lpf_nothing"}                                     # and no lpf_fake
    assert protos["lpf_scalars"] == (C.c_int, [C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float,
                                               C.c_double])
    assert protos["lpf_pointers"] == (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int), C.c_char_p,
                                                C.c_char_p, vp, vp, vp, vp, vp])
    assert protos["lpf_three_lines"] == (C.c_int64, [i64, vp, vp])
    assert protos["lpf_no_arguments"] == (C.c_int, [])
    assert protos["lpf_text"] == (C.c_char_p, [C.c_int])
    assert protos["lpf_nothing"] == (None, [vp])


def test_parser_constants():
    _, consts = parse_header(SYNTHETIC)
    assert consts == {"LPF_PLAIN": 16, "LPF_NEGATIVE": -1, "LPF_UNSIGNED": 1, "LPF_SHIFTED": 1 << 30}
    assert all(type(v) is int for v in consts.values())


@pytest.mark.parametrize("text, culprit", [
    ("int lpf_a(int x);\nint lpf_odd(size_t n);", "lpf_odd"),                  # a parameter type outside the rules
    ("int lpf_a(int x);\nint lpf_odd(unsigned int n);", "lpf_odd"),
    ("int lpf_a(int x);\nint lpf_odd(float ***p);", "lpf_odd"),
    ("int lpf_a(int x);\nint lpf_odd();", "lpf_odd"),
    ("int lpf_a(int x);\nfloat lpf_odd(int x);", "lpf_odd"),                   # a return type outside the rules
    ("int lpf_a(int x);\nint64_t *lpf_odd(int x);", "lpf_odd"),
    ("int lpf_a(int x);\nstruct leftover { int y; };", "leftover"),            # text left over
    ("int lpf_a(int x);\nint lpf_odd(int (*callback)(int));", "lpf_odd"),      # a declaration the pattern cannot read
    ("int lpf_a(int x);\nint other_name(int x);", "other_name"),
    ("int lpf_a(int x);\nint lpf_unfinished(int x)", "lpf_unfinished"),
    ("int lpf_twice(int x);\nint lpf_twice(int64_t x);", "lpf_twice"),         # a name declared twice
    ("#define LPF_ODD 0x10", "LPF_ODD"),                                       # a value outside the rules
    ("#define LPF_ODD (1 << )", "LPF_ODD"),
    ("#define LPF_ODD (2", "LPF_ODD"),
    ("#define LPF_ODD sizeof(int)", "LPF_ODD"),
    ("#define LPF_ODD __import__('os')", "LPF_ODD"),
    ("#define LPF_ODD", "LPF_ODD"),
    ("#define LPF_ODD 1\n#define LPF_ODD 2", "LPF_ODD"),
])
def test_parser_refuses(text, culprit):
    with pytest.raises(LpfError, match=culprit):
        parse_header(text)


def test_missing_header_says_where(monkeypatch, tmp_path):
    missing = str(tmp_path / "include" / "lpformer_hip.h")
    monkeypatch.setattr(_lib, "HEADER_PATH", missing)
    with pytest.raises(LpfError, match="lpformer_hip.h") as e:
        _lib._read_header()
    assert missing in str(e.value)


def test_real_header_is_what_the_libraries_carry():
    with open(_lib.HEADER_PATH) as f:
        protos, consts = parse_header(f.read())
    assert protos == _lib.PROTOTYPES and consts == _lib.CONST
    assert set(_lib.HOST_PROTOTYPES) == set(_lib.HOST_NAMES) and not set(_lib.HIP_PROTOTYPES) & set(_lib.HOST_NAMES)
    assert set(_lib.HIP_PROTOTYPES) | set(_lib.HOST_PROTOTYPES) == set(protos)
    hip, host = _lib.hip(), _lib.host()          # loading works without a GPU (no compute calls here)
    for lib, table in ((hip, _lib.HIP_PROTOTYPES), (host, _lib.HOST_PROTOTYPES)):
        for name, argtypes in table.items():
            fn = getattr(lib, name)
            assert list(fn.argtypes) == argtypes == protos[name][1], name
            assert fn.restype is protos[name][0], name
    assert hip.lpf_abi_version() == host.lpf_host_abi_version() == _lib.ABI_VERSION == consts["LPF_ABI_VERSION"] == 16


def test_pinned_prototypes():
    P = _lib.PROTOTYPES
    assert P["lpf_ppr_push_workspace_bytes"] == (C.c_int64, [i64, i64, C.c_double, C.c_double])
    assert P["lpf_device_info"][1] == [C.POINTER(C.c_int)] * 3 + [C.c_char_p, C.c_int]
    assert P["lpf_ppr_push_cpu"][1][-3:] == [C.POINTER(vp), C.POINTER(vp), i32]
    assert _lib.HOST_PROTOTYPES["lpf_ppr_push_cpu"] is P["lpf_ppr_push_cpu"][1]
    assert P["lpf_host_free"][0] is None
    assert P["lpf_strerror"][0] is C.c_char_p
    assert P["lpf_select_plan_blocks"] == (C.c_int64, [i64])
    assert P["lpf_gemm_f32"][1] == [i64, i32, i32, vp, i64, vp, i64, vp, vp, i64, vp, i64, C.c_uint32, vp]


def test_pinned_constants():
    assert (_lib.ABI_VERSION, _lib.FLAG_RELU, _lib.ROWS_PERM_LB_WORDS, _lib.SELECT4_BLOCK) == (16, 1, 1025, 64)
    assert (_lib.SELECT_ERR_NODE_RANGE, _lib.SELECT_ERR_ITEM_CAP, _lib.SELECT_ERR_ENTRY_CAP) == (1, 2, 4)
    assert _lib.CONST["LPF_ERR_INVALID"] == -1 and _lib.CONST["LPF_NEGATIVE_MAX_DRAWS"] == 1 << 30
    assert _lib.CONST["LPF_SELECT_CTL_WORDS"] == 16 and _lib.CONST["LPF_SELECT4_CTL_WORDS"] == 32
