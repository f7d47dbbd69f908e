"""The kernel library's C ABI is declared once (csrc/kernels/cxn_api.h) and cxxnet_amd.native derives the
ctypes bindings from that text: the header names exactly the entry points the sources define, the
reader maps each type class as the hand-typed table it replaced did, rejects what it does not know, and
the build's export check names a symbol missing on either side.  Host-side only; no library is loaded."""
import ctypes
import glob
import os
import re

import pytest

from cxxnet_amd import build, native

VP, I, L, F, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_uint
OPERAND_FIELDS = ["ptr", "gstride", "nbytes", "ld", "rows", "kdim", "H", "W", "C", "Ho", "Wo", "KH", "KW",
                  "stride", "pad_h", "pad_w", "dil", "Cg"]


@pytest.fixture(scope="module")
def api():
    with open(native._HEADER) as f:
        return native._read_protos(f.read())


def test_header_names_every_definition_and_nothing_else(api):
    defined = []
    for src in glob.glob(os.path.join(os.path.dirname(native._HEADER), "*.hip")):
        with open(src) as f:
            defined += re.findall(r"^CXN_API\b[^\n(]*?\b(cxn_\w+)\s*\(", f.read(), re.M)
    assert len(defined) == len(set(defined)), sorted(n for n in set(defined) if defined.count(n) > 1)
    assert set(api) - set(defined) == set(), "declared, not defined"
    assert set(defined) - set(api) == set(), "defined, not declared"
    assert len(api) == len(defined) > 0
    assert api == native._API  # what kernels() binds is what the header says


def test_fixed_vectors_cover_every_type_class(api):
    op = ctypes.POINTER(native.CxnOperand)
    assert api["cxn_zero"] == ([VP, L, VP], I)
    assert api["cxn_rec_end"] == ([], VP)
    assert api["cxn_rec_free"] == ([VP], None)
    assert api["cxn_gemm_sgd_stream_calls"] == ([], L)
    args, res = api["cxn_dropout"]
    assert (args[3], args[5], res) == (U, F, I) and len(args) == 7
    assert api["cxn_gemm"][0][:3] == [op, op, I]
    assert api["cxn_conv_weight_flip_multi"] == ([VP, VP, VP, I, VP], I)


def test_operand_struct_layout():
    assert [n for n, _ in native.CxnOperand._fields_] == OPERAND_FIELDS
    assert [t for _, t in native.CxnOperand._fields_] == [VP, L, L] + [I] * 15
    # the same numbers as the static_asserts under the struct
    assert ctypes.sizeof(native.CxnOperand) == 88
    assert native.CxnOperand.ld.offset == 24
    assert native.CxnOperand.Cg.offset == 80
    with open(native._HEADER) as f:
        text = f.read()
    for cond in ("sizeof(CxnOperand) == 88", "offsetof(CxnOperand, ld) == 24", "offsetof(CxnOperand, Cg) == 80"):
        assert f"static_assert({cond}," in text


@pytest.mark.parametrize("text,name", [
    ("CXN_API int cxn_bad_double(const void *x, double scale, void *stream);", "cxn_bad_double"),
    ("CXN_API int cxn_bad_size(void *x, size_t n, void *stream);", "cxn_bad_size"),
    ("CXN_API int cxn_bad_unnamed(void *x, int, void *stream);", "cxn_bad_unnamed"),
    ("CXN_API int cxn_bad_unnamed_ptr(const void *, int n);", "cxn_bad_unnamed_ptr"),
    ("CXN_API int cxn_twice(int a);\nCXN_API int cxn_twice(int a);", "cxn_twice"),
    ("CXN_API int cxn_no_semicolon(int a)\nCXN_API int cxn_next(int b);", "cxn_no_semicolon"),
    ("CXN_API int cxn_ok(int a);\nint cxn_stray(int b);\nCXN_API int cxn_after(int c);", "cxn_stray"),
    ("CXN_API double cxn_bad_return(int a);", "cxn_bad_return"),
    ("CXN_API int cxn_bad_comment(int a, /* rows */ int b);", "cxn_bad_comment"),
])
def test_reader_rejects_what_it_does_not_know(text, name):
    with pytest.raises(ValueError, match=rf"\b{name}\b"):
        native._read_protos(text)


def test_struct_reader_rejects_what_it_does_not_know():
    with pytest.raises(ValueError, match="double"):
        native._read_struct("struct CxnOperand {\n  const void *ptr;\n  double scale;\n};")
    with pytest.raises(ValueError, match="ld, rows"):
        native._read_struct("struct CxnOperand {\n  int ld, rows;\n};")
    with pytest.raises(ValueError, match="found 0"):
        native._read_struct("CXN_API int cxn_zero(void *dst, long bytes, void *stream);")


def test_wrapped_prototype_and_every_scalar_parse():
    got = native._read_protos("// a comment between prototypes\n"
                              "CXN_API long cxn_wrapped(const float *const *ws,\n"
                              "                         uint32_t seed, unsigned more,\n"
                              "                         float p, long n, int k, const CxnOperand *a);\n"
                              "CXN_API void *cxn_handle();\n")
    assert got == {"cxn_wrapped": ([VP, U, U, F, L, I, ctypes.POINTER(native.CxnOperand)], L),
                   "cxn_handle": ([], VP)}


def test_export_check_names_both_sides():
    nm = ("0000000000715ed0 T cxn_zero\n"
          "0000000000715f00 T cxn_only_in_library\n"
          "0000000000759d40 B cxn_deterministic\n"              # data, no entry point
          "0000000000700000 T _Z14cxn_fill_bytesPvimP12ihipStream_t\n"
          "0000000000700100 W _ZN3cxr8rec_slotEv\n").splitlines()
    assert build._export_mismatch(nm, ["cxn_zero", "cxn_only_in_header"]) == (["cxn_only_in_header"],
                                                                               ["cxn_only_in_library"])
    readelf = ("    41: 0000000000715ed0    40 FUNC    GLOBAL DEFAULT    13 cxn_zero\n"
               "    42: 0000000000715f00    40 FUNC    GLOBAL DEFAULT    13 cxn_only_in_library\n"
               "    79: 0000000000759d40     4 OBJECT  GLOBAL DEFAULT    27 cxn_deterministic\n").splitlines()
    assert build._export_mismatch(readelf, ["cxn_zero", "cxn_only_in_header"]) == (["cxn_only_in_header"],
                                                                                    ["cxn_only_in_library"])
    assert build._export_mismatch(nm[:1], ["cxn_zero"]) == ([], [])
