"""The ctypes binding is derived from include/lidog_amd.h (lidog_amd/_lib.py:parse_header): the parser on small
headers, a dozen entries of the real header written out, and the loaded library's argtypes / restypes."""
import ctypes
from ctypes import POINTER, c_char_p, c_int, c_int64, c_uint32, c_void_p

import pytest

from lidog_amd import _lib
from lidog_amd._lib import parse_header

ABI = "#define LIDOG_ABI_VERSION 3\n"
i32, i64, p, f, d = ctypes.c_int32, c_int64, c_void_p, ctypes.c_float, ctypes.c_double


def test_comments_and_preprocessor_lines_are_not_parsed():
    args, res, abi = parse_header(
        "#include <stdint.h>\n" + ABI + "/* int lidog_in_block(int32_t a);\n * calls lidog_other(x) */\n"
        "// int lidog_in_line(int32_t a);\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
        "int lidog_real(int32_t a /* int lidog_inner(void); */, void *stream);  // lidog_tail(\n"
        "#ifdef __cplusplus\n}\n#endif\n")
    assert (args, res, abi) == ({"lidog_real": [i32, p]}, {"lidog_real": c_int}, 3)


def test_parameter_kinds():
    args, res, _ = parse_header(
        ABI + "int64_t lidog_spread(const float *x,\n        int64_t n,\n\n        double w, float e,\n"
        "    uint32_t fill, int flag,\n   void *stream\n);\n"
        "int32_t lidog_none(void);\nconst char *lidog_text(void);\n"
        "int lidog_ptrs(const float *const *p, void *const *q, void **out, const uint64_t *keys, uint16_t *h);\n")
    assert args == {"lidog_spread": [p, i64, d, f, c_uint32, c_int, p], "lidog_none": [], "lidog_text": [],
                    "lidog_ptrs": [p, p, POINTER(c_void_p), p, p]}
    assert res == {"lidog_spread": c_int64, "lidog_none": c_int, "lidog_text": c_char_p, "lidog_ptrs": c_int}


@pytest.mark.parametrize("body, words", [
    ("int lidog_a(const float *x, size_t n);", ["lidog_a", "`n`", "size_t"]),
    ("int lidog_a(size_t *n);", ["lidog_a", "`n`", "size_t"]),
    ("int lidog_a(float *x, int32_t);", ["lidog_a", "int32_t", "no name"]),
    ("int lidog_a(const float *, int32_t n);", ["lidog_a", "const float *", "no name"]),
    ("int lidog_a(int32_t n, int (*cb)(int32_t what, int64_t a), void *stream);", ["lidog_a", "`cb`", "function"]),
    ("int lidog_a(int32_t n);\nint lidog_b(void);\nint lidog_a(int32_t n);", ["lidog_a", "twice"]),
    ("size_t lidog_a(int32_t n);", ["lidog_a"]),
    ("int lidog_a(int32_t n)\nint lidog_b(void);", ["lidog_a"]),
    ("typedef int lidog_fn(int32_t n);", ["lidog_fn"]),
    ("struct lidog_s { int a; };", ["lidog_s"]),
    ("static inline int lidog_a(int32_t n) { return lidog_b(n); }", ["lidog_a"]),
    ("int lidog_a();", ["lidog_a"]),
])
def test_what_the_parser_cannot_read_raises(body, words):
    with pytest.raises(RuntimeError) as e:
        parse_header(ABI + "int lidog_ok(int32_t n);\n" + body + "\nint lidog_ok2(void);\n")
    for w in words:
        assert w in str(e.value), str(e.value)


def test_header_without_abi_macro_raises():
    for text in ("int lidog_ok(int32_t n);\n", "/* #define LIDOG_ABI_VERSION 3 */\nint lidog_ok(int32_t n);\n",
                 "#define LIDOG_ABI_VERSION\nint lidog_ok(int32_t n);\n"):
        with pytest.raises(RuntimeError, match="LIDOG_ABI_VERSION"):
            parse_header(text)


# written out by hand from include/lidog_amd.h: every scalar kind, both return widths
PINNED = {
    "lidog_adam_step": ([p, p, p, p, i64, f, f, f, f, f, i32, f, p], c_int),
    "lidog_ce_fwd": ([p, p, i64, i32, i64, i32, p, i32, d, d, p, p, p, p], c_int),
    "lidog_point_labels": ([p, i64, i32, i32, p, p, p, i64, i64, p, p, p, c_uint32, p, i32, i32, p, i32, i64, p, p, p,
                            p, p], c_int),
    "lidog_comm_init_rank": ([p, i32, i32, POINTER(c_void_p)], c_int),
    "lidog_trunk_in_bn_readers": ([p, i32, p, i32, p, i32, p, i32, p], c_int),
    "lidog_abi_version": ([], c_int),
    "lidog_hash_capacity": ([i64], c_int64),
    "lidog_sconv_wgrad_slots": ([i32, i32, i32], c_int),
    "lidog_raycast_ws": ([i64, i64], c_int64),
    "lidog_tta_vote": ([p, i64, i32, p, i64, i32, i32, p, p, p], c_int),
    "lidog_sconv_gemm": ([p, p, p, p, p, p, p, i32, i32, i32, p, p, i64, p], c_int),
    "lidog_mix_gather_aug": ([p, i64, p, i64, p, p, p, p, i32, i64, f, p, i32, p, i32, d, d, d, p, i32, p, p, p],
                             c_int),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_real_header_entry(name):
    args, res = PINNED[name]
    got = _lib.SIGNATURES[name]
    assert len(got) == len(args) and all(a is b for a, b in zip(got, args)), got
    assert _lib._RESTYPES[name] is res


def test_module_tables_are_one_parse_of_the_real_header():
    with open(_lib.HEADER_PATH) as fh:
        args, res, abi = parse_header(fh.read())
    assert abi == _lib.ABI_VERSION == 9 and isinstance(_lib.ABI_VERSION, int)
    assert "lidog_last_error" not in _lib.SIGNATURES and args.pop("lidog_last_error") == []
    assert args == _lib.SIGNATURES and res == _lib._RESTYPES and len(args) >= 178


def test_built_library_carries_the_derived_types():
    from lidog_amd import build
    build.build()
    lib = _lib.load()
    for name, args in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args and all(a is b for a, b in zip(fn.argtypes, args)), name
        assert fn.restype is _lib._RESTYPES[name], name
    assert lib.lidog_last_error.restype is c_char_p and list(lib.lidog_last_error.argtypes) == []
    assert lib.lidog_abi_version() == _lib.ABI_VERSION == 9
