"""The ctypes signatures of the native entry points are derived from their C definitions
(``ops/build.py`` api_signatures): the parser on synthetic sources, the whole tree, the host
library as loaded, and the textual check that every entry point the package calls is in the table."""
import ctypes
import glob
import os
import re
import subprocess

import pytest

from flink_ml_amd.ops import build as b
from flink_ml_amd.ops import native

PKG = os.path.dirname(os.path.dirname(os.path.abspath(b.__file__)))

SYNTHETIC = """
#define OTHER extern "C"
namespace { int helper(int a, float b) { return a; } }
// FMLX_API int commented_out(int a);
/* a comment with ( and ) and , in it: FMLX_API void also_commented(void); */
FMLX_API int
fmlx_four_lines(int dtype, const void* X,
                long ld,   // stride (in elements), not (bytes)
                void* stream) {
  return helper(dtype, 0.f);
}
FMLX_API void fmlx_restrict(const long* __restrict__ p, /* (n, m) */ unsigned long long n, uint32_t m, float f) { }
FMLX_API int64_t fmlx_empty() { return 0; }
FMLX_API void* fmlx_void(void) { return nullptr; }
extern "C" int unmarked(double d) { return (int)d; }
int64_t also_unmarked(int64_t v) { const char* s = "FMLX_API int in_a_string(int a)"; return v + s[0]; }
FMLX_API double fmlx_mixed(int32_t a, unsigned b, unsigned int c, int64_t d, long long e, uint64_t f, size_t g,
                           unsigned long h, double i, const double* const* j, void** k, const char* l, int) { return i; }
"""


def test_parser_on_synthetic_source():
    assert b.parse_api(SYNTHETIC, "synthetic.hip") == {
        "fmlx_four_lines": ("c_int", ["c_int", "c_void_p", "c_int64", "c_void_p"]),
        "fmlx_restrict": (None, ["c_void_p", "c_uint64", "c_uint", "c_float"]),
        "fmlx_empty": ("c_int64", []),
        "fmlx_void": ("c_void_p", []),
        "fmlx_mixed": ("c_double", ["c_int", "c_uint", "c_uint", "c_int64", "c_int64", "c_uint64", "c_uint64",
                                    "c_uint64", "c_double", "c_void_p", "c_void_p", "c_void_p", "c_int"]),
    }


@pytest.mark.parametrize("src", [
    "struct Cfg { int a; };\nFMLX_API int fmlx_bad(int a, Cfg cfg) { return a; }",  # struct by value
    "FMLX_API int fmlx_bad(int a, struct Cfg cfg);",
    "FMLX_API int fmlx_bad(long double x);",
    "FMLX_API int fmlx_bad(short x);",
    "FMLX_API int fmlx_bad(int& x);",
    "FMLX_API int fmlx_bad(int x[4]);",
    "FMLX_API int fmlx_bad(int (*cb)(int));",
    "FMLX_API int fmlx_bad(int a, ...);",
    "FMLX_API Cfg fmlx_bad(int a);",
    "FMLX_API bool fmlx_bad(void);",
])
def test_parser_refuses_types_outside_the_table(src):
    with pytest.raises(ValueError, match=r"fmlx_bad in bad\.cpp"):
        b.parse_api(src, "bad.cpp")


def test_parser_refuses_a_marker_without_a_function_and_duplicates():
    with pytest.raises(ValueError, match=r"odd\.cpp"):
        b.parse_api("FMLX_API int fmlx_value = 3;", "odd.cpp")
    with pytest.raises(ValueError, match=r"fmlx_twice in dup\.cpp.*twice"):
        b.parse_api("FMLX_API int fmlx_twice(int a);\nFMLX_API int fmlx_twice(int a) { return a; }", "dup.cpp")


def _marker_count(paths):
    # textual, independent of the parser: comments are the only other place the marker may stand
    n = 0
    for p in paths:
        text = re.sub(r"//[^\n]*|/\*.*?\*/", " ", open(p).read(), flags=re.S)
        n += len(re.findall(r"\bFMLX_API\b", text))
    return n


@pytest.mark.parametrize("which", ["kernels", "host"])
def test_whole_tree(which):
    srcs, _ = b.kernel_sources() if which == "kernels" else b.host_sources()
    api = b.api_signatures(which)  # raises on a duplicate name and on a type outside the table
    assert len(api) == _marker_count(srcs) > 30
    per_file = [b.parse_api(open(p).read(), os.path.basename(p)) for p in srcs]
    assert sum(len(a) for a in per_file) == len(api)  # no name in two files
    assert all(name.startswith("fmlx_") for name in api)
    known = set(b.C_TYPES.values()) | {"c_void_p"}
    for name, (restype, argtypes) in api.items():
        assert set(argtypes) <= known and (restype is None or restype in known), name


def test_host_markers_replace_the_extern_blocks():
    for p in b.host_sources()[0]:
        assert 'extern "C"' not in open(p).read(), p


def test_host_library_carries_the_derived_signatures():
    lib = native.host()
    api = b.api_signatures("host")
    for name, (restype, argtypes) in api.items():
        fn = getattr(lib, name)  # resolves: AttributeError otherwise
        assert list(fn.argtypes) == [getattr(ctypes, a) for a in argtypes], name
        assert fn.restype is (getattr(ctypes, restype) if restype else None), name
    assert api["fmlx_dc_open"] == ("c_void_p", ["c_void_p", "c_int64", "c_int64"])
    assert api["fmlx_gk_query"][0] is None and api["fmlx_dc_append"][0] == "c_int64"


def test_kernel_library_exports_the_derived_entry_points():
    """No GPU needed to read the built library's dynamic symbols: an entry point that only some
    preprocessor branch defines would be in the table and not in the library."""
    b.build_kernels()
    p = subprocess.run(["nm", "-D", "--defined-only", b.KERNEL_LIB], stdout=subprocess.PIPE, text=True, check=True)
    exported = {line.split()[-1] for line in p.stdout.splitlines() if line.strip()}
    api = set(b.api_signatures("kernels"))
    assert api <= exported, sorted(api - exported)
    assert {s for s in exported if s.startswith("fmlx_")} <= api  # nothing exported that is not marked


def _called(pattern):
    names = set()
    for p in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True):
        names.update(re.findall(pattern, open(p).read()))
    return names


def test_every_entry_point_the_package_calls_is_in_a_table():
    host, kernels = b.api_signatures("host"), b.api_signatures("kernels")
    on_host = _called(r"native\.host\(\)\s*\.\s*(fmlx_\w+)")
    on_kernels = _called(r"native\.kernels\(\)\s*\.\s*(fmlx_\w+)") | _called(r"native\.call\(\s*\"(fmlx_\w+)\"")
    assert len(on_host) > 10 and len(on_kernels) > 50
    assert on_host <= set(host), sorted(on_host - set(host))
    assert on_kernels <= set(kernels), sorted(on_kernels - set(kernels))
    # calls through a local handle (lib.fmlx_x(...), self.lib.fmlx_x(...), getattr(lib, "fmlx_x"))
    anywhere = _called(r"\.\s*(fmlx_\w+)\s*\(") | _called(r"[\"'](fmlx_\w+)[\"']")
    unknown = anywhere - set(host) - set(kernels)
    assert not unknown, sorted(unknown)


def test_load_takes_the_table_from_the_manifest_and_parses_only_without_one(monkeypatch):
    b.build_host()
    parsed = []
    monkeypatch.setattr(b, "api_signatures", lambda which: parsed.append(which) or {})
    monkeypatch.setattr(native, "_HLIB", None)
    native.host()
    assert parsed == []  # the manifest record check_fresh accepted carries the table
    monkeypatch.setattr(b, "check_fresh", lambda which: None)  # a library built by hand: no record
    monkeypatch.setattr(native, "_HLIB", None)
    native.host()
    assert parsed == ["host"]
