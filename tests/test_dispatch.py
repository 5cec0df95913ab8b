"""The host visitors of ``csrc/dispatch.h`` (run-time dtype / width / flag → template arguments),
checked on the CPU: a stand-alone program built by hipcc for the host only, launching nothing."""
import os
import subprocess

from flink_ml_amd.ops import build as b

PROGRAM = r"""
#include "common.h"
#include <cstdio>
#include <type_traits>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

template <typename X, typename Y> constexpr bool same = std::is_same<X, Y>::value;

int main() {
  int calls = 0;
  // with_dtype: one call with the matching <T, A>, f's own return (negative too) passed through
  auto size_of = [&](auto t) { ++calls; return (int)sizeof(typename decltype(t)::T) * 10 + (int)sizeof(typename decltype(t)::A); };
  CHECK((with_dtype<float, double, bf16_t, int>(DT_F32, size_of) == 44) && calls == 1);
  CHECK((with_dtype<float, double, bf16_t, int>(DT_F64, size_of) == 88) && calls == 2);
  CHECK((with_dtype<float, double, bf16_t, int>(DT_BF16, size_of) == 24) && calls == 3);
  CHECK((with_dtype<float, double, bf16_t, int>(DT_I32, size_of) == 44) && calls == 4);
  CHECK((with_dtype<double, float>(DT_F32, [&](auto t) {
    ++calls;
    return same<typename decltype(t)::T, float> && same<typename decltype(t)::A, float> ? -7 : 0;
  }) == -7) && calls == 5);
  // a code outside the list: nothing called, miss returned (default -1)
  CHECK((with_dtype<float, double>(DT_BF16, size_of) == -1) && calls == 5);
  CHECK((with_dtype<float, double>(DT_I64, size_of, -4) == -4) && calls == 5);
  CHECK((with_dtype<float, double>(-3, size_of) == -1) && calls == 5);

  // with_acc: a value of the accumulator type
  calls = 0;
  CHECK(with_acc(1, [&](auto a) { ++calls; return same<decltype(a), double> ? 8 : 0; }) == 8 && calls == 1);
  CHECK(with_acc(0, [&](auto a) { ++calls; return same<decltype(a), float> ? 4 : 0; }) == 4 && calls == 2);

  // with_value: exact match, in any listed order
  calls = 0;
  auto value = [&](auto v) { ++calls; return 100 + decltype(v)::value; };
  CHECK((with_value<4, 8, 16, 32>(16, value) == 116) && calls == 1);
  CHECK((with_value<8, 4, 2>(2, value) == 102) && calls == 2);
  CHECK((with_value<4, 8, 16, 32>(9, value) == -1) && calls == 2);
  CHECK((with_value<4, 8, 16, 32>(64, value, -2) == -2) && calls == 2);
  CHECK((with_value<1>(1, [&](auto v) { ++calls; return same<decltype(v), std::integral_constant<int, 1>> ? -9 : 0; }) == -9) &&
        calls == 3);

  // with_ceil: the first rung at v = V, the next at v = V + 1, nothing past the last
  calls = 0;
  CHECK((with_ceil<4, 8, 16>(-5, value) == 104) && calls == 1);
  CHECK((with_ceil<4, 8, 16>(4, value) == 104) && calls == 2);
  CHECK((with_ceil<4, 8, 16>(5, value) == 108) && calls == 3);
  CHECK((with_ceil<4, 8, 16>(8, value) == 108) && calls == 4);
  CHECK((with_ceil<4, 8, 16>(9, value) == 116) && calls == 5);
  CHECK((with_ceil<4, 8, 16>(16, value) == 116) && calls == 6);
  CHECK((with_ceil<4, 8, 16>(17, value) == -1) && calls == 6);
  CHECK((with_ceil<4, 8, 16>(17, value, -3) == -3) && calls == 6);

  // with_bool
  calls = 0;
  CHECK(with_bool(5, [&](auto f) { ++calls; return same<decltype(f), std::true_type> ? 1 : 0; }) == 1 && calls == 1);
  CHECK(with_bool(0, [&](auto f) { ++calls; return same<decltype(f), std::false_type> ? 2 : 0; }) == 2 && calls == 2);

  // nested: one call of the innermost, a miss of the inner visitor comes out
  calls = 0;
  auto nested = [&](int code, int w) {
    return with_dtype<float, double>(code, [&](auto t) {
      return with_value<1, 2>(w, [&](auto v) { ++calls; return (int)sizeof(typename decltype(t)::T) + decltype(v)::value; }, -2);
    });
  };
  CHECK(nested(DT_F64, 2) == 10 && calls == 1);
  CHECK(nested(DT_F64, 3) == -2 && calls == 1);
  CHECK(nested(DT_I32, 2) == -1 && calls == 1);

  std::printf("%s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
"""


def test_visitors(tmp_path):
    src, exe = tmp_path / "dispatch_check.hip", tmp_path / "dispatch_check"
    src.write_text(PROGRAM)
    b._run([b._hipcc(), "--offload-host-only", "-std=c++17", "-O1", "-I", b.CSRC, str(src), "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout


def test_one_mechanism():
    """Every kernel source sees the visitors through common.h, and none keeps a copy of its own."""
    with open(os.path.join(b.CSRC, "common.h")) as f:
        assert '#include "dispatch.h"' in f.read()
    srcs, hdrs = b.kernel_sources()
    for p in srcs + [h for h in hdrs if not h.endswith("dispatch.h")]:
        with open(p) as f:
            text = f.read()
        for name in ("with_dtype", "with_acc", "with_value", "with_ceil", "with_bool"):
            assert ("int %s(" % name) not in text, (p, name)
