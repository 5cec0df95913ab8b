// Host side of every launcher: the map from an entry point's run-time arguments (a dtype code, an
// accumulator flag, a width, a ceiling, a flag) to a kernel's template arguments. Each visitor
// calls f exactly once, with a tag that carries the compile-time value, and returns f's int; when
// nothing matches it calls nothing and returns `miss`. A call site lists only the types / widths
// it ships, so no other kernel is instantiated:
//
//   return with_dtype<float, double>(dtype, [&](auto t) {
//     typedef typename decltype(t)::T T;
//     hipLaunchKernelGGL(some_kernel<T>, dim3(g), dim3(256), 0, s, (const T*)x, n, (T*)out);
//     return (int)hipGetLastError();
//   });
//
// The folds are left folds: the compiler then instantiates f (and the kernels it names) in the
// listed order, which is the order of the kernels in the code object; a right fold reverses it.
// Included from common.h (which defines FmlxDType, DTypeCode and AccOf); host code only.
#pragma once
#include <type_traits>

namespace {

// with_dtype's tag: the storage type T and its accumulator type A
template <typename T_>
struct DType {
  typedef T_ T;
  typedef typename AccOf<T_>::type A;
};

// the first of Ts (from float, double, bf16_t, int) whose FmlxDType code is `code`
template <typename... Ts, typename F>
int with_dtype(int code, F&& f, int miss = -1) {
  int r = miss;
  (void)(... || (code == DTypeCode<Ts>::value && ((r = f(DType<Ts>{})), true)));
  return r;
}

// an entry point's acc_f64 / f64 flag: f is called with a value of the accumulator type
template <typename F>
int with_acc(int acc_f64, F&& f) {
  return acc_f64 ? f(double{}) : f(float{});
}

// the V equal to v, as std::integral_constant<int, V>
template <int... Vs, typename F>
int with_value(int v, F&& f, int miss = -1) {
  int r = miss;
  (void)(... || (v == Vs && ((r = f(std::integral_constant<int, Vs>{})), true)));
  return r;
}

// the first V (listed ascending) with v <= V; a ladder whose last rung takes everything passes
// min(v, last)
template <int... Vs, typename F>
int with_ceil(int v, F&& f, int miss = -1) {
  int r = miss;
  (void)(... || (v <= Vs && ((r = f(std::integral_constant<int, Vs>{})), true)));
  return r;
}

// a flag, as std::true_type / std::false_type
template <typename F>
int with_bool(int b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace
