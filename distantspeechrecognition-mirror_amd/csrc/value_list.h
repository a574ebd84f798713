// csrc/value_list.h -- a run-time int picks one of the values a template is instantiated for (plain C++17, no HIP).
// A list is written once, `using MkCt = ints<4, 6, 8>;`, and serves both questions: has_value (the path functions) and for_value (the launch).
#pragma once
#include <type_traits>
#include <utility>

namespace dsr {

template <int... Vs> struct ints {};

// v is one of Vs
template <int... Vs> constexpr bool has_value(ints<Vs...>, int v) { return ((v == Vs) || ...); }

// calls f(std::integral_constant<int, V>{}) for the one V == v and returns true; false, and no call, when v is not listed.
// A fold over ||: the first match ends it, so f runs at most once even if a value is listed twice.  (A left fold: the compiler then instantiates
// f's bodies, and with them the kernels, in the order of the list.)
template <int... Vs, class F> bool for_value(ints<Vs...>, int v, F&& f)
{
  return (... || (v == Vs && (f(std::integral_constant<int, Vs>{}), true)));
}

}  // namespace dsr
