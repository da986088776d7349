// What the register column-selection kernels of colsel.hip and
// colsel_mix.hip share besides the networks of selnet.h: the pad value, the
// f32 min/max policy, the scalar-to-vector copy, the wave-scope LDS fence
// and the runtime-to-template switches of their launchers. Everything sits
// in an unnamed namespace: each file that includes it gets its own copy.
#pragma once
#include "common.h"
#include <type_traits>

namespace {

typedef unsigned int u32;

// +inf (not a big-finite sentinel): adversarial rows can BE +inf
// (InfAttack) and pads must never sort below a real value — with inf pads
// a pad/value tie still yields the mathematically-correct inf statistics.
#define PAD __builtin_huge_valf()

// Copy a wave-uniform int into a VGPR. Unrolled predicates like
// `i == pos` / `i >= n` (i compile-time, pos/n uniform) otherwise become
// batched s_cmp/s_cselect_b64 SGPR mask pairs — ~64 live masks spill
// through v_writelane/readlane and dominate the kernel. Against a VGPR
// operand they lower to v_cmp/v_cndmask instead (2 VALU each, no spills).
DEV int vecify(int x) {
  int r;
  asm("v_mov_b32_e32 %0, %1" : "=v"(r) : "s"(x));
  return r;
}

enum Mode { MEDIAN = 0, TRIMMED = 1, MEAMED = 2 };

// min/max policy of the selnet.h networks on f32 registers
struct F32MinMax {
  static DEV float mn(float a, float b) { return fminf(a, b); }
  static DEV float mx(float a, float b) { return fmaxf(a, b); }
};

// Orders this wave's LDS accesses before the fence against those after it,
// for the compiler only: the LDS serves one wave's operations in order.
DEV void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Turns the runtime mode / row count into the kernels' template arguments:
// fn receives std::integral_constant<int, MODE> / <int, P>.
template <typename F>
inline void by_mode(int mode, F&& fn) {
  if (mode == MEDIAN) fn(std::integral_constant<int, MEDIAN>{});
  else if (mode == TRIMMED) fn(std::integral_constant<int, TRIMMED>{});
  else fn(std::integral_constant<int, MEAMED>{});
}

// padded register width of the n <= 64 kernels
template <typename F>
inline void by_reg_width(int n, F&& fn) {
  if (n <= 8) fn(std::integral_constant<int, 8>{});
  else if (n <= 16) fn(std::integral_constant<int, 16>{});
  else if (n <= 32) fn(std::integral_constant<int, 32>{});
  else fn(std::integral_constant<int, 64>{});
}

}  // namespace
