// Register-resident selection networks on a fixed-size array, each written
// once: generic over the element type E, a min/max policy OP and a hook.
//
//   OP::mn(a, b), OP::mx(a, b)   the smaller / the larger of two elements.
//                                A compare-exchange is the two of them on
//                                the same pair, so an element may pack
//                                several keys as long as OP orders each.
//   tick(k)                      runs before every group of k OP calls of a
//                                network; the default does nothing. A caller
//                                counts the ops with it and drops work of
//                                its own between them at chosen counts
//                                (median_gram_bf16_kernel: its Gram).
//
// colsel.hip instantiates them on f32 registers (fminf / fmaxf) and on
// packed u32 words (two u16 keys, or two raw bf16 words ordered as f16);
// tests/oem_sort_check.cpp instantiates them on host arrays of int and
// proves the selection and the pad split. Like oem_sort.h the file uses no
// device builtin: all loop bounds are constants once unrolled, so on the
// device every index is compile-time and the array stays in registers.
#pragma once

#include "oem_sort.h"

namespace selnet {

struct NoTick {
  OEM_FN void operator()(int) const {}
};

// Full bitonic sort, ascending.
template <int P, typename OP, typename E, typename Tick = NoTick>
OEM_FN void bitonic_sort(E (&v)[P], Tick&& tick = Tick{}) {
#pragma unroll
  for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int l = i ^ j;
        if (l > i) {
          tick(2);
          const bool asc = (i & k) == 0;
          const E a = v[i], b = v[l];
          const E lo = OP::mn(a, b), hi = OP::mx(a, b);
          v[i] = asc ? lo : hi;
          v[l] = asc ? hi : lo;
        }
      }
    }
  }
}

// Sort of one half of a median's array: UP = true ascending, UP = false the
// mirrored (descending) network. Why a half at a time, and why the order in
// the source matters: sorting a half touches only its own P2 elements, so a
// kernel that converts and sorts the FIRST half before it touches the second
// lets those compare-exchanges issue while the second half's row loads are
// still in flight (a network over all P elements takes every load in its
// first phase and waits for the last one before any compute).
// The schedule is Batcher's odd-even merge sort (oem_sort.h): 191
// compare-exchanges per 32 elements against the bitonic network's 240 at the
// same depth.
template <int P2, bool UP, typename OP, typename E, typename Tick = NoTick>
OEM_FN void half_sort(E (&v)[P2], Tick&& tick = Tick{}) {
  auto ce = [&](int lo, int hi) __attribute__((always_inline)) {
    tick(2);
    const E a = v[lo], b = v[hi];
    v[lo] = OP::mn(a, b);
    v[hi] = OP::mx(a, b);
  };
  oem::sort<P2, UP>(ce);
}

// Ranks P/2-1 (mlo) and P/2 (mhi) of [ascending P/2 | descending P/2], a
// bitonic sequence: one elementwise min/max pass splits it into the smallest
// and the largest P/2 elements, then rank P/2-1 is the maximum of the lower
// and rank P/2 the minimum of the upper set: 3P/2 - 2 ops replacing the
// last merge phase of a sort (P/2 * log2(P) compare-exchanges) PLUS two O(P)
// predicated rank extractions. The caller pads so that the median lands on
// exactly these ranks (median_pad_split).
template <int P, typename OP, typename E, typename Tick = NoTick>
OEM_FN void median_select(E (&v)[P], E& mlo, E& mhi, Tick&& tick = Tick{}) {
#pragma unroll
  for (int i = 0; i < P / 2; ++i) {
    tick(2);
    const E a = v[i], b = v[i + P / 2];
    v[i] = OP::mn(a, b);
    v[i + P / 2] = OP::mx(a, b);
  }
#pragma unroll
  for (int s = P / 4; s >= 1; s >>= 1)
#pragma unroll
    for (int i = 0; i < s; ++i) {
      tick(2);
      v[i] = OP::mx(v[i], v[i + s]);
      v[P / 2 + i] = OP::mn(v[P / 2 + i], v[P / 2 + s + i]);
    }
  mlo = v[0];
  mhi = v[P / 2];
}

// Pad split of the median: with n real elements in slots [0, n), slots
// [n, median_pad_split<P>(n)) take a pad below every element and the slots
// from there to P a pad above, and ranks P/2-1 and P/2 of the P slots are
// then the sorted positions (n-1)/2 and n/2 of the real ones (the same
// position twice for odd n, where the higher rank is not a median and the
// caller drops it).
template <int P>
OEM_FN constexpr int median_pad_split(int n) {
  return n + (P / 2 - 1 - ((n - 1) >> 1));
}

// Half H (0: lower, 1: upper) of v as an array of its own.
template <int H, int P, typename E>
OEM_FN E (&half(E (&v)[P]))[P / 2] {
  return *reinterpret_cast<E(*)[P / 2]>(&v[H * (P / 2)]);
}

// The median of a padded array: lower half ascending, upper half
// descending, select. A kernel that converts or pads per half keeps the
// three calls apart instead, with that step before each half_sort.
template <int P, typename OP, typename E, typename Tick = NoTick>
OEM_FN void median_network(E (&v)[P], E& mlo, E& mhi, Tick&& tick = Tick{}) {
  half_sort<P / 2, true, OP>(half<0>(v), tick);
  half_sort<P / 2, false, OP>(half<1>(v), tick);
  median_select<P, OP>(v, mlo, mhi, tick);
}

// v[pos] for a runtime pos, as a predicated unrolled scan (a runtime index
// would move the array out of registers).
template <int P, typename E>
OEM_FN E extract_at(const E (&v)[P], int pos) {
  E r = E(0);
#pragma unroll
  for (int i = 0; i < P; ++i)
    if (i == pos) r = v[i];
  return r;
}

}  // namespace selnet
