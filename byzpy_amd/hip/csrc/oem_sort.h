// Batcher's odd-even merge sort as a compile-time index schedule.
//
// The schedule only names WHICH pairs are compare-exchanged, in which
// order; what a compare-exchange does is the caller's functor
//   ce(lo, hi):  afterwards element lo holds the smaller, hi the larger.
// selnet.h's half_sort instantiates it for the kernels of colsel.hip (f32
// registers, packed u16 keys, packed raw bf16 words);
// tests/oem_sort_check.cpp instantiates it on host arrays and proves it by
// the 0-1 principle. Every loop bound is a constant once
// the enclosing loops are unrolled, so on the device all indices are
// compile-time and the element array stays in registers.
//
// Cost: N = 8 / 16 / 32 take 19 / 63 / 191 compare-exchanges (bitonic:
// 24 / 80 / 240) at the same depth, log2(N) * (log2(N) + 1) / 2.
#pragma once

#if defined(__HIPCC__)
#define OEM_FN __host__ __device__ __forceinline__
#else
#define OEM_FN inline
#endif

namespace oem {

// One level of the sort: every aligned block of 2 * RUN elements holds two
// sorted runs of RUN elements and leaves as one sorted run. UP = false is
// the mirrored network (index i -> N - 1 - i): it takes and leaves
// DESCENDING runs.
template <int N, int RUN, bool UP, typename CE>
OEM_FN void merge_runs(CE& ce) {
#pragma unroll
  for (int k = RUN; k >= 1; k >>= 1) {
#pragma unroll
    for (int j = k % RUN; j + k < N; j += 2 * k) {
#pragma unroll
      for (int i = 0; i < k; ++i) {
        const int a = i + j, b = i + j + k;
        if (b < N && a / (2 * RUN) == b / (2 * RUN)) {
          if (UP) ce(a, b);
          else ce(N - 1 - a, N - 1 - b);
        }
      }
    }
  }
}

// Full sort of N elements (N a power of two): runs of 1, 2, 4, ... N / 2.
template <int N, bool UP, int RUN = 1, typename CE>
OEM_FN void sort(CE& ce) {
  if constexpr (RUN < N) {
    merge_runs<N, RUN, UP>(ce);
    sort<N, UP, 2 * RUN>(ce);
  }
}

// The last level alone: merges the sorted halves of N elements.
template <int N, bool UP, typename CE>
OEM_FN void merge(CE& ce) {
  merge_runs<N, N / 2, UP>(ce);
}

}  // namespace oem
