// Host proof of the odd-even merge schedule in byzpy_amd/hip/csrc/oem_sort.h
// by the 0-1 principle (a network that sorts every 0-1 input sorts every
// input). Built and run by tests/test_oem_sort_and_colsel_gram_args.py.
//
//   sort<8>, sort<16>: all 2^8 / 2^16 inputs, ascending and descending;
//   merge<32>:         all 17 x 17 pairs of sorted 0-1 halves, both ways;
//   sort<32>:          its compare-exchange list is sort<16> on each half
//                      followed by merge<32>, so the two facts above prove
//                      it; 2^32 inputs are out of reach, a sample is run on
//                      top;
//   counts:            191 compare-exchanges for 32 inputs, 63 for 16.
//
// and of the networks built on it in byzpy_amd/hip/csrc/selnet.h, on int
// arrays with an integer min/max policy, for P = 8, 16, 32, 64:
//   median_select:     every [ascending 0-1 half | descending 0-1 half],
//                      (P/2 + 1)^2 inputs: mlo / mhi are ranks P/2-1 / P/2
//                      (0-1 principle: all inputs of that shape);
//   whole median path: every n in 1..P on n values of 3 levels, every
//                      count-split of the levels, in a fixed and in the
//                      reversed arrangement, padded at median_pad_split,
//                      through median_network: the median of the n values;
//   bitonic_sort:      every 0-1 input for P <= 16, for larger P every 0-1
//                      input that is constant on aligned runs of P / 16.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "oem_sort.h"
#include "selnet.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL: %s\n", what);
    ++failures;
  }
}

struct ArrayCE {
  int* v;
  long count = 0;
  void operator()(int lo, int hi) {
    ++count;
    if (v[lo] > v[hi]) std::swap(v[lo], v[hi]);
  }
};

struct RecordCE {
  std::vector<std::pair<int, int>> list;
  void operator()(int lo, int hi) { list.emplace_back(lo, hi); }
};

template <int N, bool UP>
bool is_sorted_dir(const int (&v)[N]) {
  for (int i = 0; i + 1 < N; ++i)
    if (UP ? v[i] > v[i + 1] : v[i] < v[i + 1]) return false;
  return true;
}

template <int N, bool UP>
void exhaustive_sort() {
  bool ok = true;
  for (uint32_t bits = 0; bits < (1u << N); ++bits) {
    int v[N], ones = 0;
    for (int i = 0; i < N; ++i) ones += v[i] = (bits >> i) & 1;
    ArrayCE ce{v};
    oem::sort<N, UP>(ce);
    int after = 0;
    for (int i = 0; i < N; ++i) after += v[i];
    ok = ok && after == ones && is_sorted_dir<N, UP>(v);
  }
  char what[64];
  std::snprintf(what, sizeof what, "sort<%d> %s over all 0-1 inputs", N,
                UP ? "up" : "down");
  expect(ok, what);
}

// halves sorted in the direction of the merge, a and b ones in them
template <bool UP>
void merge32_all_pairs() {
  bool ok = true;
  for (int a = 0; a <= 16; ++a)
    for (int b = 0; b <= 16; ++b) {
      int v[32];
      for (int i = 0; i < 16; ++i) {
        // ascending half: zeros first; descending half: ones first
        v[i] = UP ? (i >= 16 - a) : (i < a);
        v[16 + i] = UP ? (i >= 16 - b) : (i < b);
      }
      ArrayCE ce{v};
      oem::merge<32, UP>(ce);
      int ones = 0;
      for (int i = 0; i < 32; ++i) ones += v[i];
      ok = ok && ones == a + b && is_sorted_dir<32, UP>(v);
    }
  expect(ok, UP ? "merge<32> up over 17 x 17 sorted halves"
                : "merge<32> down over 17 x 17 sorted halves");
}

template <bool UP>
void sort32_is_two_sort16_then_merge() {
  RecordCE full, half, last;
  oem::sort<32, UP>(full);
  oem::sort<16, UP>(half);
  oem::merge<32, UP>(last);
  // every level of sort<32> below the last works on both halves at once,
  // and the two halves share no element: the subsequence of pairs inside
  // [0, 16) must be sort<16>'s list, the one inside [16, 32) that list
  // shifted by 16 (for the mirrored network too: 31 - i = 16 + (15 - i))
  const size_t nlow = 2 * half.list.size();
  bool ok = full.list.size() == nlow + last.list.size();
  if (ok) {
    std::vector<std::pair<int, int>> lo, hi, hi_want;
    for (size_t i = 0; i < nlow; ++i) {
      const auto p = full.list[i];
      if ((p.first < 16) != (p.second < 16)) ok = false;  // crosses halves
      (p.first < 16 ? lo : hi).push_back(p);
    }
    for (auto p : half.list) hi_want.emplace_back(p.first + 16, p.second + 16);
    ok = ok && lo == half.list && hi == hi_want;
    ok = ok && std::equal(last.list.begin(), last.list.end(),
                          full.list.begin() + nlow);
  }
  expect(ok, UP ? "sort<32> up = sort<16> per half, then merge<32>"
                : "sort<32> down = sort<16> per half, then merge<32>");
}

template <bool UP>
void sort32_sample() {
  bool ok = true;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (int trial = 0; trial < 20000; ++trial) {
    int v[32], ref[32];
    for (int i = 0; i < 32; ++i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      // few distinct values in some trials, many in others: ties matter
      v[i] = ref[i] = (int)((s >> 33) % (trial % 2 ? 4 : 65536));
    }
    ArrayCE ce{v};
    oem::sort<32, UP>(ce);
    std::sort(ref, ref + 32);
    if (!UP) std::reverse(ref, ref + 32);
    ok = ok && std::equal(v, v + 32, ref);
  }
  expect(ok, UP ? "sort<32> up on sampled inputs"
                : "sort<32> down on sampled inputs");
}

template <int N>
long count_ces() {
  int v[N] = {};
  ArrayCE ce{v};
  oem::sort<N, true>(ce);
  return ce.count;
}

struct IntMinMax {
  static int mn(int a, int b) { return std::min(a, b); }
  static int mx(int a, int b) { return std::max(a, b); }
};

template <int P>
void median_select_all_01_halves() {
  bool ok = true;
  for (int za = 0; za <= P / 2; ++za)
    for (int zb = 0; zb <= P / 2; ++zb) {
      int v[P], ref[P];
      for (int i = 0; i < P / 2; ++i) {
        v[i] = i >= za;               // ascending: za zeros first
        v[P / 2 + i] = i < P / 2 - zb;  // descending: zb zeros last
      }
      std::copy(v, v + P, ref);
      std::sort(ref, ref + P);
      int mlo = -1, mhi = -1;
      selnet::median_select<P, IntMinMax>(v, mlo, mhi);
      ok = ok && mlo == ref[P / 2 - 1] && mhi == ref[P / 2];
    }
  char what[80];
  std::snprintf(what, sizeof what,
                "median_select<%d> over %d x %d sorted 0-1 halves", P,
                P / 2 + 1, P / 2 + 1);
  expect(ok, what);
}

// n real values of levels 1, 2, 3 (c1, c2, n - c1 - c2 of each), laid out by
// a fixed scatter or its reverse; pads 0 below and 4 above, split where the
// kernels split them
template <int P>
void median_path_all_n() {
  bool ok = true;
  long cases = 0;
  for (int n = 1; n <= P; ++n) {
    const int n_lo = selnet::median_pad_split<P>(n);
    ok = ok && n_lo >= n && n_lo <= P;
    for (int c1 = 0; c1 <= n; ++c1)
      for (int c2 = 0; c1 + c2 <= n; ++c2)
        for (int rev = 0; rev < 2; ++rev) {
          int real[P], v[P];
          for (int i = 0; i < n; ++i) {
            // 37 is coprime to every n <= 64 but 37 itself
            const int slot = n == 37 ? i : (int)((37L * i + 11) % n);
            real[rev ? n - 1 - slot : slot] = i < c1 ? 1 : (i < c1 + c2 ? 2 : 3);
          }
          for (int i = 0; i < P; ++i) v[i] = i < n ? real[i] : (i < n_lo ? 0 : 4);
          std::sort(real, real + n);
          int mlo = -1, mhi = -1;
          selnet::median_network<P, IntMinMax>(v, mlo, mhi);
          if (n & 1) mhi = mlo;  // as the kernels do
          ok = ok && mlo == real[(n - 1) >> 1] && mhi == real[n >> 1];
          ++cases;
        }
  }
  char what[80];
  std::snprintf(what, sizeof what,
                "median_network<%d>: median of n = 1..%d padded values (%ld cases)",
                P, P, cases);
  expect(ok, what);
}

template <int P>
void bitonic_sort_01_runs() {
  constexpr int RUN = P <= 16 ? 1 : P / 16, BITS = P / RUN;
  bool ok = true;
  for (uint32_t bits = 0; bits < (1u << BITS); ++bits) {
    int v[P], ones = 0;
    for (int i = 0; i < P; ++i) ones += v[i] = (bits >> (i / RUN)) & 1;
    selnet::bitonic_sort<P, IntMinMax>(v);
    int after = 0;
    for (int i = 0; i < P; ++i) after += v[i];
    ok = ok && after == ones && is_sorted_dir<P, true>(v);
  }
  char what[96];
  std::snprintf(what, sizeof what,
                "bitonic_sort<%d> over all 0-1 inputs constant on runs of %d",
                P, RUN);
  expect(ok, what);
}

template <int P>
void selnet_checks() {
  median_select_all_01_halves<P>();
  median_path_all_n<P>();
  bitonic_sort_01_runs<P>();
  // half<H> is a view, extract_at a read
  int v[P];
  for (int i = 0; i < P; ++i) v[i] = 100 + i;
  bool ok = &selnet::half<0>(v)[0] == &v[0] && &selnet::half<1>(v)[0] == &v[P / 2];
  for (int i = 0; i < P; ++i) ok = ok && selnet::extract_at(v, i) == 100 + i;
  expect(ok, "half<H> views v in place, extract_at(v, i) is v[i]");
}

}  // namespace

int main() {
  exhaustive_sort<8, true>();
  exhaustive_sort<8, false>();
  exhaustive_sort<16, true>();
  exhaustive_sort<16, false>();
  merge32_all_pairs<true>();
  merge32_all_pairs<false>();
  sort32_is_two_sort16_then_merge<true>();
  sort32_is_two_sort16_then_merge<false>();
  sort32_sample<true>();
  sort32_sample<false>();
  expect(count_ces<32>() == 191, "191 compare-exchanges for 32 inputs");
  expect(count_ces<16>() == 63, "63 compare-exchanges for 16 inputs");
  expect(count_ces<8>() == 19, "19 compare-exchanges for 8 inputs");
  selnet_checks<8>();
  selnet_checks<16>();
  selnet_checks<32>();
  selnet_checks<64>();
  std::printf("bitonic_sort: exhaustive 0-1 inputs (runs of P / 16 past P = 16), "
              "not sampled permutations\n");
  if (failures == 0) std::printf("oem_sort_check: all checks passed\n");
  return failures == 0 ? 0 : 1;
}
