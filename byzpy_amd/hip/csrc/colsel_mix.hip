// Mixed column selection (K18): the column median / trimmed mean of
// Y = W X without Y. X is (n, d) bf16, W the (m, n) row map of a mixing
// pre-aggregator (NNM, Bucketing): a 0/1 membership matrix `mix` times
// 1 / row count, n and m <= 64. The composition writes the (m, d) matrix Y
// (rounded to bf16) and reads it back; here the matrix pipe rebuilds every
// mixed column next to the selection network that consumes it.
//
// A wave works on strips of 64 columns, one column per lane:
//  - load: lane l reads column 64 s + l of every row (one 128 B wave
//    transaction per row, the walk of colsel_reg_kernel), packs row pairs
//    into 32 words and writes them to its wave's PRIVATE LDS slab as
//    [column][row] (8 ds_write_b128, column stride 2 KN + 16 B: an odd
//    number of 16 B slots). No wave reads another wave's slab, so the strip
//    loop has no block barrier (wave_lds_fence).
//  - product: v_mfma_f32_32x32x16_bf16 with W's 0/1 pattern as A (built once
//    per wave from the bit rows of mix_prep_kernel: 1.0 and 0.0 are exact in
//    bf16) and the slab as B: lane (h, j) = (l >> 5, l & 31) reads rows
//    16 k + 8 h .. + 7 of column 32 t + j, 16 contiguous bytes. 2 M-tiles
//    (m > 32) x 2 N-tiles x ceil(n / 16) k-steps, f32 accumulation.
//  - one lane, one column: of C tile (u, t) lane (h, j) holds column
//    32 t + j and the rows 32 u + 8 (r / 4) + 4 h + r % 4 of register r. One
//    v_permlane32_swap of register r of (u, 0) with register r of (u, 1)
//    hands lanes >= 32 the h = 0 rows of column 32 + j and lanes < 32 the
//    h = 1 rows of column j: 32 swaps, and lane l owns all m sums of column
//    l, each at a compile-time slot.
//  - selection: scale by 1 / count, pad the slots >= m as colsel_reg_kernel
//    does and run selnet.h's networks on the f32 registers.
//
// Values that are not finite. 0 x inf is NaN in the matrix pipe, and a row
// that is no member of y_i must not touch it. Every packed word is tested
// for an all-ones exponent (two VALU per row pair, OR-ed into one flag); a
// lane whose column holds one (rare, divergent) zeroes those words before
// they reach the slab and notes their rows in a 64-bit mask. After the
// product it adds, with plain f32 adds, the members it took out back to the
// sums that own them, read again from X: y_i is then the f32 sum of exactly
// its members (+inf members give +inf, mixed infinities or a NaN give NaN).
// The min/max networks would drop a NaN, so that lane also counts its NaN
// sums and turns them into +inf: they rank last, as torch.sort ranks them,
// and the result is NaN exactly where a counted slot is selected.
#include "colsel_shared.h"
#include "launchers.h"
#include "selnet.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 mix_bf16x8;
typedef __attribute__((ext_vector_type(16))) float mix_f32x16;
typedef __attribute__((ext_vector_type(4))) u32 mix_u32x4;
typedef unsigned long long u64;

constexpr int MIX_THREADS = 256;
constexpr int MIX_WAVES = MIX_THREADS / 64;
constexpr int MIX_BLOCKS_PER_CU = 2;

// scratch layout (COLSEL_MIX_SCRATCH_WORDS u64): bit rows, then 1 / count
// as f32, then one flag: some row of mix is empty (its y is 0 / 0)
constexpr int MIX_INV_WORD = 64, MIX_FLAG_WORD = 96;

// Thread i < m: bit k of wbits[i] = (mix[i][k] != 0), inv[i] = 1 / popcount.
// Rows past m get no bits. One wave.
__global__ void __launch_bounds__(64)
mix_prep_kernel(const unsigned char* __restrict__ mix, int m, int n,
                u64* __restrict__ scratch) {
  const int i = threadIdx.x;
  u64 bits = 0;
  if (i < m)
    for (int k = 0; k < n; ++k)
      bits |= (u64)(mix[i * n + k] != 0) << k;
  scratch[i] = bits;
  float* const inv = reinterpret_cast<float*>(scratch + MIX_INV_WORD);
  inv[i] = 1.0f / (float)__popcll(bits);
  const bool empty = i < m && bits == 0;
  const int any_empty = __any(empty);
  if (i == 0) *reinterpret_cast<int*>(scratch + MIX_FLAG_WORD) = any_empty;
}

DEV float bf16_bits_to_f(u32 bits) { return __uint_as_float(bits << 16); }

// P: selection width (m padded), KN: row width of the load walk and the
// slab (n padded to 32 / 64)
template <int P, int KN, int MODE>
__global__ void __launch_bounds__(MIX_THREADS, MIX_BLOCKS_PER_CU)
colsel_mix_bf16_kernel(const unsigned short* __restrict__ X,
                       const u64* __restrict__ scratch,
                       unsigned short* __restrict__ out, int n, int m, long d,
                       int f) {
  constexpr int MU = P > 32 ? 2 : 1;  // M-tiles of 32 mixed rows
  constexpr int KS = KN / 16;         // k-steps of 16 rows
  constexpr int COLB = 2 * KN + 16;   // slab bytes per column
  __shared__ __attribute__((aligned(16))) char img[MIX_WAVES * 64 * COLB];
  const u64* __restrict__ wbits = scratch;
  const float* __restrict__ inv =
      reinterpret_cast<const float*>(scratch + MIX_INV_WORD);
  const bool any_empty =
      *reinterpret_cast<const int*>(scratch + MIX_FLAG_WORD) != 0;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fj = lane & 31, fh = lane >> 5;
  char* const slab = img + wave * (64 * COLB);
  char* const wr = slab + lane * COLB;
  const char* const rd = slab + fj * COLB + 16 * fh;

  // A fragments: row 32 u + j of W, columns 16 s + 8 h .. + 7, as 0.0 / 1.0
  mix_bf16x8 a[MU][KS];
#pragma unroll
  for (int u = 0; u < MU; ++u) {
    const u64 w = wbits[32 * u + fj];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const u32 byte = (u32)(w >> (16 * s + 8 * fh)) & 0xFFu;
      mix_u32x4 q;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        q[e] = (((byte >> (2 * e)) & 1u) ? 0x3F80u : 0u) |
               (((byte >> (2 * e + 1)) & 1u) ? 0x3F800000u : 0u);
      a[u][s] = __builtin_bit_cast(mix_bf16x8, q);
    }
  }

  const int ksteps = (n + 15) >> 4;
  const long nstrips = (d + 63) >> 6;
  const long nwaves = (long)gridDim.x * MIX_WAVES;
  for (long strip = (long)blockIdx.x * MIX_WAVES + wave; strip < nstrips;
       strip += nwaves) {
    const long col = strip * 64 + lane;
    const long ccol = min(col, d - 1);  // tail lanes: clamped, not stored

    // pinned raw-load walk: see colsel_reg_kernel's load phase. Slots past
    // n repeat row n - 1; W has no bits there.
    // The row walk is a wave-uniform base on the scalar unit plus one
    // per-lane byte offset; its bounds are opaque per strip, or the KN
    // chosen steps are hoisted out of the strip loop into SGPRs that spill.
    u32 raw[KN];
    const char* base = reinterpret_cast<const char*>(X + strip * 64);
    const u32 off = (u32)(ccol - strip * 64) * 2u;
    int n_walk = n;
    long rowbytes = d * 2;
    asm volatile("" : "+s"(n_walk), "+s"(rowbytes));
#pragma unroll
    for (int i = 0; i < KN; ++i) {
      raw[i] = *reinterpret_cast<const unsigned short*>(base + off);
      if (i + 1 < n_walk) base += rowbytes;
      __builtin_amdgcn_sched_barrier(0);
    }
    u32 pk[KN / 2];
    u32 flag = 0;
#pragma unroll
    for (int q = 0; q < KN / 2; ++q) {
      pk[q] = raw[2 * q] | (raw[2 * q + 1] << 16);
      // exponent field + 1 carries into the half's top bit iff all ones
      flag |= (pk[q] & 0x7F807F80u) + 0x00800080u;
    }
    u64 bad = 0;  // rows of this column taken out of the product
    if (flag & 0x80008000u) {
#pragma unroll
      for (int q = 0; q < KN / 2; ++q) {
        if ((pk[q] & 0x7F80u) == 0x7F80u) {
          pk[q] &= 0xFFFF0000u;
          bad |= 1ull << (2 * q);
        }
        if ((pk[q] & 0x7F800000u) == 0x7F800000u) {
          pk[q] &= 0x0000FFFFu;
          bad |= 1ull << (2 * q + 1);
        }
      }
    }

    wave_lds_fence();  // the last strip's fragment reads stay above the stores
#pragma unroll
    for (int c = 0; c < KN / 8; ++c)
      *reinterpret_cast<mix_u32x4*>(wr + 16 * c) =
          mix_u32x4{pk[4 * c], pk[4 * c + 1], pk[4 * c + 2], pk[4 * c + 3]};
    wave_lds_fence();  // the slab is complete for this wave's own reads

    mix_f32x16 acc[MU][2];
#pragma unroll
    for (int u = 0; u < MU; ++u)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[u][t][r] = 0.0f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (s == 0 || s < ksteps) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const mix_bf16x8 b = *reinterpret_cast<const mix_bf16x8*>(
              rd + t * 32 * COLB + 32 * s);
#pragma unroll
          for (int u = 0; u < MU; ++u)
            acc[u][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                a[u][s], b, acc[u][t], 0, 0, 0);
        }
      }
    }

    // lane l takes column l: the swap trades the upper lanes of its first
    // operand (tile t = 0, rows of h = 1) for the lower lanes of its second
    // (tile t = 1, rows of h = 0)
    float v[P];
#pragma unroll
    for (int u = 0; u < MU; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row0 = 32 * u + 8 * (r / 4) + (r % 4);
        if (row0 < P) {
          const auto sw = __builtin_amdgcn_permlane32_swap(
              __float_as_uint(acc[u][0][r]), __float_as_uint(acc[u][1][r]),
              false, false);
          v[row0] = __uint_as_float(sw[0]);
          v[row0 + 4] = __uint_as_float(sw[1]);
        }
      }

    // m in a VGPR (vecify), opaque per strip like the bounds derived from
    // it below: hoisted out of the strip loop, the unrolled `i >= m`
    // compares would stay live as 64 mask pairs and spill
    int mv = vecify(m);
    asm volatile("" : "+v"(mv));
    const bool rare = bad != 0 || any_empty;
    if (bad != 0) {
      // the members taken out, added back to the sums that own them. The
      // bit rows are read here, through a pointer the compiler cannot see
      // through: hoisted out of the strip loop they would hold 128 SGPRs
      const u64* wb = wbits;
      asm volatile("" : "+s"(wb));
#pragma unroll
      for (int i = 0; i < P; ++i) {
        u64 hit = wb[i] & bad;
        float add = 0.0f;
        while (hit) {
          const int k = __builtin_ctzll(hit);
          hit &= hit - 1;
          add += bf16_bits_to_f(X[(long)k * d + ccol]);
        }
        v[i] += add;
      }
    }
    // 1 / count by scalar loads, per strip for the same reason
    const float* invp = inv;
    asm volatile("" : "+s"(invp));
#pragma unroll
    for (int i = 0; i < P; ++i) v[i] *= invp[i];
    int cnan = 0;  // NaN sums of this column, ranked last as +inf
    if (rare) {
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (i < mv && v[i] != v[i]) {
          v[i] = PAD;
          ++cnan;
        }
    }

    float result;
    if (MODE == MEDIAN) {
      // pad split as in colsel_reg_kernel: the median lands on ranks
      // P/2 - 1 and P/2
      int n_lo = vecify(selnet::median_pad_split<P>(m));
      asm volatile("" : "+v"(n_lo));
      if (m < P) {
#pragma unroll
        for (int i = 0; i < P; ++i)
          if (i >= mv) v[i] = (i < n_lo) ? -PAD : PAD;
      }
      float mlo, mhi;
      selnet::median_network<P, F32MinMax>(v, mlo, mhi);
      result = (m & 1) ? mlo : 0.5f * (mlo + mhi);
      // sorted position m / 2 lies among the last cnan
      if (cnan > 0 && (m >> 1) >= m - cnan) result = __builtin_nanf("");
    } else {
      if (m < P) {
#pragma unroll
        for (int i = 0; i < P; ++i)
          if (i >= mv) v[i] = PAD;
      }
      // Batcher's network over all P slots (543 compare-exchanges at
      // P = 64, bitonic 672)
      selnet::half_sort<P, true, F32MinMax>(v);
      int fv = vecify(f), mfv = vecify(m - f);
      asm volatile("" : "+v"(fv), "+v"(mfv));
      float s = 0.0f;
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (i >= fv && i < mfv) s += v[i];
      result = s / (float)(m - 2 * f);
      if (cnan > f) result = __builtin_nanf("");  // position m - f - 1
    }
    if (col < d) {
      union { unsigned short s; __hip_bfloat16 h; } o;
      o.h = __float2bfloat16(result);
      out[col] = o.s;
    }
  }
}

}  // namespace

void launch_colsel_mix_bf16(const __hip_bfloat16* X, const unsigned char* mix,
                            unsigned long long* scratch, __hip_bfloat16* out,
                            int n, int m, long d, int mode, int f,
                            hipStream_t stream) {
  hipLaunchKernelGGL(mix_prep_kernel, dim3(1), dim3(64), 0, stream, mix, m, n,
                     scratch);
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess ||
      cus < 1)
    cus = 256;
  // persistent grid: the waves stride over the strips
  const long nstrips = (d + 63) / 64;
  const long need = (nstrips + MIX_WAVES - 1) / MIX_WAVES;
  const long cap = (long)MIX_BLOCKS_PER_CU * cus;
  const unsigned blocks = (unsigned)(need < cap ? need : cap);
  const unsigned short* Xu = reinterpret_cast<const unsigned short*>(X);
  unsigned short* Ou = reinterpret_cast<unsigned short*>(out);
  auto launch = [&](auto md, auto p, auto kn) {
    hipLaunchKernelGGL(
        (colsel_mix_bf16_kernel<decltype(p)::value, decltype(kn)::value,
                                decltype(md)::value>),
        dim3(blocks), dim3(MIX_THREADS), 0, stream, Xu,
        (const unsigned long long*)scratch, Ou, n, m, d, f);
  };
  auto by_rows = [&](auto md, auto p) {
    if (n <= 32) launch(md, p, std::integral_constant<int, 32>{});
    else launch(md, p, std::integral_constant<int, 64>{});
  };
  by_reg_width(m, [&](auto p) {
    if (mode == MEDIAN) by_rows(std::integral_constant<int, MEDIAN>{}, p);
    else by_rows(std::integral_constant<int, TRIMMED>{}, p);
  });
}
