// Batched coefficient combine (K23) for gfx950: out = A X, A (M, n) f32,
// X (n, d) f32 or bf16, out (M, d) in X's dtype, n and M <= 128. One pass:
// every element of a read row of X comes from HBM once, every output element
// is written once, f32 accumulation on the matrix pipe, no atomics, the same
// bits from run to run. The gossip round's last step: row i of A holds node
// i's coefficients over the resident states (gramfp.hip's gossip solver).
//
// Set-up, once per workgroup. The rows of X whose column of A is all zero
// (dead rows, rows no node listens to) are compacted out of the K dimension
// in LDS and never read: `rowmap` lists the Kc rows that are left, in index
// order. Each wave then builds the A fragments of its 32-row M-tile from
// global A through rowmap and keeps them in registers for the whole launch.
//
// bf16 X. An f32 coefficient is split exactly into three bf16 parts by
// truncation, a = a1 + a2 + a3 (the 24-bit significand as 8 + 8 + 8; a part
// whose exponent field would be 0 is dropped). [A1 A2 A3] against X three
// times is then a product of bf16 numbers only, each exact in the f32
// accumulator of v_mfma_f32_32x32x16_bf16: one B fragment feeds three MFMAs.
// f32 X: v_mfma_f32_32x32x2_f32 with A unsplit. (The 32 x 32 shapes of both
// types share one C layout, so one store path serves both; M <= 128 is at
// most four M-tiles, one per wave.)
//
// Work split. A workgroup of four waves owns strips of 128 columns, N-tiles
// of 32. With MU M-tiles (1, 2 or 4) wave w takes M-tile w % MU and the MU
// N-tiles from (w / MU) MU on: 4 x 4 tile products per strip at MU = 4, and
// at MU = 1 each wave its own 32 columns. K runs in chunks of 32 compacted
// rows; a chunk of a strip is one LDS slab, shared by the four waves, and
// the slabs are double buffered: while the waves multiply chunk k out of one
// buffer, every thread already holds chunk k + 1 (of this strip or the first
// of the next) in 16 registers, loaded before the MFMAs were issued, and
// stores it to the other buffer after them. One block barrier per chunk.
//  - load: thread t reads column t % 128 of the rows 16 (t / 128) .. + 15 of
//    the chunk, a wave 64 consecutive elements of one row per instruction.
//    Element loads: d and the row starts may have any alignment. Slots past
//    Kc and columns past d are not loaded and stage as 0.
//  - bf16 slab: [column][32 rows], colsel_mix.hip's layout: column stride
//    64 + 16 B (an odd number of 16 B slots), a thread stores its 16 rows as
//    two 16 B words, lane (h, j) of the 32 x 32 x 16 B operand reads rows
//    16 s + 8 h .. + 7 of column 32 t + j as one 16 B word.
//  - f32 slab: [32 rows][128 + 32 columns], stored and read along the
//    columns: lane (h, j) of 32 x 32 x 2 reads row 2 s + h, column 32 t + j.
//  - store: of C tile (u, t) lane (h, j) holds column 32 t + j and rows
//    32 u + 8 (r / 4) + 4 h + r % 4: 32-element runs of one output row.
// The ragged last strip and tile rows past M are masked at the store.
//
// Non-finite entries of a READ row reach the matrix pipe, where 0 x inf is
// NaN: such an entry may make its column of every output non-finite. A row
// under an all-zero column of A is not read, whatever it holds.
#include "common.h"
#include "launchers.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 cb_bf16x8;
typedef __attribute__((ext_vector_type(16))) float cb_f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int cb_u32x4;
typedef unsigned int u32;

constexpr int CB_THREADS = 256;
constexpr int CB_STRIP = 128;            // columns of a strip
constexpr int CB_CHUNK = 32;             // compacted rows of a slab
constexpr int CB_COLB = 2 * CB_CHUNK + 16;  // bf16 slab: bytes per column
constexpr int CB_ROWF = CB_STRIP + 32;      // f32 slab: floats per row
constexpr int CB_BLOCKS_PER_CU = 2;

template <typename T>
struct CbSlab;
template <>
struct CbSlab<__hip_bfloat16> { static constexpr int BYTES = CB_STRIP * CB_COLB; };
template <>
struct CbSlab<float> { static constexpr int BYTES = CB_CHUNK * CB_ROWF * 4; };

DEV u32 cb_raw(const __hip_bfloat16* p) {
  return *reinterpret_cast<const unsigned short*>(p);
}
DEV u32 cb_raw(const float* p) { return __float_as_uint(*p); }

// One truncated bf16 part of x (bits) and what is left of x, exactly.
DEV u32 cb_split(float& x) {
  u32 top = __float_as_uint(x) & 0xFFFF0000u;
  if ((top & 0x7F800000u) == 0) top = 0;  // would underflow: dropped
  x -= __uint_as_float(top);
  return top >> 16;
}

// NCH: chunks the A fragments are sized for (n <= 32 NCH), MU: M-tiles
template <typename T, int NCH, int MU>
__global__ void __launch_bounds__(CB_THREADS)
combine_batched_kernel(const T* __restrict__ X, const float* __restrict__ A,
                       T* __restrict__ out, int n, int M, long d) {
  constexpr bool BF = sizeof(T) == 2;
  __shared__ __attribute__((aligned(16))) char slab[2][CbSlab<T>::BYTES];
  __shared__ int rowmap[GRAMFP_MAX_N];
  __shared__ int used[GRAMFP_MAX_N];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fj = lane & 31, fh = lane >> 5;

  // -- compaction: rowmap lists the rows some node listens to, in order ----
  if (tid < GRAMFP_MAX_N) {
    int any = 0;
    if (tid < n)
      for (int i = 0; i < M; ++i) any |= (A[(long)i * n + tid] != 0.0f);
    used[tid] = any;
  }
  __syncthreads();
  if (tid < n && used[tid]) {
    int pos = 0;
    for (int k = 0; k < tid; ++k) pos += used[k];
    rowmap[pos] = tid;
  }
  int kc = 0;
  for (int k = 0; k < n; ++k) kc += used[k];
  kc = __builtin_amdgcn_readfirstlane(kc);
  __syncthreads();
  const int nchunks = (kc + CB_CHUNK - 1) / CB_CHUNK;

  // -- A fragments of this wave's M-tile ------------------------------------
  const int mu = wave % MU;
  const int tile0 = (wave / MU) * MU;
  const int arow = 32 * mu + fj;
  // bf16: part p of rows' slots 32 c + 16 s + 8 h .. + 7; f32: slot 32 c +
  // 2 s + h
  cb_bf16x8 ab[BF ? NCH : 1][2][3];
  float af[BF ? 1 : NCH][16];
  if (BF) {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        u32 part[3][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int slot = 32 * c + 16 * s + 8 * fh + e;
          float a = 0.0f;
          if (arow < M && slot < kc) a = A[(long)arow * n + rowmap[slot]];
#pragma unroll
          for (int p = 0; p < 3; ++p) part[p][e] = cb_split(a);
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          cb_u32x4 q;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            q[e] = part[p][2 * e] | (part[p][2 * e + 1] << 16);
          ab[c][s][p] = __builtin_bit_cast(cb_bf16x8, q);
        }
      }
  } else {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int slot = 32 * c + 2 * s + fh;
        float a = 0.0f;
        if (arow < M && slot < kc) a = A[(long)arow * n + rowmap[slot]];
        af[c][s] = a;
      }
  }

  // -- staging ----------------------------------------------------------------
  const int lcol = tid & (CB_STRIP - 1);
  const int lrow = 16 * (tid >> 7);  // first of this thread's 16 chunk rows
  u32 raw[16];
  auto load = [&](long strip, int c) {
    const long col = strip * CB_STRIP + lcol;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int slot = 32 * c + lrow + e;
      raw[e] = 0;
      if (slot < kc && col < d) raw[e] = cb_raw(X + (long)rowmap[slot] * d + col);
    }
  };
  auto store = [&](int buf) {
    if (BF) {
      char* const wr = slab[buf] + lcol * CB_COLB + 2 * lrow;
#pragma unroll
      for (int q = 0; q < 2; ++q)
        *reinterpret_cast<cb_u32x4*>(wr + 16 * q) = cb_u32x4{
            raw[8 * q] | (raw[8 * q + 1] << 16),
            raw[8 * q + 2] | (raw[8 * q + 3] << 16),
            raw[8 * q + 4] | (raw[8 * q + 5] << 16),
            raw[8 * q + 6] | (raw[8 * q + 7] << 16)};
    } else {
      u32* const wr = reinterpret_cast<u32*>(slab[buf]) + lrow * CB_ROWF + lcol;
#pragma unroll
      for (int e = 0; e < 16; ++e) wr[e * CB_ROWF] = raw[e];
    }
  };

  const long nstrips = (d + CB_STRIP - 1) / CB_STRIP;
  long strip = blockIdx.x;
  if (nchunks == 0) {
    // A is all zero: so is the output
    for (; strip < nstrips; strip += gridDim.x)
      for (int i = tid; i < M * CB_STRIP; i += CB_THREADS) {
        const long col = strip * CB_STRIP + (i & (CB_STRIP - 1));
        if (col < d) out[(long)(i / CB_STRIP) * d + col] = from_f<T>(0.0f);
      }
    return;
  }
  if (strip < nstrips) {
    load(strip, 0);
    store(0);
  }
  __syncthreads();
  int buf = 0;
  for (; strip < nstrips; strip += gridDim.x) {
    cb_f32x16 acc[MU];
#pragma unroll
    for (int q = 0; q < MU; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c < nchunks) {  // block-uniform
        const bool last = c + 1 == nchunks;
        const long nstrip = last ? strip + gridDim.x : strip;
        const bool more = nstrip < nstrips;
        if (more) load(nstrip, last ? 0 : c + 1);
        const int left = kc - 32 * c;  // live slots of this chunk
        if (BF) {
          const char* const rd = slab[buf] + fj * CB_COLB + 16 * fh;
#pragma unroll
          for (int s = 0; s < 2; ++s)
            if (16 * s < left)
#pragma unroll
              for (int q = 0; q < MU; ++q) {
                const cb_bf16x8 b = *reinterpret_cast<const cb_bf16x8*>(
                    rd + (tile0 + q) * 32 * CB_COLB + 32 * s);
#pragma unroll
                for (int p = 0; p < 3; ++p)
                  acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                      ab[BF ? c : 0][s][p], b, acc[q], 0, 0, 0);
              }
        } else {
          const float* const rd =
              reinterpret_cast<const float*>(slab[buf]) + fh * CB_ROWF + fj;
#pragma unroll
          for (int s = 0; s < 16; ++s)
            if (2 * s < left)
#pragma unroll
              for (int q = 0; q < MU; ++q)
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                    af[BF ? 0 : c][s],
                    rd[2 * s * CB_ROWF + (tile0 + q) * 32], acc[q], 0, 0, 0);
        }
        if (more) store(buf ^ 1);
        __syncthreads();
        buf ^= 1;
      }
    }
#pragma unroll
    for (int q = 0; q < MU; ++q) {
      const long col = strip * CB_STRIP + (tile0 + q) * 32 + fj;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * mu + 8 * (r / 4) + 4 * fh + (r % 4);
        if (row < M && col < d) out[(long)row * d + col] = from_f<T>(acc[q][r]);
      }
    }
  }
}

template <typename T, int NCH>
void cb_launch(const T* X, const float* A, T* out, int n, int M, long d,
               unsigned blocks, hipStream_t stream) {
  if (M <= 32)
    hipLaunchKernelGGL((combine_batched_kernel<T, NCH, 1>), dim3(blocks),
                       dim3(CB_THREADS), 0, stream, X, A, out, n, M, d);
  else if (M <= 64)
    hipLaunchKernelGGL((combine_batched_kernel<T, NCH, 2>), dim3(blocks),
                       dim3(CB_THREADS), 0, stream, X, A, out, n, M, d);
  else
    hipLaunchKernelGGL((combine_batched_kernel<T, NCH, 4>), dim3(blocks),
                       dim3(CB_THREADS), 0, stream, X, A, out, n, M, d);
}

}  // namespace

template <typename T>
void launch_combine_batched(const T* X, const float* A, T* out, int n, int M,
                            long d, hipStream_t stream) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess ||
      cus < 1)
    cus = 256;
  // persistent grid: the workgroups stride over the strips
  const long nstrips = (d + CB_STRIP - 1) / CB_STRIP;
  const long cap = (long)CB_BLOCKS_PER_CU * cus;
  const unsigned blocks = (unsigned)(nstrips < cap ? nstrips : cap);
  if (n <= 32) cb_launch<T, 1>(X, A, out, n, M, d, blocks, stream);
  else if (n <= 64) cb_launch<T, 2>(X, A, out, n, M, d, blocks, stream);
  else cb_launch<T, 4>(X, A, out, n, M, d, blocks, stream);
}

INSTANTIATE_LAUNCHER(launch_combine_batched)
