// Column-wise order-statistic kernels: per-coordinate
// median / trimmed mean / mean-of-medians over the n-axis of an (n, d)
// matrix, one column per thread. Large n (> 64 at d >= 32K, always past
// 512) is served by the generic streaming radix-select engine in
// rsel.hip; this file keeps the small-n register kernels and the
// mid-n/small-d LDS sort.
//
// Two variants:
//  - register kernel (n <= 64): the column lives in a register array; the
//    sorting network is fully unrolled so every index is compile-time
//    (guide §5.4 rule 20 — runtime-indexed register arrays spill).
//    Order statistics at runtime positions are extracted with predicated
//    unrolled scans for the same reason. The networks themselves (bitonic
//    sort, half sort, median selection, pad split) are the templates of
//    selnet.h, written once for f32 registers and packed words; this file
//    supplies their min/max policies, the loads, the pads and the epilogues.
//  - LDS kernel (64 < n <= 512): one wave per block, each lane owns a
//    column staged in LDS with a +1 pad row stride (bank-conflict free,
//    guide §6 G4); runtime bitonic loops.
// Plus, for bf16 with 32 < n <= 64, the register median fused with the
// Gram in one pass over X (median_gram_bf16_kernel).
//
// Loads are coalesced: adjacent lanes read adjacent columns, so each
// row-iteration is one 256 B (f32) / 128 B (bf16) wave transaction.
#include "common.h"
#include "launchers.h"
#include "selnet.h"
#include <type_traits>

namespace {

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

// ---------------------------------------------------------------------------
// Row-indexed variants (template <bool ROWS>): the statistic runs over the
// rows named by `rows[0..n)` of an (n_src, d) matrix, as if on X[rows],
// without the gather. ROWS = false is the plain kernel and compiles to the
// code it had before the variant existed: every use of `rows` sits behind
// the compile-time flag.
//
// A row's offset rows[i] * rowstride is the same for every lane, so the
// register kernels never compute it per lane: before the column loop lane l
// of each wave stages the 64-bit BYTE offset of selected row min(l, n-1) in
// two VGPRs (one coalesced 4 B/lane read of `rows`), and the unrolled load
// phase pulls offset i into SGPRs with v_readlane (i is compile-time) —
// two readlanes and one 64-bit pointer add per row, no multiply, no
// per-lane index load. Slots past n repeat the last row, exactly like the plain walk that
// stops advancing; the pad logic overwrites them. Indices are clamped to
// [0, n_src) so a bad `rows` can misselect but never read out of bounds.
//
// v_readlane returns lane i's register whatever EXEC says, but the value is
// only defined if lane i was active when it was written AND the compiler is
// free to assume nothing about inactive lanes — so the ROWS column loops
// keep whole waves active (see wave_active) and clamp/predicate the tail
// lanes instead of dropping them.
// ---------------------------------------------------------------------------

typedef unsigned int u32;

struct RowOffsets { u32 lo, hi; };

// rowbytes: bytes from one row of X to the next
DEV RowOffsets stage_row_offsets(const int* __restrict__ rows, int n,
                                 int n_src, long rowbytes) {
  const int lane = threadIdx.x & 63;
  int r = rows[min(lane, n - 1)];
  r = min(max(r, 0), n_src - 1);
  const unsigned long off = (unsigned long)r * (unsigned long)rowbytes;
  return {(u32)off, (u32)(off >> 32)};
}

// `base` moved to selected row I (compile-time); the byte offset is a
// wave-uniform scalar pair, so the move is one 64-bit add per lane
template <int I, typename E>
DEV const E* at_row(const E* base, const RowOffsets& ro) {
  const u32 lo = __builtin_amdgcn_readlane(ro.lo, I);
  const u32 hi = __builtin_amdgcn_readlane(ro.hi, I);
  // a register pair, not (hi << 32) | lo: the compiler turns the OR of
  // disjoint halves into two separate 64-bit adds
  typedef u32 u32x2 __attribute__((ext_vector_type(2)));
  const u32x2 pair = {lo, hi};
  const unsigned long off = __builtin_bit_cast(unsigned long, pair);
  return reinterpret_cast<const E*>(reinterpret_cast<const char*>(base) + off);
}

// Column-loop condition. Plain kernels run a lane while its own unit is in
// range; ROWS kernels run the whole wave while its FIRST lane's unit is
// (tail lanes clamp their loads and skip the store).
template <bool ROWS>
DEV bool wave_active(long unit, long nunits) {
  if (ROWS) return unit - (long)(threadIdx.x & 63) < nunits;
  return unit < nunits;
}

// ---------------------------------------------------------------------------
// register variant, n <= P, P in {8, 16, 32, 64}
// ---------------------------------------------------------------------------

// min/max policy of the selnet.h networks on f32 registers
struct F32MinMax {
  static DEV float mn(float a, float b) { return fminf(a, b); }
  static DEV float mx(float a, float b) { return fmaxf(a, b); }
};

// key-value bitonic sort (sort key ascending, carry val along): it swaps on
// a comparison, so it is not a min/max network and stays here
template <int P>
DEV void bitonic_sort_kv_reg(float (&key)[P], float (&val)[P]) {
#pragma unroll
  for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int l = i ^ j;
        if (l > i) {
          const bool asc = (i & k) == 0;
          const float a = key[i], b = key[l];
          if (asc ? (a > b) : (a < b)) {
            key[i] = b; key[l] = a;
            const float t = val[i]; val[i] = val[l]; val[l] = t;
          }
        }
      }
    }
  }
}

// Indexed load phase shared by the register kernels: element I of `dst`
// comes from at_row<I>(base). Same pinned load/advance alternation as
// the plain walk (see the load-phase comment in colsel_reg_kernel).
template <int P, int I = 0, typename E>
DEV void load_rows_indexed(E (&dst)[P], const E* base, const RowOffsets& ro) {
  if constexpr (I < P) {
    dst[I] = *at_row<I>(base, ro);
    __builtin_amdgcn_sched_barrier(0);
    load_rows_indexed<P, I + 1>(dst, base, ro);
  }
}

// MEAMED keeps two live P-float arrays (values + deviation keys); at P=64
// that needs ~140 VGPRs, above the occupancy heuristic's 128 cap — the
// MEAMED instantiations get __launch_bounds__(256, 2) via this trait so the
// allocator may use 256 VGPRs instead of spilling, while MEDIAN/TRIMMED
// keep the default 4-waves/SIMD occupancy.
template <int P, int MODE, typename T, bool ROWS>
__global__ void
__launch_bounds__(256, (MODE == MEAMED && P >= 64)            ? 2
                       : (ROWS && MODE == TRIMMED && P >= 64) ? 3
                                                              : 4)
colsel_reg_kernel(const T* __restrict__ X, T* __restrict__ out,
                                  int n, long d, int f,
                                  const int* __restrict__ rows, int n_src) {
  const long col0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  RowOffsets ro = {0u, 0u};
  if (ROWS) ro = stage_row_offsets(rows, n, n_src, d * (long)sizeof(T));
  for (long col = col0; wave_active<ROWS>(col, d); col += stride) {
    float v[P];
    T raw[P];
    // Load phase. Two rules keep the address walk at ONE live base:
    // (1) raw loads only — any data-dependent convert inside the walk
    //     would force a wait per element; conversion happens after;
    // (2) sched_barrier(0) pins the load/advance alternation — without it
    //     the compiler batches all P addresses into SGPR pairs and spills
    //     them through v_writelane/readlane (~1100 VALU per column).
    // Once a load ISSUES its address registers are free; the loads stay
    // in flight and the converts below wait on counted vmcnt.
    if (ROWS) {
      // indexed walk: scalar row offset + this lane's (clamped) column
      const T* xc = X + min(col, d - 1);
      load_rows_indexed<P>(raw, xc, ro);
    } else {
      const T* p = X + col;
#pragma unroll
      for (int i = 0; i < P; ++i) {
        raw[i] = *p;
        if (i + 1 < n) p += d;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const int nv = vecify(n);

    float result;
    if (MODE == MEDIAN) {
      // selection network; each half is converted and padded right
      // before its sort (selnet::half_sort has why), so half A's work
      // overlaps the tail loads. Pad split: the low pads (-inf) put the
      // median on ranks P/2-1 / P/2; a -inf pad tying a -inf data value
      // is value-identical.
      const int n_lo = vecify(selnet::median_pad_split<P>(n));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int base = h * (P / 2);
#pragma unroll
        for (int i = base; i < base + P / 2; ++i) v[i] = to_f<T>(raw[i]);
        if (n < P) {
#pragma unroll
          for (int i = base; i < base + P / 2; ++i)
            if (i >= nv) v[i] = (i < n_lo) ? -PAD : PAD;
        }
        if (h == 0)
          selnet::half_sort<P / 2, true, F32MinMax>(selnet::half<0>(v));
        else
          selnet::half_sort<P / 2, false, F32MinMax>(selnet::half<1>(v));
      }
      float mlo, mhi;
      selnet::median_select<P, F32MinMax>(v, mlo, mhi);
      result = (n & 1) ? mlo : 0.5f * (mlo + mhi);
    } else if (MODE == TRIMMED) {
#pragma unroll
      for (int i = 0; i < P; ++i) v[i] = to_f<T>(raw[i]);
      if (n < P) {
#pragma unroll
        for (int i = 0; i < P; ++i)
          if (i >= nv) v[i] = PAD;
      }
      selnet::bitonic_sort<P, F32MinMax>(v);
      const int fv = vecify(f), nfv = vecify(n - f);
      float s = 0.0f;
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (i >= fv && i < nfv) s += v[i];
      result = s / (float)(n - 2 * f);
    } else {  // MEAMED: mean of the n-f values closest to the median
#pragma unroll
      for (int i = 0; i < P; ++i) v[i] = to_f<T>(raw[i]);
      if (n < P) {
#pragma unroll
        for (int i = 0; i < P; ++i)
          if (i >= nv) v[i] = PAD;
      }
      selnet::bitonic_sort<P, F32MinMax>(v);
      const int pos_lo = vecify((n - 1) >> 1), pos_hi = vecify(n >> 1);
      const float med =
          0.5f * (selnet::extract_at(v, pos_lo) + selnet::extract_at(v, pos_hi));
      const int nv2 = vecify(n), nfv = vecify(n - f);
      float dev[P];
#pragma unroll
      for (int i = 0; i < P; ++i)
        dev[i] = (i < nv2) ? fabsf(v[i] - med) : PAD;
      bitonic_sort_kv_reg<P>(dev, v);
      float s = 0.0f;
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (i < nfv) s += v[i];
      result = s / (float)(n - f);
    }
    if (!ROWS || col < d) out[col] = from_f<T>(result);
  }
}

// ---------------------------------------------------------------------------
// Packed bf16 median (n <= 64, even d): TWO adjacent columns per thread.
// Order statistics only need a monotone key, so bf16 values become
// sortable u16 keys (sign-flip transform) and the sorting networks run on
// v_pk_min_u16 / v_pk_max_u16 — one instruction per HALF of a
// compare-exchange (a compare-exchange is the min and the max of the same
// two registers: two packed ops) for BOTH columns (no packed f32 min/max
// exists on gfx950), with half the register footprint (P u32 regs for 2
// columns) and 4 B/lane loads.
// ---------------------------------------------------------------------------

// The min/max policies of the selnet.h networks on packed words. PkKeyU16
// orders sortable u16 keys (pk_key_from_bf16). PkRawF16 orders RAW bf16 words with no transform at all: a bf16 word is
// sign | monotone magnitude and so is an f16 word, so read as f16 two bf16
// patterns compare exactly as the values they encode — as long as neither
// is an f16 NaN or infinity, i.e. magnitude bits < 0x7C00, |x| < 2^121
// (63,488 of the 65,536 patterns). The pair returns its two inputs bit for
// bit (f16 subnormals pass through: the kernels keep f16 denormals on) and
// orders -0 below +0 in either operand order, as the u16 keys do
// (benchmarks/csrc/pkminprobe.hip measures both, and that the f16 pair
// issues as fast as the u16 pair). Callers must rule the other 2,048
// patterns out themselves (median_gram_bf16_kernel: its Gram's diagonal).
struct PkKeyU16 {
  static DEV u32 mn(u32 a, u32 b) {
    u32 r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  }
  static DEV u32 mx(u32 a, u32 b) {
    u32 r;
    asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  }
};
struct PkRawF16 {
  static DEV u32 mn(u32 a, u32 b) {
    u32 r;
    asm("v_pk_min_f16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  }
  static DEV u32 mx(u32 a, u32 b) {
    u32 r;
    asm("v_pk_max_f16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  }
};
// pad words of PkRawF16 for slots past n: the extreme legal patterns
constexpr u32 PK_RAW_PAD_LO = 0xFBFFFBFFu, PK_RAW_PAD_HI = 0x7BFF7BFFu;

// bf16 bits -> sortable u16 key, two lanes at once: per half
// key = bits ^ (sign ? 0xFFFF : 0x8000). The packed arithmetic shift
// broadcasts each half's sign to a 0x0000/0xFFFF mask in one op, so the
// transform is 3 VALU (ashr, or, xor) for both columns — it runs once
// per element on a VALU-bound kernel, so width matters.
DEV u32 pk_key_from_bf16(u32 bits) {
  u32 t;
  // shift amount lives in a VGPR as {15, 15}: a bare inline constant
  // would shift only the LOW half (VOP3P literals do not replicate)
  asm("v_pk_ashrrev_i16 %0, %2, %1"
      : "=v"(t)
      : "v"(bits), "v"(0x000F000Fu));
  return bits ^ (t | 0x80008000u);
}

// the inverse, two lanes at once: non-negative values (key bit 15 set) drop
// the bit, negative ones are complemented. 4 VALU; a bf16 word is the upper
// half of its f32, so a raw word then unpacks with one shift or mask where a
// key takes key_to_float's select per half.
DEV u32 pk_bf16_from_key(u32 key) {
  u32 t;
  asm("v_pk_ashrrev_i16 %0, %2, %1"
      : "=v"(t)
      : "v"(key), "v"(0x000F000Fu));
  return key ^ (~t | 0x80008000u);
}
DEV float pk_lo_float(u32 w) { return __uint_as_float(w << 16); }
DEV float pk_hi_float(u32 w) { return __uint_as_float(w & 0xFFFF0000u); }

DEV float key_to_float(u32 key16) {
  unsigned short bits =
      (key16 & 0x8000u) ? (unsigned short)(key16 ^ 0x8000u)
                        : (unsigned short)(~key16 & 0xFFFFu);
  union { unsigned short s; __hip_bfloat16 h; } c;
  c.s = bits;
  return __bfloat162float(c.h);
}

// MODE: MEDIAN reads its order statistics off the selection network,
// TRIMMED and MEAMED off the sorted keys (unpacked and summed in f32).
// (A four-columns-per-lane variant of this kernel, 8 B/lane row reads and
// two key arrays, was retired: its ~150 VGPRs allow 3 waves per SIMD against
// this kernel's 5 and it measured 3x slower, 9.09 vs 3.09 ms at 64 x 125M;
// docs/NOTES_R03.md, profiles/r01_bench125_kernel_stats.md.)
//
// GUARD = true is the fallback of the fused median + Gram call
// (launch_median_gram_bf16): `guard_G` is the (n, n) Gram, and every wave
// returns at once, `out` untouched, if all n diagonal entries are finite
// (one 4 B/lane read, n <= 64 lanes); else the kernel runs as always. It is
// an instantiation of its own, so that GUARD = false, which never looks at
// `guard_G`, keeps the instruction stream it had without it.
template <int P, int MODE, bool ROWS, bool GUARD = false>
__global__ void
__launch_bounds__(256, (MODE == MEDIAN && P >= 64) ? 5 : 4)
colsel_pk_median_bf16(const unsigned short* __restrict__ X,
                                      unsigned short* __restrict__ out, int n,
                                      long d, int f,
                                      const int* __restrict__ rows,
                                      int n_src,
                                      const float* __restrict__ guard_G) {
  if (GUARD) {
    const int gl = threadIdx.x & 63;
    // |g| < inf is false for +-inf and for NaN
    const bool finite =
        gl >= n || __builtin_fabsf(guard_G[(long)gl * n + gl]) < PAD;
    if (__all(finite)) return;
  }
  const long npairs = d >> 1;
  const long unit0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const long rowstride = d >> 1;  // in u32 units
  RowOffsets ro = {0u, 0u};
  if (ROWS) ro = stage_row_offsets(rows, n, n_src, rowstride * (long)sizeof(u32));
  for (long unit = unit0; wave_active<ROWS>(unit, npairs); unit += stride) {
    // ROWS: tail lanes of the last wave load a clamped (valid) pair and
    // skip the store
    const long pair = ROWS ? min(unit, npairs - 1) : unit;
    u32 v[P];
    // raw loads first + pinned alternation: see colsel_reg_kernel's load
    // phase for why (one live base, no SGPR spill storm). The walk
    // condition is vecified too — 64 uniform selects otherwise become
    // batched SGPR mask pairs.
    const u32* p = reinterpret_cast<const u32*>(X) + pair;
    if (ROWS) {
      load_rows_indexed<P>(v, p, ro);
    } else if (n == P) {
      // full tile (the flagship n=64 shape): unconditional walk, no pads
      // — drops ~190 predication VALU ops from a VALU-bound kernel
#pragma unroll
      for (int i = 0; i < P; ++i) {
        v[i] = *p;
        if (i + 1 < P) p += rowstride;
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      const int n_walk = vecify(n);
#pragma unroll
      for (int i = 0; i < P; ++i) {
        v[i] = *p;
        p += (i + 1 < n_walk) ? rowstride : 0;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const int nv = vecify(n);  // conversion/pad loops + MEAMED epilogue
    u32 sel_lo = 0u, sel_hi = 0u;
    if (MODE == MEDIAN) {
      // selection network as in colsel_reg_kernel: key transform and pads
      // per half, right before its sort. The low-pad key 0 only ties a
      // negative-NaN data key (NaN order statistics are unspecified in the
      // full-sort path too).
      const int n_lo = vecify(selnet::median_pad_split<P>(n));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int base = h * (P / 2);
#pragma unroll
        for (int i = base; i < base + P / 2; ++i)
          v[i] = pk_key_from_bf16(v[i]);
        if (n < P) {
#pragma unroll
          for (int i = base; i < base + P / 2; ++i)
            if (i >= nv) v[i] = (i < n_lo) ? 0u : 0xFFFFFFFFu;
        }
        if (h == 0)
          selnet::half_sort<P / 2, true, PkKeyU16>(selnet::half<0>(v));
        else
          selnet::half_sort<P / 2, false, PkKeyU16>(selnet::half<1>(v));
      }
      selnet::median_select<P, PkKeyU16>(v, sel_lo, sel_hi);
    } else {
#pragma unroll
      for (int i = 0; i < P; ++i) v[i] = pk_key_from_bf16(v[i]);
      if (n < P) {
#pragma unroll
        for (int i = 0; i < P; ++i)
          if (i >= nv) v[i] = 0xFFFFFFFFu;
      }
      selnet::bitonic_sort<P, PkKeyU16>(v);
    }
    const int plo = vecify((n - 1) >> 1), phi = vecify(n >> 1);
    const int fv = vecify(f), nfv = vecify(n - f);
    u32* outw = reinterpret_cast<u32*>(out);
    // One trip: the loop is what is left of the retired four-column variant,
    // which ran it once per packed pair. As straight-line code 10 of the
    // TRIMMED and MEAMED instantiations come out scheduled differently
    // (profiles/r06_colsel_networks.md), so it stays until a change that is
    // measured, not only compared, takes it out.
#pragma unroll
    for (int half = 0; half < 1; ++half) {
      float m0, m1;
      if (MODE == MEDIAN) {
        const u32 lo = sel_lo;
        const u32 hi = (n & 1) ? lo : sel_hi;
        m0 = 0.5f * (key_to_float(lo & 0xFFFFu) + key_to_float(hi & 0xFFFFu));
        m1 = 0.5f * (key_to_float(lo >> 16) + key_to_float(hi >> 16));
      } else if (MODE == TRIMMED) {
        // unpack the kept range of the sorted keys and sum
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int i = 0; i < P; ++i)
          if (i >= fv && i < nfv) {
            s0 += key_to_float(v[i] & 0xFFFFu);
            s1 += key_to_float(v[i] >> 16);
          }
        const float inv = 1.0f / (float)(n - 2 * f);
        m0 = s0 * inv;
        m1 = s1 * inv;
      } else {  // MEAMED: per half, shrink the sorted window [l, r) from
        // whichever end deviates more from the median. The walk only ever
        // touches positions [0, f] and [n-f-1, n), so those 2(f+1) sorted
        // words are staged into a per-thread LDS strip and each step reads
        // its two candidate ends by dynamic ds_read in O(1) — the previous
        // O(P) predicated extract per step cost ~f*P*4 VALU ops per column
        // pair and left the kernel 4x slower than MEDIAN.
        // Sorted, the keys have done their work: back to raw bf16 words
        // once, so that every unpack below is one shift or mask.
#pragma unroll
        for (int i = 0; i < P; ++i) v[i] = pk_bf16_from_key(v[i]);
        extern __shared__ __attribute__((aligned(16))) u32 pk_lds[];
        const int stride_l = 2 * (f + 1) + 1;  // odd => spread banks
        u32* strip = pk_lds + (int)threadIdx.x * stride_l;
        const int roff = vecify(2 * f + 2 - n);  // maps [n-f-1, n) -> [f+1, 2f+2)
#pragma unroll
        for (int i = 0; i < P; ++i) {
          if (i <= fv) strip[i] = v[i];
          if (i >= nv - fv - 1 && i < nv) strip[i + roff] = v[i];
        }
        u32 mlo = 0, mhi = 0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
          if (i == plo) mlo = v[i];
          if (i == phi) mhi = v[i];
        }
        // The sums only ever ADD kept values, never a dropped one: a dropped
        // Byzantine +-inf in a sum-then-subtract total leaves inf - inf, and
        // +-1e30 has absorbed every honest value before it is taken out
        // again. The core [f, n-f) is kept whatever the walk decides (empty
        // for 2f >= n) and is summed from the registers; the ends are added
        // from the strip once the walk has fixed the window.
        float t0 = 0.0f, t1 = 0.0f;
#pragma unroll
        for (int i = 0; i < P; ++i)
          if (i >= fv && i < nfv) {
            t0 += pk_lo_float(v[i]);
            t1 += pk_hi_float(v[i]);
          }
        int wl[2], wr[2];  // the kept window [wl, wr) of either half
#pragma unroll
        for (int half2 = 0; half2 < 2; ++half2) {
          auto val = [&](u32 w) {
            return half2 ? pk_hi_float(w) : pk_lo_float(w);
          };
          const float med = 0.5f * (val(mlo) + val(mhi));
          int l = vecify(0), r = nv;
          for (int kdrop = 0; kdrop < f; ++kdrop) {
            const float vl = val(strip[l]);
            const float vr = val(strip[r - 1 + roff]);
            const bool drop_left = (med - vl) > (vr - med);
            l += drop_left ? 1 : 0;
            r -= drop_left ? 0 : 1;
          }
          wl[half2] = l;
          wr[half2] = r;
        }
        // The ends, one strip word of each side per trip (both halves share
        // it): position j on the left, n-1-j on the right. The right side
        // stops at max(f, n-f), where for 2f >= n the left side's [0, f)
        // ends, so no position is taken twice. Selects, not products with
        // a 0/1 mask: 0 * inf is NaN.
        const int nright = vecify(min(f, n - f));
        for (int j = 0; j < f; ++j) {
          const u32 ws = strip[j];
          const int pr = nv - 1 - j;
          const u32 wd = strip[pr + roff];
          const bool right = j < nright;
          const bool kl0 = j >= wl[0] && j < wr[0];
          const bool kl1 = j >= wl[1] && j < wr[1];
          const bool kr0 = right && pr < wr[0];
          const bool kr1 = right && pr < wr[1];
          t0 += kl0 ? pk_lo_float(ws) : 0.0f;
          t1 += kl1 ? pk_hi_float(ws) : 0.0f;
          t0 += kr0 ? pk_lo_float(wd) : 0.0f;
          t1 += kr1 ? pk_hi_float(wd) : 0.0f;
        }
        const float kept = (float)(n - f);
        m0 = t0 / kept;
        m1 = t1 / kept;
      }
      union { unsigned short s[2]; u32 w; } o;
      union { unsigned short s; __hip_bfloat16 h; } c0, c1;
      c0.h = __float2bfloat16(m0);
      c1.h = __float2bfloat16(m1);
      o.s[0] = c0.s;
      o.s[1] = c1.s;
      if (!ROWS || unit < npairs) outw[pair + half] = o.w;
    }
  }
}

// ---------------------------------------------------------------------------
// Median + Gram in ONE pass over X (bf16, 32 < n <= 64, even d).
//
// The median side is colsel_pk_median_bf16<64>'s selection network on the
// RAW loaded words: every lane holds its column pair in 64 registers and
// runs the network with the packed f16 pair (PkRawF16) in place of the key
// transform and the u16 pair, which orders every bf16 pattern below 2^121
// in magnitude exactly as the keys do, so the result bits are the separate
// kernel's. A word of 2^121 or more, an infinity or a NaN makes its row's
// diagonal Gram entry non-finite (x^2 >= 2^242 overflows f32; diagonal
// products are never negative, so nothing cancels), and the launcher's
// second kernel (colsel_pk_median_bf16 with GUARD) then recomputes the
// whole median with the u16-key kernel: a finite diagonal proves that every
// word was legal. What is new against the separate kernel is that each lane
// also drops its raw loaded words into an LDS image, and the SAME wave runs
// the Gram MFMAs of its own columns from that image in the issue gaps of
// its own sort. X is read once.
//
// A wave works on strips of 64 rows x 128 columns (64 lanes x one column
// pair), and the strip's image is the wave's PRIVATE LDS slab: the wave
// accumulates the whole 64 x 64 Gram of its slab (upper triangle: 10 tiles
// of 16x16, 40 accumulator registers, v_mfma_f32_16x16x32_bf16 — the
// 32x32x16 form would take 48 registers and 768 matrix-pipe cycles per
// strip against 640), so no wave ever reads what another wave wrote and the
// strip loop has NO block barrier: the LDS serves one wave's operations in
// order, and a wave-scope fence keeps the compiler from moving the reads
// over the stores.
//
// Slab: [64 rows][256 B + 16 B pad] (MG_ROW_BYTES = 272, 17,408 B per wave,
// 69,632 B per block: two blocks per CU):
//  - store: lane l writes dword l of row i — one base VGPR plus an
//    immediate; 32 consecutive lanes hit 32 consecutive banks;
//  - fragment read: four k-steps of 32 per strip. ds_read_b128 is served in
//    four NON-contiguous 16-lane groups; with r = l & 15, q = l >> 4 a group
//    carries rows {0-3, 12-15} of one q and rows {4-11} of its neighbour
//    q ^ 1. A row holds only 16 slots of 16 B, so the two q of a group must
//    read different slots c, and with a 17-slot row stride the group's bank
//    quads are (row + c) mod 16. Rows 8-11 and 12-15 of every 16-row block
//    therefore swap places in the image (mg_phys_row): a group then holds
//    image rows {0-3, 8-11} of one q and {4-7, 12-15} of the other, and
//    slots that differ by 8 make the two sets tile all 16 bank quads. Lane
//    (r, q) reads slot 8 * (q & 1) + 4 * (q >> 1) + s in k-step s: over
//    q < 4, s < 4 all 16 slots once. A Gram sums over k, so which 8 columns
//    a (q, s) names is free as long as the A and B fragments agree — and
//    they are the same registers.
//
// A k-step is 4 ds_read_b128 (one fragment per 16-row block) + 10 MFMAs
// (blocks a <= b), spread through the selection network: each MFMA is
// followed by a run of the network's v_pk_min/max, so the matrix work sits
// in the VALU stream's issue gaps instead of a phase of its own. The places
// are fixed in the source (a hook in the network counts its ops, full
// scheduling barriers pin each event); a sched_group_barrier pipeline over
// the 890-op network was not honoured by the compiler.
//
// The next strip's 64 raw words are loaded into a second register set right
// after the current strip's words have been stored, so they stay in flight
// through the whole sort: at two waves per SIMD that prefetch, not
// occupancy, hides the HBM latency. The network sorts the loaded registers
// in place, so the two sets swap roles from strip to strip: the strip loop
// is unrolled by two with the sets exchanged, and no word is ever copied
// from one set to the other. The row walk is a
// wave-uniform base (strip start, advanced by the row stride on the scalar
// unit) plus one 32-bit per-lane byte offset below 1 KiB, so the loads are
// global_load_dword v, v, s[..] with no vector address arithmetic and no
// limit on the row length.
//
// Rows >= n and lanes past d / 2 put zeros in the image (their loads are
// clamped to valid addresses and nothing is stored for them).
//
// At large d strips are handed out, not split evenly: with an even static
// split the average wave was done after 75-85 % of the kernel's time and
// the slowest set it. Each wave starts on its own chunk of consecutive
// strips and draws every further chunk from a caller-zeroed ticket counter,
// one chunk ahead. Below median_gram_bf16_ticketed(d) there is no ticket
// and every wave takes one even share (profiles/r04_median_gram_wave.md has
// the sizes measured either way).
//
// At the end the four waves of a block park their partials in the (now
// free) slabs, one barrier, and every thread sums the four partials of 10
// entries and adds each into the caller-zeroed G at (i, j) and, off the
// diagonal blocks, (j, i): 4,096 atomics per block.
// ---------------------------------------------------------------------------

typedef __attribute__((ext_vector_type(8))) __bf16 mg_bf16x8;
typedef __attribute__((ext_vector_type(4))) float mg_f32x4;

constexpr int MG_THREADS = 256;
constexpr int MG_ROW_BYTES = 64 * 4 + 16;          // 272: one wave's row + pad
constexpr int MG_SLAB_BYTES = 64 * MG_ROW_BYTES;   // 17,408
constexpr int MG_LDS_BYTES = 4 * MG_SLAB_BYTES;    // 69,632
constexpr int MG_TILES = 10;                       // 16x16 blocks a <= b
constexpr int MG_CHUNK = 8;                        // strips per ticket draw

// image row of matrix row i: rows 8-11 and 12-15 of each 16-row block swap
constexpr int mg_phys_row(int i) {
  const int r = i & 15;
  return (i & ~15) | (r < 8 ? r : (r < 12 ? r + 4 : r - 4));
}

// index of block (a, b), a <= b, in the 10-tile upper triangle
constexpr int mg_tile(int a, int b) { return 4 * a - a * (a - 1) / 2 + (b - a); }

// pinned load walk of one strip's 64 row words (see colsel_reg_kernel's load
// phase): `base` is the strip's first pair in row 0 (wave-uniform), `off` the
// lane's clamped byte offset inside the strip, `rowbytes` the row stride
template <int P, bool FULL>
DEV void mg_load_tile(u32 (&r)[P], const char* base, u32 off, long rowbytes,
                      int n) {
  if (FULL) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      r[i] = *reinterpret_cast<const u32*>(base + off);
      if (i + 1 < P) base += rowbytes;
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
    // the walk stops at row n - 1; slots past it repeat that row and the
    // pad logic overwrites them. Per-lane pointer with a predicated step:
    // on the scalar unit the 63 chosen steps are loop-invariant, get
    // hoisted out of the strip loop into 126 SGPRs and spill
    const char* p = base + off;
    const int n_walk = vecify(n);
#pragma unroll
    for (int i = 0; i < P; ++i) {
      r[i] = *reinterpret_cast<const u32*>(p);
      p += (i + 1 < n_walk) ? rowbytes : 0;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// Where the Gram work of a strip sits in the selection network's packed ops
// (two half-sorts of 191 compare-exchanges, the 32 compare-exchanges of the
// split and its 2 x 31 reductions): k-step s starts at op MG_STEP * s with
// its 4 fragment reads, MG_LEAD ops cover their latency, then its 10 MFMAs
// follow MG_GAP ops apart. Events the network did not reach are issued
// right after it (see the kernel), so a shorter network costs speed, never
// a missing MFMA.
constexpr int MG_NET_OPS = 2 * (2 * 191) + 2 * 32 + 2 * 31;  // 890
constexpr int MG_STEP = 222, MG_LEAD = 32, MG_GAP = 19;
constexpr int MG_EVENTS = 4 * (1 + MG_TILES);
static_assert(3 * MG_STEP + MG_LEAD + (MG_TILES - 1) * MG_GAP <= MG_NET_OPS - 2,
              "the last MFMA must be due before the network's last group");

// Orders this wave's LDS accesses before the fence against those after it,
// for the compiler only: the LDS serves one wave's operations in order.
DEV void mg_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// FULL: n == 64 (no pad slots, no row clamp), chosen by the launcher so
// that each instantiation has ONE load walk: with both in one kernel the
// prefetched words reach the loop's end through 33 register copies.
template <bool FULL>
__global__ void __launch_bounds__(MG_THREADS, 2)
median_gram_bf16_kernel(const unsigned short* __restrict__ X,
                        unsigned short* __restrict__ out,
                        float* __restrict__ G, int n, long d, int chunk,
                        unsigned long long* __restrict__ ticket) {
  constexpr int P = 64;
  __shared__ __attribute__((aligned(16))) char img[MG_LDS_BYTES];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long npairs = d >> 1;
  // A wave's unit of work is a strip: 64 rows x 128 columns, the column
  // pairs [64 u, 64 u + 64). Strips go out in chunks of `chunk` consecutive
  // ones: wave g of the grid starts on chunk g, every later chunk comes off
  // the caller-zeroed ticket counter, drawn one chunk ahead so that the
  // atomic's round trip hides behind a chunk of work.
  const long nstrips = (npairs + 63) / 64;
  const long nwaves = (long)gridDim.x * (MG_THREADS / 64);
  auto draw = [&]() {
    if (ticket == nullptr) return 0x3fffffffffffffffL;  // even split: no more
    unsigned long long got = 0;
    if (lane == 0)
      got = __hip_atomic_fetch_add(ticket, (unsigned long long)chunk,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)got);
    const u32 hi = __builtin_amdgcn_readfirstlane((u32)(got >> 32));
    return nwaves * chunk + (long)(((unsigned long long)hi << 32) | lo);
  };
  long u = ((long)blockIdx.x * (MG_THREADS / 64) + wave) * chunk;
  long chunk_end = u + chunk;
  long next_chunk = draw();

  const char* Xb = reinterpret_cast<const char*>(X);
  u32* outw = reinterpret_cast<u32*>(out);
  const long rowbytes = npairs * 4;
  char* const slab = img + wave * MG_SLAB_BYTES;
  char* const wr = slab + 4 * lane;
  const int fr = lane & 15, fq = lane >> 4;
  const char* const rd = slab + mg_phys_row(fr) * MG_ROW_BYTES +
                         16 * (8 * (fq & 1) + 4 * (fq >> 1));

  mg_f32x4 acc[MG_TILES];
#pragma unroll
  for (int e = 0; e < MG_TILES; ++e) acc[e] = mg_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  const int nv = vecify(n);
  const int n_lo = vecify(selnet::median_pad_split<P>(n));

  // loads of strip s, per lane clamped to the row's last pair. A strip past
  // the end is never used: the wave reads `own` (in range) again instead,
  // its own strip and not the matrix's last one, where every wave of a
  // small call would meet.
  auto load_strip = [&](u32 (&dst)[P], long s, long own)
      __attribute__((always_inline)) {
    s = s < nstrips ? s : own;
    const u32 off = (u32)min((long)lane, npairs - 1 - s * 64) * 4u;
    mg_load_tile<P, FULL>(dst, Xb + s * 256, off, rowbytes, n);
  };

  // One strip: `v` holds strip u's 64 raw words on entry and is sorted in
  // place; `r` receives the next strip's words.
  auto strip = [&](u32 (&v)[P], u32 (&r)[P]) __attribute__((always_inline)) {
    const long pair = u * 64 + lane;
    const bool valid = pair < npairs;
    mg_wave_fence();  // the last strip's fragment reads stay above the stores
    // raw words into the slab
    if (FULL && (u + 1) * 64 <= npairs) {
#pragma unroll
      for (int i = 0; i < P; ++i)
        *reinterpret_cast<u32*>(wr + mg_phys_row(i) * MG_ROW_BYTES) = v[i];
    } else if (FULL) {
      // the matrix's last strip: every row is real, tail lanes are not
#pragma unroll
      for (int i = 0; i < P; ++i)
        *reinterpret_cast<u32*>(wr + mg_phys_row(i) * MG_ROW_BYTES) =
            valid ? v[i] : 0u;
    } else {
      const int n_img = valid ? nv : 0;
#pragma unroll
      for (int i = 0; i < P; ++i)
        *reinterpret_cast<u32*>(wr + mg_phys_row(i) * MG_ROW_BYTES) =
            (i < n_img) ? v[i] : 0u;
    }
    if (!FULL) {
      // slots [n, n_lo) pad low, [n_lo, P) pad high (n > P / 2 here). The
      // bounds go through opaque per-tile copies: hoisted out of the tile
      // loop, the 31 pad words and their masks would stay live through it
      // and spill
      int nv_t = nv, n_lo_t = n_lo;
      asm volatile("" : "+v"(nv_t), "+v"(n_lo_t));
#pragma unroll
      for (int i = P / 2 + 1; i < P; ++i) {
        if (i >= nv_t) v[i] = PK_RAW_PAD_LO;
        if (i >= n_lo_t) v[i] = PK_RAW_PAD_HI;
      }
    }
    // the next strip: the chunk's next one, or the first of the chunk drawn
    // a chunk ago (and then the draw for the one after)
    long u_next = u + 1;
    if (u_next == chunk_end) {
      u_next = next_chunk;
      chunk_end = next_chunk + chunk;
      next_chunk = draw();
    }
    // unconditional: behind a branch the 64 words come back through copies
    // at the loop's end
    load_strip(r, u_next, u);
    mg_wave_fence();  // the slab is complete for this wave's own reads

    // Gram of the slab inside the selection network. Event 11 * s + m is
    // k-step s's fragment reads (m == 0: one per 16-row block) or its MFMA
    // m - 1 (blocks a <= b); an event runs once the network has issued the
    // op count it is due at, and a full scheduling barrier on either side
    // pins that place (with one side open an MFMA floats up to its reads).
    // `ops` and `ev` are compile-time once the network unrolls.
    mg_bf16x8 f[4];
    int ops = 0, ev = 0;
    auto tick = [&](int k) __attribute__((always_inline)) {
      const int s = ev / (1 + MG_TILES), m = ev % (1 + MG_TILES);
      const int due =
          MG_STEP * s + (m == 0 ? 0 : MG_LEAD + MG_GAP * (m - 1));
      if (ev < MG_EVENTS && ops >= due) {
        __builtin_amdgcn_sched_barrier(0);
        if (m == 0) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            f[j] = *reinterpret_cast<const mg_bf16x8*>(
                rd + 16 * j * MG_ROW_BYTES + 16 * s);
        } else {
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a; b < 4; ++b)
              if (mg_tile(a, b) == m - 1)
                acc[mg_tile(a, b)] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    f[a], f[b], acc[mg_tile(a, b)], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        ++ev;
      }
      ops += k;
    };
    u32 lo, hi;
    selnet::median_network<P, PkRawF16>(v, lo, hi, tick);
    // whatever the network did not reach (nothing, with the constants above)
#pragma unroll
    for (int k = 0; k < MG_EVENTS; ++k) {
      ops = MG_NET_OPS * 4;
      tick(0);
    }
    // pins the network in this block: left alone it sinks, whole, into the
    // `valid` branch of the store below, away from the MFMAs
    asm volatile("" : "+v"(lo), "+v"(hi));

    // lo and hi are bf16 bits: a bf16 is the upper half of its f32
    if (n & 1) hi = lo;
    const float m0 =
        0.5f * (__uint_as_float(lo << 16) + __uint_as_float(hi << 16));
    const float m1 = 0.5f * (__uint_as_float(lo & 0xFFFF0000u) +
                             __uint_as_float(hi & 0xFFFF0000u));
    union { unsigned short s[2]; u32 w; } o;
    union { unsigned short s; __hip_bfloat16 h; } c0, c1;
    c0.h = __float2bfloat16(m0);
    c1.h = __float2bfloat16(m1);
    o.s[0] = c0.s;
    o.s[1] = c1.s;
    if (valid) outw[pair] = o.w;
    u = u_next;
  };

  // two register sets that swap roles: the set a strip was prefetched into
  // is the set it is sorted in
  u32 ra[P], rb[P];
  load_strip(ra, u, nstrips - 1);
  while (u < nstrips) {
    strip(ra, rb);
    if (!(u < nstrips)) break;
    strip(rb, ra);
  }

  // Block epilogue. Wave w parks register q of tile e at float
  // (4 * e + q) * 64 + lane of its own slab (its reads are done: the MFMAs
  // consumed them); after the barrier thread (w, lane) owns register w of
  // every tile. C/D map for 16x16: col = lane & 15, row = (lane >> 4) * 4 +
  // register.
  // The lane's coordinates are worked out again, from the lane counter and
  // not from the thread index: kept from the kernel's start they (or the
  // thread index) would hold, through the whole strip loop, registers that
  // the two word sets need (they spilled).
  const int ln =
      __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const int er = ln & 15, eq = ln >> 4;
  mg_wave_fence();
  float* const part = reinterpret_cast<float*>(slab) + ln;
#pragma unroll
  for (int e = 0; e < MG_TILES; ++e)
#pragma unroll
    for (int q = 0; q < 4; ++q) part[(4 * e + q) * 64] = acc[e][q];
  __syncthreads();
  const float* const sum =
      reinterpret_cast<const float*>(img) + wave * 64 + ln;
  const float* const mirror = reinterpret_cast<const float*>(img) +
                              (er & 3) * 64 + 16 * (er >> 2) + 4 * eq + wave;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = a; b < 4; ++b) {
      float g = 0.0f;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        g += sum[w * (MG_SLAB_BYTES / 4) + 4 * mg_tile(a, b) * 64];
      const int row = 16 * a + (ln >> 4) * 4 + wave;
      const int col = 16 * b + (ln & 15);
      if (row < n && col < n) atomicAdd(&G[(long)row * n + col], g);
      if (a != b) {
        // the mirror image, with the lanes along G's rows again: this
        // thread takes tile element (er, 4 * eq + wave), which sits in
        // register er & 3 of lane 16 * (er >> 2) + 4 * eq + wave. Written
        // from `g` above the 16 lanes of a row group would hit 16 cache
        // lines, and the atomics are what a small call spends its time on.
        float gt = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w)
          gt += mirror[w * (MG_SLAB_BYTES / 4) + 4 * mg_tile(a, b) * 64];
        const int mrow = 16 * b + 4 * eq + wave;
        const int mcol = 16 * a + er;
        if (mrow < n && mcol < n) atomicAdd(&G[(long)mrow * n + mcol], gt);
      }
    }
}

// (the specialized 2-pass 256-bin bf16 median radix kernels that lived
// here were retired: the generic 64-bin engine in rsel.hip runs the same
// selection in 3 passes at 32 waves/CU and measures 2x faster)

// ---------------------------------------------------------------------------
// LDS variant, 64 < n <= 512: block-COOPERATIVE batched bitonic. One block
// (16 waves) owns 64 columns staged as an LDS plane [P][64]; every
// compare-exchange step spreads its P/2 x 64 sites over all 1024 threads
// (adjacent threads take adjacent columns of one site -> adjacent banks,
// conflict-free), with a block barrier between j-substeps. Replaces the
// original one-wave-per-block version whose single wave left the CU 97%
// idle (n=512 d=1M: 91.7 -> ~1 ms).
// ---------------------------------------------------------------------------

constexpr int LDS_COLS = 64;
// 512 threads (8 waves): halves barrier cost vs 16 waves and lets 2-4
// blocks co-reside per CU at small P (LDS is the binding resource at
// P=512: 128 KB -> 1 block)
constexpr int LDS_THREADS = 512;

template <int MODE, typename T, bool ROWS>
__global__ void __launch_bounds__(LDS_THREADS)
colsel_lds_kernel(const T* __restrict__ X, T* __restrict__ out,
                  int n, long d, int f, int P,
                  const int* __restrict__ rows, int n_src) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* buf = reinterpret_cast<float*>(smem);  // [P][LDS_COLS]
  const int t = threadIdx.x;
  const long col0 = (long)blockIdx.x * LDS_COLS;
  const int cols = (int)min((long)LDS_COLS, d - col0);

  // cooperative stage: element (row, c) by thread index
  for (int idx = t; idx < P * LDS_COLS; idx += LDS_THREADS) {
    const int row = idx / LDS_COLS;
    const int c = idx % LDS_COLS;
    float v = PAD;
    if (row < n && c < cols) {
      int src = row;
      if (ROWS) {
        // the 64 idx of one wave iteration share `row` (LDS_COLS == 64):
        // readfirstlane makes that provable, so rows[row] is one scalar
        // load per wave and the row offset stays in SGPRs
        const int r = rows[__builtin_amdgcn_readfirstlane(row)];
        src = min(max(r, 0), n_src - 1);
      }
      v = to_f<T>(X[(long)src * d + col0 + c]);
    }
    buf[idx] = v;
  }
  __syncthreads();

  // batched bitonic: P/2 compare sites x LDS_COLS columns per substep.
  // j is always a power of two, so the site decomposition is pure shifts
  // (an integer division per site per substage dominated this kernel).
  for (int k = 2; k <= P; k <<= 1) {
    for (int jl = 31 - __clz(k >> 1); jl >= 0; --jl) {
      const int j = 1 << jl;
      const int k_ = k;
      for (int idx = t; idx < (P >> 1) * LDS_COLS; idx += LDS_THREADS) {
        const int site = idx >> 6;          // LDS_COLS == 64
        const int c = idx & 63;
        // site s enumerates pairs (i, i^j) with i^j > i:
        // i = (s >> jl) << (jl+1) | (s & (j-1))
        const int i = ((site >> jl) << (jl + 1)) | (site & (j - 1));
        const int l = i ^ j;
        const bool asc = (i & k_) == 0;
        float* a = &buf[i * LDS_COLS + c];
        float* b = &buf[l * LDS_COLS + c];
        const float av = *a, bv = *b;
        const float lo = fminf(av, bv), hi = fmaxf(av, bv);
        *a = asc ? lo : hi;
        *b = asc ? hi : lo;
      }
      __syncthreads();
    }
  }

  // per-column epilogue: threads 0..cols-1
  if (t < cols) {
    float* mine = buf + t;
    const int stride = LDS_COLS;
    const float med =
        0.5f * (mine[((n - 1) >> 1) * stride] + mine[(n >> 1) * stride]);
    float result;
    if (MODE == MEDIAN) {
      result = med;
    } else if (MODE == TRIMMED) {
      float s = 0.0f;
      for (int i2 = f; i2 < n - f; ++i2) s += mine[i2 * stride];
      result = s / (float)(n - 2 * f);
    } else {  // MEAMED: contiguous window of the sorted column (two-pointer)
      int l = 0, r = n;
      for (int kk = 0; kk < f; ++kk) {
        const float dl = med - mine[l * stride];
        const float dr = mine[(r - 1) * stride] - med;
        if (dl > dr) ++l; else --r;
      }
      float s = 0.0f;
      for (int i2 = l; i2 < r; ++i2) s += mine[i2 * stride];
      result = s / (float)(n - f);
    }
    out[col0 + t] = from_f<T>(result);
  }
}

// ---------------------------------------------------------------------------
// Coordinate-wise tailored attack objective (n <= 64): for each of 32 trial
// gammas, D_t = sum_j (mu_j - A_j(gamma_t))^2, where A_j is the median or the
// f-trimmed mean of column j's n honest values plus f copies of
// v = mu_j + gamma_t p_j. One pass over X for all trials: the honest column
// is sorted ONCE in registers, ascending with +inf pads (s_1 <= .. <= s_n,
// 1-based below), and a trial never sorts again.
//
//  - rank k of the attacked column is v clamped between two honest order
//    statistics, max(s_{k-f}, min(v, s_k)) with s_i = -inf below 1 and +inf
//    past n: the median (M = 0) reads two (odd n + f) or four of them per
//    column and clamps per trial.
//  - the trimmed mean (M > 0) keeps honest rank i iff
//    (s_i < v ? i > f : i <= n - f). With m = min(f, n - f): ranks
//    f < i <= n - f are always kept (summed once per column, in f64), ranks
//    n - f < i <= f never, rank i <= m iff !(s_i < v), rank i > n - m iff
//    s_i < v; the copies of v fill the n - f kept slots that the honest
//    values leave. Per trial that is 2 M compare-selects, M >= m the
//    kernel's tail width (a template argument: 4, 8, 16 or 32). Both tails
//    are read at compile-time indices: the low one is v[0 .. m) as sorted,
//    the high one comes top-aligned out of a barrel shift by P - n (six
//    wave-uniform conditional moves of the array, none taken at n == P);
//    slots m .. M hold -inf (low) and +inf (high), which no v keeps: the
//    compares see v raised to -FLT_MAX at least (below). The trial loop is
//    straight-line code with no wave-uniform guard in it: 32 x 2 M
//    loop-invariant conditions would be hoisted into scalar mask pairs and
//    spill.
//
// Values that are not finite follow the order torch.sort gives them, which
// is what the oracle and the torch composition see: a NaN ranks above +inf.
// A NaN in X is loaded as +inf (the min/max network would drop it), a NaN v
// compares as +inf, and v = -inf (or an f64 v below the f32 range) compares
// as -FLT_MAX, which ranks it below every finite value and level with an
// honest -inf, whose place in the sum it takes with the same value. The
// kept copies enter the sum as count x v in f64 with v as it is, so a kept
// NaN or infinite copy makes D non-finite, and a dropped one does not.
//
// v, the clamp, the sum of the kept values and mu - A are f64 (the tails'
// partial sums f32); (mu - A)^2 goes into one f64 accumulator per trial and
// thread, 64 VGPRs that live through the whole column loop next to the 64
// sort registers: the kernel is built for 2 waves per SIMD (256 VGPRs).
// Reduction, the same bits on every run: lanes by shuffle, the block's four
// waves through LDS in wave order, one f64 partial per (block, trial);
// coord_objective_finish adds the blocks in index order. No atomics.
// ---------------------------------------------------------------------------

constexpr int COORD_THREADS = 256;
constexpr int COORD_T = COORD_MAX_TRIALS;

// sorted[idx] of the n real values for a runtime idx that may fall outside:
// -inf below 0, +inf from n on (the pads of the sorted array, or past it)
template <int P>
DEV float coord_rank(const float (&v)[P], int idx) {
  float r = idx < 0 ? -PAD : PAD;
#pragma unroll
  for (int i = 0; i < P; ++i)
    if (i == idx) r = v[i];
  return r;
}

DEV double coord_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

// gammas holds ntrials <= COORD_T values; the trials past them repeat the
// last one and coord_objective_finish drops their sums
template <int P, int M, typename T>
__global__ void __launch_bounds__(COORD_THREADS, 2)
coord_objective_kernel(const T* __restrict__ X, const float* __restrict__ mu,
                       const float* __restrict__ p,
                       const float* __restrict__ gammas,
                       double* __restrict__ part, int n, long d, int f,
                       int ntrials) {
  double acc[COORD_T];
#pragma unroll
  for (int t = 0; t < COORD_T; ++t) acc[t] = 0.0;
  // the trial values, padded to COORD_T with the last one, staged once
  __shared__ float gam[COORD_T];
  if (threadIdx.x < COORD_T)
    gam[threadIdx.x] = gammas[min((int)threadIdx.x, ntrials - 1)];
  __syncthreads();

  const double inv_kept = 1.0 / (double)(n - f);
  const long col0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long col = col0; col < d; col += stride) {
    float v[P];
    T raw[P];
    // pinned raw-load walk: see colsel_reg_kernel's load phase
    const T* xp = X + col;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      raw[i] = *xp;
      if (i + 1 < n) xp += d;
      __builtin_amdgcn_sched_barrier(0);
    }
    const float muc = mu[col], pc = p[col];
    const int nv = vecify(n);
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const float x = to_f<T>(raw[i]);
      v[i] = x == x ? x : PAD;  // NaN ranks last, as in torch.sort
    }
    if (n < P) {
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (i >= nv) v[i] = PAD;
    }
    // Batcher's network over all P slots (selnet's half_sort sorts whatever
    // array it is given: 543 compare-exchanges at P = 64, bitonic 672)
    selnet::half_sort<P, true, F32MinMax>(v);
    const double mud = (double)muc, pd = (double)pc;
    // opaque per column: the 32 LDS reads stay in the loop instead of
    // holding 32 (converted: 64) registers through it
    int g0 = 0;
    asm volatile("" : "+v"(g0));

    if constexpr (M == 0) {
      // 0-based positions q1 <= q2 of the attacked column's middles; position
      // q lies between honest sorted[q - f] and sorted[q]
      const int q1 = (n + f - 1) >> 1, q2 = (n + f) >> 1;
      const double lo1 = (double)coord_rank<P>(v, vecify(q1 - f));
      const double hi1 = (double)coord_rank<P>(v, vecify(q1));
      const double lo2 = (double)coord_rank<P>(v, vecify(q2 - f));
      const double hi2 = (double)coord_rank<P>(v, vecify(q2));
#pragma unroll
      for (int t = 0; t < COORD_T; ++t) {
        const double vt = fma((double)gam[g0 + t], pd, mud);
        const double c1 = fmax(lo1, fmin(vt, hi1));
        const double c2 = fmax(lo2, fmin(vt, hi2));
        // q1 == q2 (odd n + f): c1 == c2 and the mean is c1, exactly
        const double diff = mud - (c1 + c2) * 0.5;
        acc[t] = fma(diff, diff, acc[t]);
      }
    } else {
      // always-kept middle, 0-based [f, n - f) (empty for 2f >= n)
      const int fv = vecify(f), nfv = vecify(n - f);
      double mid = 0.0;
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (i >= fv && i < nfv) mid += (double)v[i];
      const int mv = vecify(min(f, n - f));  // ranks per tail, <= M
      float lo[M], hi[M];  // lo[j] = s_{1+j}, hi[j] = s_{n-j}, j < m
#pragma unroll
      for (int j = 0; j < M; ++j) lo[j] = j < mv ? v[j] : -PAD;
      const int sh = P - n;
#pragma unroll
      for (int b = 1; b < P; b <<= 1) {
        if (sh & b) {
#pragma unroll
          for (int i = P - 1; i >= b; --i) v[i] = v[i - b];
        }
      }
#pragma unroll
      for (int j = 0; j < M; ++j) hi[j] = j < mv ? v[P - 1 - j] : PAD;
#pragma unroll
      for (int t = 0; t < COORD_T; ++t) {
        const double vt = fma((double)gam[g0 + t], pd, mud);
        // v as the compares see it: NaN as +inf, nothing below -FLT_MAX
        // (the pads stay inert for every v; see the header)
        const float vr = (float)vt;
        const float vf = vr == vr ? fmaxf(vr, -__FLT_MAX__) : PAD;
        float tail = 0.0f;
        int honest = 0;  // kept tail values
#pragma unroll
        for (int j = 0; j < M; ++j) {
          // selects, not products with a 0/1 mask: 0 * inf is NaN. (Rank
          // 1 + j and rank n - j could share one v_med3_f32(lo, v, hi), but
          // the copies of v would then add up in f32: count x v in f64
          // keeps a single column's mu - A within the tests' bound.)
          const bool kl = !(lo[j] < vf);
          const bool kh = hi[j] < vf;
          tail += kl ? lo[j] : 0.0f;
          tail += kh ? hi[j] : 0.0f;
          honest += (kl ? 1 : 0) + (kh ? 1 : 0);
        }
        // the n - f kept slots hold the middle's max(n - 2f, 0) values, the
        // kept tail values and, for the rest, copies of v
        const int copies = mv - honest;
        const double vsum = copies > 0 ? (double)copies * vt : 0.0;
        const double diff = mud - (mid + (double)tail + vsum) * inv_kept;
        acc[t] = fma(diff, diff, acc[t]);
      }
    }
  }

  __shared__ double wsum[COORD_THREADS / 64][COORD_T];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < COORD_T; ++t) {
    const double s = coord_wave_sum(acc[t]);
    if (lane == 0) wsum[wave][t] = s;
  }
  __syncthreads();
  if (threadIdx.x < COORD_T) {
    double s = wsum[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < COORD_THREADS / 64; ++w) s += wsum[w][threadIdx.x];
    part[(long)blockIdx.x * COORD_T + threadIdx.x] = s;
  }
}

// out[t] = part[0][t] + part[1][t] + ... in block order; one thread per trial
__global__ void coord_objective_finish(const double* __restrict__ part,
                                       double* __restrict__ out, int nblocks,
                                       int ntrials) {
  const int t = threadIdx.x;
  if (t >= ntrials) return;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += part[(long)b * COORD_T + t];
  out[t] = s;
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

// plain (rows == nullptr) or row-indexed kernel variant:
// fn receives std::bool_constant<ROWS>
template <typename F>
inline void by_rows(const int* rows, F&& fn) {
  if (rows != nullptr) fn(std::true_type{});
  else fn(std::false_type{});
}

// grid-stride launch width: one unit per thread, capped at 8192 blocks
inline int capped_grid(long units, int block) {
  const long want = (units + block - 1) / block;
  return (int)(want < 8192 ? (want > 0 ? want : 1) : 8192);
}

}  // namespace

// ---------------------------------------------------------------------------
// host-side launch (called from bind.cpp)
// ---------------------------------------------------------------------------

template <typename T>
static void colsel_generic(const T* X, T* out, int n, long d, int mode, int f,
                           const int* rows, int n_src, hipStream_t stream) {
  by_mode(mode, [&](auto m) {
    constexpr int MODE = decltype(m)::value;
    by_rows(rows, [&](auto r) {
      constexpr bool ROWS = decltype(r)::value;
      if (n <= 64) {
        const int block = 256;
        const int grid = capped_grid(d, block);
        by_reg_width(n, [&](auto p) {
          hipLaunchKernelGGL(
              (colsel_reg_kernel<decltype(p)::value, MODE, T, ROWS>),
              dim3(grid), dim3(block), 0, stream, X, out, n, d, f, rows,
              n_src);
        });
      } else {
        int P = 128;
        while (P < n) P <<= 1;  // 128/256/512
        const long grid = (d + LDS_COLS - 1) / LDS_COLS;
        const size_t lds = (size_t)P * LDS_COLS * sizeof(float);
        hipLaunchKernelGGL((colsel_lds_kernel<MODE, T, ROWS>), dim3(grid),
                           dim3(LDS_THREADS), lds, stream, X, out, n, d, f, P,
                           rows, n_src);
      }
    });
  });
}

template <>
void launch_colsel<float>(const float* X, float* out, int n, long d, int mode,
                          int f, const int* rows, int n_src,
                          hipStream_t stream) {
  colsel_generic(X, out, n, d, mode, f, rows, n_src, stream);
}

// bf16 with n <= 64 and even d takes the packed path (two columns per lane)
template <>
void launch_colsel<__hip_bfloat16>(const __hip_bfloat16* X,
                                   __hip_bfloat16* out, int n, long d,
                                   int mode, int f, const int* rows,
                                   int n_src, hipStream_t stream) {
  if (n <= 64 && (d % 2) == 0) {
    const int block = 256;
    const int grid = capped_grid(d >> 1, block);
    const unsigned short* Xu = reinterpret_cast<const unsigned short*>(X);
    unsigned short* Ou = reinterpret_cast<unsigned short*>(out);
    by_mode(mode, [&](auto m) {
      constexpr int MODE = decltype(m)::value;
      // MEAMED stages a 2(f+1)-key strip per thread in LDS (odd stride)
      const size_t lds =
          MODE == MEAMED ? (size_t)block * (2 * (f + 1) + 1) * sizeof(u32) : 0;
      by_rows(rows, [&](auto r) {
        constexpr bool ROWS = decltype(r)::value;
        by_reg_width(n, [&](auto p) {
          hipLaunchKernelGGL(
              (colsel_pk_median_bf16<decltype(p)::value, MODE, ROWS>),
              dim3(grid), dim3(block), lds, stream, Xu, Ou, n, d, f, rows,
              n_src, (const float*)nullptr);
        });
      });
    });
    return;
  }
  colsel_generic(X, out, n, d, mode, f, rows, n_src, stream);
}

// Persistent grid: two blocks per CU (what the 69,632 B of slabs admit);
// the waves draw their strips in chunks from `ticket`.
void launch_median_gram_bf16(const __hip_bfloat16* X, __hip_bfloat16* med,
                             float* G, unsigned long long* ticket, int n,
                             long d, hipStream_t stream) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess ||
      cus < 1)
    cus = 256;
  const long nstrips = ((d >> 1) + 63) / 64;
  const long want = 2L * cus;
  const long need = (nstrips + 3) / 4;
  const long blocks = need < want ? need : want;
  // With a ticket: chunks of MG_CHUNK strips (the draws all hit one address
  // and cost ~20 ns each in a row, so they must stay far apart). Without:
  // an even split, one chunk per wave.
  const long nwaves = 4 * blocks;
  const int chunk =
      ticket != nullptr ? MG_CHUNK : (int)((nstrips + nwaves - 1) / nwaves);
  hipLaunchKernelGGL(n == 64 ? median_gram_bf16_kernel<true>
                             : median_gram_bf16_kernel<false>,
                     dim3((unsigned)blocks), dim3(MG_THREADS), 0, stream,
                     reinterpret_cast<const unsigned short*>(X),
                     reinterpret_cast<unsigned short*>(med), G, n, d, chunk,
                     ticket);
  // The fused kernel's network is only right for words below 2^121 in
  // magnitude; G's diagonal tells (see the kernel's header). Next on the
  // stream, no host sync: the u16-key median over all of X into `med`,
  // which every wave leaves at once when the diagonal is finite. The grid
  // is capped at four blocks per CU and strides, so that the launch that
  // has nothing to do costs a few microseconds.
  const long gwant = (long)capped_grid(d >> 1, 256);
  const long gcap = 4L * cus;
  hipLaunchKernelGGL((colsel_pk_median_bf16<64, MEDIAN, false, true>),
                     dim3((unsigned)(gwant < gcap ? gwant : gcap)), dim3(256),
                     0, stream, reinterpret_cast<const unsigned short*>(X),
                     reinterpret_cast<unsigned short*>(med), n, d, 0,
                     (const int*)nullptr, 0, (const float*)G);
}

// One objective launch plus the block-order sum. `part` holds
// coord_objective_blocks(d) * COORD_MAX_TRIALS doubles of scratch. The
// trimmed mean runs the narrowest tail width M in {4, 8, 16, 32} that holds
// its min(f, n - f) <= n / 2 <= P / 2 ranks, and never one past P / 2.
template <typename T>
void launch_coord_objective(const T* X, const float* mu, const float* p,
                            const float* gammas, double* part, double* out,
                            int n, long d, int mode, int f, int ntrials,
                            hipStream_t stream) {
  const int blocks = coord_objective_blocks(d);
  const int m = f < n - f ? f : n - f;
  by_reg_width(n, [&](auto pw) {
    constexpr int P = decltype(pw)::value;
    auto go = [&](auto mw) {
      constexpr int M = decltype(mw)::value <= P / 2 ? decltype(mw)::value : P / 2;
      hipLaunchKernelGGL((coord_objective_kernel<P, M, T>), dim3(blocks),
                         dim3(COORD_THREADS), 0, stream, X, mu, p, gammas,
                         part, n, d, f, ntrials);
    };
    if (mode == MEDIAN) go(std::integral_constant<int, 0>{});
    else if (m <= 4) go(std::integral_constant<int, 4>{});
    else if (m <= 8) go(std::integral_constant<int, 8>{});
    else if (m <= 16) go(std::integral_constant<int, 16>{});
    else go(std::integral_constant<int, 32>{});
  });
  hipLaunchKernelGGL(coord_objective_finish, dim3(1), dim3(64), 0, stream,
                     (const double*)part, out, blocks, ntrials);
}
INSTANTIATE_LAUNCHER(launch_coord_objective)
