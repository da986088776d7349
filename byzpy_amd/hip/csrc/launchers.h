// Host launchers of the byzpy_amd gfx950 kernel library: the one place a
// launcher signature is declared. Included by bind.cpp and by every .hip
// file that defines one, so a signature drift fails to compile instead of
// surfacing as an undefined symbol when _hip_ops.so is imported.
//
// Every launch_x<T> is defined for T in {float, __hip_bfloat16}, explicitly
// instantiated next to its definition (INSTANTIATE_LAUNCHER, one block per
// file). All launches enqueue on `stream`; none syncs the host.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

// Row cap of the kernels that stage per-row weights in LDS
// (weiszfeld_update, cc_update, caf_colsum in rowops.hip). The bindings
// reject larger n before launching; the kernels size their arrays by it.
constexpr int MAX_N_LDS = 1024;

// `template void f<T>(full signature)` without repeating the signature
#define INSTANTIATE_LAUNCHER(f)           \
  template decltype(f<float>) f<float>;   \
  template decltype(f<__hip_bfloat16>) f<__hip_bfloat16>;

// colsel.hip: register / LDS-sort column selection, n <= 512.
// mode: 0 median, 1 trimmed mean, 2 mean-around-median.
// `rows` null: the statistic runs over rows 0..n-1 of the (n, d) matrix.
// `rows` non-null: an int32 device vector of n distinct row indices into an
// (n_src, d) matrix; the statistic runs over exactly those rows, as if on
// X[rows], with no gather (n <= COLSEL_MAX_ROWS counts the selected rows,
// n_src is unbounded; indices are clamped to [0, n_src)).
constexpr int COLSEL_MAX_ROWS = 512;
template <typename T>
void launch_colsel(const T* X, T* out, int n, long d, int mode, int f,
                   const int* rows, int n_src, hipStream_t stream);

// colsel.hip: column median and Gram X X^T in one pass over X. bf16 only;
// `med` receives what launch_colsel(mode 0) writes, bit for bit, and the
// partial Grams are ADDED into the caller-zeroed (n, n) G. Call it only
// where median_gram_bf16_applies(n, d). Two launches on `stream`: the fused
// kernel, whose median is right when every |x| < 2^121, and a guard that
// reads G's diagonal on the device and, if any entry is not finite, runs
// launch_colsel's median kernel over X into `med` (else it returns at
// once). G must therefore be this call's own Gram, not yet reduced with
// anyone else's.
inline bool median_gram_bf16_applies(long n, long d) {
  return n > 32 && n <= 64 && d >= 2 && (d % 2) == 0;
}
// `ticket` is one caller-zeroed 64-bit device word (the kernel's work
// counter) where median_gram_bf16_ticketed(d), else null: from 2^18 strips
// of 128 columns up the waves draw their work instead of splitting it evenly.
inline bool median_gram_bf16_ticketed(long d) { return d >= (1L << 25); }
void launch_median_gram_bf16(const __hip_bfloat16* X, __hip_bfloat16* med,
                             float* G, unsigned long long* ticket, int n,
                             long d, hipStream_t stream);

// colsel.hip: objective of the coordinate-wise tailored attack. For each of
// the ntrials values of gammas, out[t] = sum_j (mu_j - A_j)^2 in f64, A_j the
// median (mode 0) or f-trimmed mean (mode 1) of column j's n honest values
// plus f copies of mu_j + gammas[t] p_j. 1 <= n <= COORD_MAX_N, 1 <= ntrials
// <= COORD_MAX_TRIALS, f >= 1 and f < n in mode 1. One pass over X; the grid
// is capped and strides, each block leaves one f64 partial per trial in
// `part` (coord_objective_blocks(d) * COORD_MAX_TRIALS doubles of scratch)
// and a second launch adds them in block order: bitwise repeatable, no
// atomics. Non-finite values rank as torch.sort ranks them (NaN last).
constexpr int COORD_MAX_N = 64;
constexpr int COORD_MAX_TRIALS = 32;
constexpr int COORD_MAX_BLOCKS = 1024;  // of 256 columns a trip
inline int coord_objective_blocks(long d) {
  const long want = (d + 255) / 256;
  return (int)(want < COORD_MAX_BLOCKS ? (want > 0 ? want : 1)
                                       : COORD_MAX_BLOCKS);
}
template <typename T>
void launch_coord_objective(const T* X, const float* mu, const float* p,
                            const float* gammas, double* part, double* out,
                            int n, long d, int mode, int f, int ntrials,
                            hipStream_t stream);

// rsel.hip: streaming radix-select engine for large n, same modes.
// `state` is caller-zeroed d*4 u32 scratch; `med` is a d-float scratch,
// read only by mode 2 (may be null otherwise)
template <typename T>
void launch_rsel(int mode, const T* X, T* out, unsigned int* state, float* med,
                 int n, long d, int f, hipStream_t stream);

// gram.hip
template <typename T>
void launch_gram(const T* X, float* G, int n, long d, hipStream_t stream);

// gram.hip / subsets.hip (K15, DnC). Row cap of both DnC kernels: the Gram
// kernel's register blocks and the selection kernel's register-resident
// matrix are sized by it.
constexpr int DNC_MAX_N = 128;
// A sampled entry counts as finite up to this magnitude (2^48): past it the
// squares would overflow the f32 Gram, so the row is flagged bad like one
// holding inf or NaN.
constexpr float DNC_MAX_ABS = 281474976710656.0f;
// Column chunking of launch_gram_sampled: tiles of 64 columns, grouped so
// that nchunks * niters stays near one block per CU. The caller sizes the
// partial buffers with it.
inline void dnc_gram_chunks(int b, int niters, int& nchunks,
                            int& tiles_per_chunk) {
  const int ntiles = (b + 63) / 64;
  int want = 256 / (niters < 1 ? 1 : niters);
  if (want < 1) want = 1;
  tiles_per_chunk = (ntiles + want - 1) / want;
  nchunks = (ntiles + tiles_per_chunk - 1) / tiles_per_chunk;
}
// Per iteration t < niters: Gc[t] = C C^T (n, n) f32 of the sample
// X[:, cols[t]] (cols: int32 (niters, b), clamped to [0, d)), C centred per
// column by the mean of its finite entries, non-finite entries 0;
// bad[t][i] = 1 where row i holds a non-finite sampled entry. part / badpart
// are nchunks * niters * n * n floats / * n ints of scratch; the partials
// are added in chunk order (bitwise repeatable). n <= DNC_MAX_N.
template <typename T>
void launch_gram_sampled(const T* X, const int* cols, int n, long d,
                         int niters, int b, float* part, int* badpart,
                         float* Gc, int* bad, hipStream_t stream);
// Spectral selection on those Grams: per iteration a fixed-count power
// iteration for the top eigenvector u, score_i = u_i^2 (+inf for bad rows),
// kept_t = the `keep` lowest scores (ties to the smaller index) minus the
// bad rows; idx receives the ascending indices of the intersection over t,
// padded with 0 to n entries, count their number. kept is niters * n ints
// of scratch. n <= DNC_MAX_N, 1 <= keep <= n.
void launch_dnc_select(const float* Gc, const int* bad, int niters, int n,
                       int keep, int* kept, int* idx, int* count,
                       hipStream_t stream);

// subsets.hip (K16, AFA). Row cap of the selection kernel: one thread per
// (16-entry row segment, row) of the Gram.
constexpr int AFA_MAX_N = 128;
// The whole AFA loop on the f32 Gram G (n, n) with row weights w (n,), one
// block: rows with a non-finite G_ii or a weight that is not a positive
// finite number start dead; each pass drops the alive rows whose cosine to
// the weighted mean of the alive rows lies past med -/+ xi sd (the side
// chosen by mean < med), xi += delta_xi after a pass that dropped a row, and
// the first pass that drops none ends it. idx receives the ascending alive
// indices padded with 0 to n entries, count their number, rounds the number
// of passes. 1 <= n <= AFA_MAX_N.
void launch_afa_select(const float* G, const float* w, int n, double xi,
                       double delta_xi, int* idx, int* count, int* rounds,
                       hipStream_t stream);

// rowops.hip
template <typename T>
void launch_row_sqnorms(const T* X, float* out, int n, long d,
                        hipStream_t stream);
template <typename T>
void launch_row_center_sqdists(const T* X, const float* z, float* out, int n,
                               long d, hipStream_t stream);
template <typename T>
void launch_row_scale(const T* X, const float* s, T* out, int n, long d,
                      hipStream_t stream);
template <typename T>
void launch_mean_rows(const T* X, const int* idx, int k, T* out, long d,
                      hipStream_t stream);
// The mean of rows idx[0 .. *count) with the count read on device (clamped
// to [0, k]); zeros when it is 0. Entries of idx past the count are not read.
template <typename T>
void launch_mean_rows_counted(const T* X, const int* idx, int k,
                              const int* count, T* out, long d,
                              hipStream_t stream);
// The same with row weights: sum_i w[idx[i]] x[idx[i]] / sum_i w[idx[i]] over
// i < *count; zeros when the count or the weight sum is 0. X and w have
// n_src rows (idx is clamped to them); k <= MAX_N_LDS (the weights are
// staged in LDS).
template <typename T>
void launch_mean_rows_counted_weighted(const T* X, const int* idx, int k,
                                       const int* count, const float* w,
                                       int n_src, T* out, long d,
                                       hipStream_t stream);
template <typename T>
void launch_group_mean_rows(const T* X, const int* idx, int g, int k, T* out,
                            long d, hipStream_t stream);
template <typename T>
void launch_bucket_mean(const T* X, const int* perm, int n, int bucket, int nb,
                        T* out, long d, hipStream_t stream);
template <typename T>
void launch_weiszfeld_update(const T* X, const float* z, const float* dist2,
                             float* z_new, float* shift2, int n, long d,
                             float eps, hipStream_t stream);
template <typename T>
void launch_grouped_weiszfeld(const T* X, const float* Z, float* dist2,
                              float* Z_new, int G, int m, long d, float eps,
                              hipStream_t stream);
template <typename T>
void launch_cc_update(const T* X, const float* v, const float* dist2,
                      float* v_new, int n, long d, float c_tau, float eps,
                      hipStream_t stream);
template <typename T>
void launch_caf_matvec(const T* X, const float* mu, const float* v, float* out,
                       int n, long d, hipStream_t stream);
template <typename T>
void launch_caf_colsum(const T* X, const float* a, const float* mu,
                       const float* scale, float* out, int n, long d,
                       hipStream_t stream);

// attacks.hip (K14)
template <typename T>
void launch_little(const T* X, T* out, int n, long d, float z,
                   hipStream_t stream);
// Min-Max / Min-Sum statistics. perturb: 0 unit (p = -mu, unnormalised),
// 1 std (p = -sigma, population), 2 sign (p = -sign(mu)). Writes the f32
// d-vectors mu and p and ADDS into the caller-zeroed 2n + 1 floats
// stats = [a_0..a_{n-1}, b_0..b_{n-1}, c] with a_i = ||mu - x_i||^2,
// b_i = p . (mu - x_i), c = ||p||^2. n <= 64 is one fused pass; larger n is
// a moments pass plus row_center_sqdists and caf_matvec, n <= MAX_N_LDS
// (its sigma is sqrt(sum x^2 / n - mu^2), the fused pass's the root mean
// squared deviation: they differ where |mu| >> sigma cancels in f32).
template <typename T>
void launch_attack_stats(const T* X, float* mu, float* p, float* stats, int n,
                         long d, int perturb, hipStream_t stream);
template <typename T>
void launch_gaussian_fill(T* out, long d, unsigned long long seed, float mu,
                          float sigma, hipStream_t stream);

// krumsel.hip / subsets.hip (K11): f32 Gram / distance matrices only
void launch_krum_select(const float* G, int n, int f, int q, int* out_idx,
                        float* out_scores, hipStream_t stream);
// Iterative (Bulyan) selection: q picks in one launch, each the best Krum
// score among the rows still alive (k = alive - f - 1 nearest alive rows),
// the pick then leaves the pool; out_idx holds the picks in order. Needs
// n - q - f >= 1. The per-row sorted distance lists live in LDS, which
// caps n at KRUM_ITER_MAX_N.
constexpr int KRUM_ITER_MAX_N = 128;
void launch_krum_select_iter(const float* G, int n, int f, int q,
                             int* out_idx, hipStream_t stream);
// Aggregator-tailored attack search: n honest rows (their f32 Gram G and the
// 2n + 1 Min-Max statistics of launch_attack_stats), f >= 1 copies of
// m(gamma) = mu + gamma p appended, the rule run on the n + f rows with
// parameter f. rule AGR_RULE_KRUM: Krum / Multi-Krum with q winners;
// AGR_RULE_BULYAN: the iterated selection above (q unused). One workgroup
// per trial gamma. Needs n >= 2, f <= n, n + f <= KRUM_ITER_MAX_N, and
// n >= 3f + 3 for Bulyan.
constexpr int AGR_RULE_KRUM = 0;
constexpr int AGR_RULE_BULYAN = 1;
// flags[k] = 1 where gammas[k] is feasible, k < B.
void launch_agr_flags(const float* G, const float* stats, int n, int f, int q,
                      int rule, const float* gammas, int B, int* flags,
                      hipStream_t stream);
// gamma_out[0] = the feasible end of a bracket <= 2^-16 (relative) wide around
// the upper end of the feasible interval that starts at gamma = 0: a
// geometric grid, two linear grids, a one-wave finish. state
// (AGR_STATE_FLOATS) and flags (AGR_GEO_POINTS + 2 AGR_LIN_POINTS) are
// scratch. Bitwise repeatable; no host sync.
constexpr int AGR_GEO_POINTS = 42;   // 0, then gamma0 2^-20 .. gamma0 2^20
constexpr int AGR_LIN_POINTS = 256;  // gap / 257 per pass: 2 / 257^2 < 2^-15,
                                     // 1 / 257^2 < 2^-16 of the lower end
constexpr int AGR_STATE_FLOATS = 6;
void launch_agr_search(const float* G, const float* stats, int n, int f, int q,
                       int rule, float* state, int* flags, float* gamma_out,
                       hipStream_t stream);
void launch_smea_select(const float* G, const int* combos, int n, int m, int C,
                        unsigned long long* best, hipStream_t stream);
void launch_mda_pass1(const float* D2, const int* prefixes, int P, int n,
                      int m, int npre, unsigned int* best, hipStream_t stream);
void launch_mda_pass2(const float* D2, const int* prefixes, int P, int n,
                      int m, int npre, unsigned int* best, int* subsets,
                      int* found, hipStream_t stream);
