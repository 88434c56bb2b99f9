// Pivoted Cholesky and spectral factorisations of a symmetric positive semi-definite matrix held in LDS, the write-out that
// turns the factor into a prior (J0, r0), and the test kernel that runs every form on caller-supplied matrices.
//   psd_pivoted_cholesky            work-group version, any n
//   psd_pivoted_cholesky_wave<NMAX> one wave, whole columns in registers, n <= NMAX <= 48
//   psd_pivoted_cholesky_wave4      2 NQ waves, column slices in registers, 48 < n <= NQ x NH
//   psd_spectral_factor             pivoted Cholesky + one-sided Jacobi: eigenvalues to high relative accuracy
//   marg_write_prior                J0 = L^T P^T, r0 = y
//   k_psd_factor                    vpl_ba_debug_psd_factor
// k_marg (ba_marg.h) is their user; the LDS scratch each form asks for is named in ba_marg_layout.h.
#pragma once
#include "ba_common.h"
#include "ba_marg_layout.h"

namespace vpl {

// ---------------------------------------------------------------------------------------------------
// Cholesky with diagonal pivoting of the PSD matrix A (LDS, full storage): P A P^T = L L^T, L = n x rank lower trapezoidal
// left in A (upper part zeroed), perm[t] = original index of row t (positions rank..n-1: the indices that never were pivots,
// ascending).  An optional right-hand side c (length n, permuted in
// step) rides along: on exit c[k] = y_k for k < rank, where L(0:rank,0:rank) y = (P c)(0:rank).
// Stops at the first pivot <= max(abs_tol, max(n eps, rel_tol) * max_i a_ii); the trailing block is then treated as zero.
__device__ __forceinline__ int psd_pivoted_cholesky(double* A, int n, int ld, int* perm, double* red, int* iflag, double rel_tol,
                                    double abs_tol, double* c, double* col /* n doubles of scratch */) {
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63;
  for (int i = tid; i < n; i += T) perm[i] = i;
  __syncthreads();
  int rank = n;
  double tol = 0.0;
  for (int k = 0; k < n; ++k) {
    // pivot: largest remaining diagonal (first index on ties), found by wave 0
    if (tid < 64) {
      double best = -1.0;
      int bi = k;
      for (int i = k + lane; i < n; i += 64) {
        const double d = A[i * ld + i];
        if (d > best) { best = d; bi = i; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      if (lane == 0) { iflag[0] = bi; red[0] = best; }
    }
    __syncthreads();
    const int p = iflag[0];
    const double piv = red[0];
    // dpstrf-style stopping rule with a caller-supplied relative tolerance: a pivot at the noise level of the matrix
    // must not be accepted -- dividing a column of noise by the root of a noise pivot fabricates an O(1) direction
    if (k == 0) tol = fmax(abs_tol, fmax((double)n * 2.220446049250313e-16, rel_tol) * piv);
    if (!(piv > tol)) { rank = k; break; }
    if (p != k) {   // symmetric swap k <-> p (rows, then columns), full storage
      for (int c = tid; c < n; c += T) { const double t = A[k * ld + c]; A[k * ld + c] = A[p * ld + c]; A[p * ld + c] = t; }
      __syncthreads();
      for (int r = tid; r < n; r += T) { const double t = A[r * ld + k]; A[r * ld + k] = A[r * ld + p]; A[r * ld + p] = t; }
      if (tid == 0) {
        const int t = perm[k]; perm[k] = perm[p]; perm[p] = t;
        if (c) { const double tc = c[k]; c[k] = c[p]; c[p] = tc; }
      }
      __syncthreads();
    }
    const double lkk = sqrt(piv);
    const double inv = 1.0 / lkk;
    // The scaled column goes to a side vector first (one barrier); the trailing update reads only that vector, so the
    // column of L, the zeros of row k and the rhs entry can be written in the same phase: two barriers per pivot step
    // instead of three, and no division inside the update.
    for (int i = k + tid; i < n; i += T) col[i] = (i == k) ? lkk : A[i * ld + k] * inv;
    __syncthreads();
    const int m = n - k - 1;
    for (int it = tid; it < m * m; it += T) {
      const int ii = it / m, i = k + 1 + ii, j = k + 1 + (it - ii * m);
      A[i * ld + j] -= col[i] * col[j];
    }
    for (int i = k + tid; i < n; i += T) {
      A[i * ld + k] = col[i];
      if (i > k) A[k * ld + i] = 0.0;           // upper part of row k is not part of L
    }
    if (c) {   // forward substitution rides along: y_k = c_k / l_kk, c_i -= l_ik y_k
      const double yk = c[k] * inv;
      for (int i = k + 1 + tid; i < n; i += T) c[i] -= col[i] * yk;
      __syncthreads();                          // every thread has read c[k]
      if (tid == 0) c[k] = yk;
    } else {
      __syncthreads();
    }
  }
  __syncthreads();
  // positions rank..n-1: the indices that never were pivots, in ascending order as the one-wave versions leave them (the swaps
  // leave them in any order).  Row t of L moves to row dst[t] = rank + the number of smaller indices among them: thread k
  // carries column k over the tail of row k (upper part, not part of L, zeroed below).  Same L entries, same J0.
  if (rank < n) {
    int* dst = (int*)col;                       // (col is free: n ints in n doubles)
    int pt = 0, dt = 0;
    if (tid >= rank && tid < n) {
      pt = perm[tid];
      dt = rank;
      for (int s = rank; s < n; ++s) dt += perm[s] < pt ? 1 : 0;
    }
    __syncthreads();
    if (tid >= rank && tid < n) { dst[tid] = dt; perm[dt] = pt; }
    __syncthreads();
    for (int k = tid; k < rank; k += T)
      for (int t = rank; t < n; ++t) A[k * ld + dst[t]] = A[t * ld + k];
    __syncthreads();
    for (int k = tid; k < rank; k += T)
      for (int t = rank; t < n; ++t) A[t * ld + k] = A[k * ld + t];
    __syncthreads();
  }
  // columns rank..n-1 do not exist
  for (int it = tid; it < n * (n - rank); it += T) A[(it / (n - rank)) * ld + rank + it % (n - rank)] = 0.0;
  __syncthreads();
  return rank;
}

// The same factorisation (same arithmetic per entry, same pivots, same bits) by ONE wave for n <= NMAX <= 48, the matrix
// in registers: lane j owns column j (a[i] = A(i, j), static indices only), its diagonal entry and its rhs entry.  A pivot
// step is: arg-max of the live diagonals by shuffles; the pivot lane writes its scaled column to an LDS vector (col); every
// lane reads its own entry l_j and, broadcast, every l_i, and updates its column -- no work-group barrier and no swaps
// (the permutation is applied once at the end).  The work-group version above pays five barriers per pivot step
// (~3.9 k cycles; 175 k for the 45 x 45 kept block).  All threads of the block must call it; Lo is n x ld scratch.
template <int NMAX>
__device__ __forceinline__ int psd_pivoted_cholesky_wave(double* A, int n, int ld, int* perm, int* iflag, double rel_tol, double abs_tol,
                                         double* c, double* Lo /* n x ld + NMAX doubles */) {
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63;
  double* col = Lo + n * ld;             // NMAX: the pivot column, zero beyond n -- the loops over it have no bounds checks
                                         // (all of Lo: psd_scratch_doubles(n, ld, NMAX, false))
  if (tid < 64) {
    double a[NMAX];
#pragma unroll
    for (int i = 0; i < NMAX; ++i) a[i] = (i < n && lane < n) ? A[i * ld + lane] : 0.0;
    double diag = lane < n ? A[lane * ld + lane] : -1.0;
    double cj = (c && lane < n) ? c[lane] : 0.0;
    bool alive = lane < n;
    unsigned long long mask = __ballot(alive);
    int rank = n;
    double tol = 0.0;
    for (int k = 0; k < n; ++k) {
      // pivot: the largest live diagonal, first index on ties -- maximum by DPP row steps + four readlanes (VALU only; a
      // shuffle butterfly over (value, index) is six dependent LDS-path round trips), index from the ballot of the lanes
      // that hold it.  Dead lanes and the DPP fill value count as 0: no live diagonal above 0 ends the factorisation.
      const double best = alive ? diag : 0.0;
      double mx = best;
      mx = fmax(mx, dpp_shr_f64<0x111>(mx));
      mx = fmax(mx, dpp_shr_f64<0x112>(mx));
      mx = fmax(mx, dpp_shr_f64<0x114>(mx));
      mx = fmax(mx, dpp_shr_f64<0x118>(mx));
      const double piv = fmax(fmax(readlane_f64(mx, 15), readlane_f64(mx, 31)), fmax(readlane_f64(mx, 47), readlane_f64(mx, 63)));
      const unsigned long long hit = __ballot(alive && diag == piv);
      const int p = hit ? __builtin_ctzll(hit) : 0;
      if (k == 0) tol = fmax(abs_tol, fmax((double)n * 2.220446049250313e-16, rel_tol) * piv);
      if (!(piv > tol)) { rank = k; break; }
      const double lkk = sqrt(piv);
      const double inv = 1.0 / lkk;
      if (lane == p) {
        // (rows that are already eliminated get a meaningless entry: it only ever touches their own dead rows and the
        //  part of Lo above the diagonal, which the final pass never reads)
#pragma unroll
        for (int i = 0; i < NMAX; ++i) col[i] = a[i] * inv;
        col[p] = lkk;
        perm[k] = p;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      const double lj = lane < n ? col[lane] : 0.0;
      const bool upd = alive && lane != p;
      const double ljm = upd ? lj : 0.0;
#pragma unroll
      for (int i = 0; i < NMAX; ++i) a[i] -= col[i] * ljm;     // (uniform addresses: broadcast reads, all in flight)
      if (upd) diag -= lj * lj;
      if (lane < n) Lo[lane * ld + k] = lj;
      if (c) {
        const double yk = readlane_f64(cj, p) * inv;
        if (upd) cj -= lj * yk;
        if (lane == p) cj = yk;          // lane p keeps y_k: stored at position k below
      }
      if (lane == p) alive = false;
      mask &= ~(1ull << p);
      __builtin_amdgcn_wave_barrier();   // col is rewritten by the next pivot lane
    }
    // positions rank..n-1: the indices that were never pivots, ascending
    {
      const int before = __popcll(mask & ((1ull << lane) - 1ull));
      if (alive) perm[rank + before] = lane;
    }
    if (c && lane < n) col[lane] = cj;   // y_k sits in lane perm[k]
    if (lane == 0) iflag[0] = rank;
  }
  __syncthreads();
  const int rank = iflag[0];
  // L(t, k) = Lo(perm[t], k), t >= k, k < rank; everything else zero
  for (int it = tid; it < n * n; it += T) {
    const int t = it / n, k = it - t * n;
    A[t * ld + k] = (k < rank && t >= k) ? Lo[perm[t] * ld + k] : 0.0;
  }
  if (c)
    for (int k = tid; k < n; k += T) c[k] = k < rank ? col[perm[k]] : 0.0;
  __syncthreads();
  return rank;
}

// The same factorisation for 48 < n <= NMAX = NQ x NH by 2 NQ waves with column SLICES in registers (round 4: the reference's
// steady-state kept block has 75 dims; a whole 76-entry column per lane does not fit the register file next to what the
// compiler needs around it -- DESIGN.md section 8 (2)).  Wave w: column group w & 1 (columns 64 (w & 1) + lane), row slice
// w >> 1 (rows NH (w >> 1) .. + NH - 1); k_marg<512> uses NQ = 4 slices of 19 rows on its eight waves.  Every lane keeps the
// diagonal entry of its column (all slices update it with the same arithmetic), the lanes of slice 0 the rhs entry.  Pivot step k:
//   A  the two waves of slice 0 find the largest live diagonal of their columns (first lane on ties) and write (value, index,
//      rhs entry) into slot k & 1 of `meta`; EVERY wave then arrives at counter A and waits until all have: everybody has
//      finished step k - 1 (its reads of the previous column and candidates), and the candidates of step k are visible.  The
//      winner is the larger value, column group 0 on ties = the lower index (the one-wave rule);
//   B  the NQ lanes that own the winning column write its scaled slices into `col`, their waves arrive at counter B; every
//      wave waits for them;
//   C  every lane reads its own entry l_j and, broadcast, the NH entries of its row slice, and updates.
// The counters only grow (relaxed LDS atomics + work-group fences).  A wait gives up after 2^24 polls and the call returns
// -1 instead of hanging the device.  Same pivots and same arithmetic per entry as the other versions, except 1 / sqrt(pivot)
// (hardware estimate + two Newton steps).  Lo: n x ld + NMAX + 24 doubles of scratch.
template <int NH, int NQ>
__device__ __forceinline__ int psd_pivoted_cholesky_wave4(double* A, int n, int ld, int* perm, int* iflag, double rel_tol, double abs_tol,
                                                          double* c, double* Lo, int* phase /* 4 ints of LDS */,
                                                          long long* stamps = nullptr) {
  constexpr int NMAX = NQ * NH;     // NQ row slices of NH rows: 2 NQ waves
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wv = tid >> 6;
  double* col = Lo + n * ld;             // NMAX: the winning column, scaled
  static_assert(PSD_WAVE4_META >= 8 * 2 + 2, "meta: two slots of two groups of four words, and the two tail counts");
  double* meta = col + NMAX;             // PSD_WAVE4_META (all of Lo: psd_scratch_doubles(n, ld, NMAX, true)): [2 slots][2 groups][4]: value, global index, rhs entry; [16], [17]: tail counts
  if (tid < 4) phase[tid] = 0;
  if (tid == 4) iflag[1] = 0;
  __syncthreads();
  double cj = 0.0;
  int gcol = 0, hf = 1;
  if (wv < 2 * NQ) {
    const int cg = wv & 1, r0 = NH * (wv >> 1);
    hf = wv >> 1;      // row slice; slice 0 holds the candidates, the rhs and writes the factor
    gcol = 64 * cg + lane;
    double a[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) a[i] = (r0 + i < n && gcol < n) ? A[(r0 + i) * ld + gcol] : 0.0;
    double diag = gcol < n ? A[gcol * ld + gcol] : -1.0;
    cj = (c && hf == 0 && gcol < n) ? c[gcol] : 0.0;
    bool alive = gcol < n;
    int rank = n;
    double tol = 0.0;
    bool dead = false;                   // a wait timed out
    // phase[0]: arrivals at A (every wave, once per step); phase[1]: arrivals at B (the two waves that own the winning column);
    // phase[2]: the tail of the top-half waves.  Counters only grow; one LDS word is polled per wait.
#ifdef VPL_STAMPS
    long long st_wait[2] = {0, 0}, st_b = 0, st_c = 0;
#endif
    auto wait_cnt = [&](int which, int v) {
#ifdef VPL_STAMPS
      const long long t0 = __builtin_readcyclecounter();
#endif
      int polls = 0;
      while (!dead && __hip_atomic_load(&phase[which], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < v)
        if (++polls > (1 << 24)) dead = true;
#ifdef VPL_STAMPS
      if (which < 2) st_wait[which] += __builtin_readcyclecounter() - t0;
#endif
    };
    auto arrive = [&](int which) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) __hip_atomic_fetch_add(&phase[which], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    for (int k = 0; k < n; ++k) {
      // A: candidates of the two column groups (top-half waves), slot k & 1
      if (hf == 0) {
        const double best = alive ? diag : 0.0;
        double mx = best;
        mx = fmax(mx, dpp_shr_f64<0x111>(mx));
        mx = fmax(mx, dpp_shr_f64<0x112>(mx));
        mx = fmax(mx, dpp_shr_f64<0x114>(mx));
        mx = fmax(mx, dpp_shr_f64<0x118>(mx));
        const double pw = fmax(fmax(readlane_f64(mx, 15), readlane_f64(mx, 31)), fmax(readlane_f64(mx, 47), readlane_f64(mx, 63)));
        const unsigned long long hit = __ballot(alive && diag == pw);
        const int pl = hit ? __builtin_ctzll(hit) : 0;
        if (lane == pl) {
          double* mm = meta + 8 * (k & 1) + 4 * cg;
          mm[0] = (hit && pw > 0.0) ? pw : 0.0;     // (a group without a live positive diagonal offers 0)
          mm[1] = (double)gcol;
          mm[2] = cj;
        }
      }
      arrive(0);
      wait_cnt(0, 2 * NQ * (k + 1));
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (dead) break;
      const double* mk = meta + 8 * (k & 1);
      const double p0 = mk[0], p1 = mk[4];
      const int win = p1 > p0 ? 1 : 0;
      const double piv = win ? p1 : p0;
      const int p = (int)(win ? mk[5] : mk[1]);
      const double cjp = win ? mk[6] : mk[2];
      if (k == 0) tol = fmax(abs_tol, fmax((double)n * 2.220446049250313e-16, rel_tol) * piv);
      if (!(piv > tol)) { rank = k; break; }
      // 1 / sqrt(pivot) by v_rsq_f64 + two Newton steps, sqrt(pivot) = pivot / sqrt(pivot): ~10 dependent instructions on the
      // critical path of every wave where an IEEE sqrt and divide are ~45 (as k_chol's chains do; the results agree with the
      // correctly rounded ones to an ulp -- the other versions of this factorisation keep sqrt() and the division)
      double inv = __builtin_amdgcn_rsq(piv);
      inv = inv * fma(-0.5 * piv * inv, inv, 1.5);
      inv = inv * fma(-0.5 * piv * inv, inv, 1.5);
      const double lkk = piv * inv;
      // B: the two lanes of column p write its halves (everybody is past step k - 1: the wait above)
      if (gcol == p) {
#pragma unroll
        for (int i = 0; i < NH; ++i) col[r0 + i] = a[i] * inv;
        if (p >= r0 && p < r0 + NH) col[p] = lkk;
      }
      if (cg == win) arrive(1);          // (the wave holds column p: wave-uniform)
      wait_cnt(1, NQ * (k + 1));
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (dead) break;
      // C: update
      const double lj = gcol < n ? col[gcol] : 0.0;
      const bool upd = alive && gcol != p;
      const double ljm = upd ? lj : 0.0;
#pragma unroll
      for (int i = 0; i < NH; ++i) a[i] -= col[r0 + i] * ljm;     // (uniform addresses: broadcast reads)
      if (upd) diag -= lj * lj;
      if (hf == 0) {
        if (gcol < n) Lo[gcol * ld + k] = lj;
        if (c) {
          const double yk = cjp * inv;
          if (upd) cj -= lj * yk;
          if (gcol == p) cj = yk;          // column p keeps y_k: stored at position k below
        }
        if (gcol == p) perm[k] = p;
      }
      if (gcol == p) alive = false;
    }
    // positions rank..n-1: the indices that were never pivots, ascending -- column group 0 first (top-half waves)
    if (hf == 0) {
      const unsigned long long mask = __ballot(alive);
      if (lane == 0) meta[16 + cg] = (double)__popcll(mask);
      arrive(2);
      wait_cnt(2, 2);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (!dead) {
        const int before = __popcll(mask & ((1ull << lane) - 1ull)) + (cg ? (int)meta[16] : 0);
        if (alive) perm[rank + before] = gcol;
      }
    }
    if (dead && lane == 0) iflag[1] = 1;
    if (tid == 0) iflag[0] = rank;
#ifdef VPL_STAMPS
    if (stamps && lane == 0 && wv < 4) { stamps[2 * wv] = st_wait[0]; stamps[2 * wv + 1] = st_wait[1]; }
#endif
  }
  __syncthreads();                       // every wave is past its last read of col
  if (c && hf == 0 && gcol < n) col[gcol] = cj;   // y_k sits in column perm[k]
  __syncthreads();
  if (iflag[1]) return -1;
  const int rank = iflag[0];
  // L(t, k) = Lo(perm[t], k), t >= k, k < rank; everything else zero
  for (int it = tid; it < n * n; it += T) {
    const int t = it / n, k = it - t * n;
    A[t * ld + k] = (k < rank && t >= k) ? Lo[perm[t] * ld + k] : 0.0;
  }
  if (c)
    for (int k = tid; k < n; k += T) c[k] = k < rank ? col[perm[k]] : 0.0;
  __syncthreads();
  return rank;
}

// Spectral factor of a symmetric positive semi-definite matrix held in LDS (full storage, row stride ld):
//     A = B B^T,  B = P^T G,  columns of G mutually orthogonal,  |g_k|^2 = lambda_k (eigenvalues of A).
// Step 1: Cholesky with diagonal pivoting, P A P^T = L L^T (stops at the first pivot <= n eps max_i a_ii, as dpstrf).
// Step 2: one-sided (Hestenes) Jacobi on the columns of L until they are orthogonal: G = L J.
// The Cholesky factor of a graded PSD matrix is what makes Jacobi converge in a few sweeps and to high
// RELATIVE accuracy of the small eigenvalues (Demmel & Veselic), which the marginalisation needs because it
// consumes 1/lambda (pseudo-inverse) and 1/sqrt(lambda).  Round-robin ordering, 8 lanes per column pair,
// one barrier per step.  On exit: A holds G (n x rank), lam[k] = |g_k|^2, perm[t] = original index of row t.
// Returns the rank.  Needs blockDim.x >= 8 * ((n + 1) / 2).  rel_tol: pivots <= max(n eps, rel_tol) * max_i a_ii stop the
// factorisation (the trailing block is then treated as zero).
static_assert(MAXKEEP <= 80, "psd_spectral_factor keeps 10 rows per lane (8 lanes per column pair)");
__device__ __forceinline__ int psd_spectral_factor(double* A, int n, int ld, int* perm, double* lam, double* red, int* iflag,
                                   double rel_tol, double* Lo /* n x ld + 16 doubles for n <= 16, else unused */) {
  const int tid = threadIdx.x, T = blockDim.x;
  const int rank = n <= PSD_NMAX_AMM ? psd_pivoted_cholesky_wave<PSD_NMAX_AMM>(A, n, ld, perm, iflag, rel_tol, 0.0, nullptr, Lo)
                           : psd_pivoted_cholesky(A, n, ld, perm, red, iflag, rel_tol, 0.0, nullptr, lam);
  // ---- one-sided Jacobi on the rank columns ----
  const int m = (rank + 1) & ~1, half = m / 2;
  const int P = tid >> 3, sub = tid & 7;
  for (int sweep = 0; sweep < 40 && rank > 1; ++sweep) {
    if (tid == 0) iflag[1] = 0;
    __syncthreads();
    for (int step = 0; step < m - 1; ++step) {
      if (P < half) {
        const int a = P == 0 ? 0 : 1 + (P - 1 + step) % (m - 1);
        const int b = P == 0 ? 1 + (m - 2 + step) % (m - 1) : 1 + (m - 2 - P + step) % (m - 1);
        const int ci = min(a, b), cj = max(a, b);
        double gi[10], gj[10];
        double al = 0, be = 0, ga = 0;
        if (cj < rank) {
#pragma unroll
          for (int q = 0; q < 10; ++q) {
            const int r = sub + 8 * q;
            gi[q] = r < n ? A[r * ld + ci] : 0.0;
            gj[q] = r < n ? A[r * ld + cj] : 0.0;
            al += gi[q] * gi[q]; be += gj[q] * gj[q]; ga += gi[q] * gj[q];
          }
        }
        al += __shfl_xor(al, 1, 64); al += __shfl_xor(al, 2, 64); al += __shfl_xor(al, 4, 64);
        be += __shfl_xor(be, 1, 64); be += __shfl_xor(be, 2, 64); be += __shfl_xor(be, 4, 64);
        ga += __shfl_xor(ga, 1, 64); ga += __shfl_xor(ga, 2, 64); ga += __shfl_xor(ga, 4, 64);
        if (cj < rank && fabs(ga) > 1e-15 * sqrt(al * be) && ga != 0.0) {
          const double zeta = (be - al) / (2.0 * ga);
          const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
#pragma unroll
          for (int q = 0; q < 10; ++q) {
            const int r = sub + 8 * q;
            if (r < n) {
              A[r * ld + ci] = c * gi[q] - sn * gj[q];
              A[r * ld + cj] = sn * gi[q] + c * gj[q];
            }
          }
          if (sub == 0) iflag[1] = 1;
        }
      }
      __syncthreads();
    }
    if (!iflag[1]) break;
    __syncthreads();
  }
  __syncthreads();
  for (int k = tid; k < n; k += T) {
    double s2 = 0;
    if (k < rank)
      for (int r = 0; r < n; ++r) s2 += A[r * ld + k] * A[r * ld + k];
    lam[k] = s2;
  }
  __syncthreads();
  return rank;
}

// The prior out of the factor the routines above leave in LDS (G: L, n x rank lower trapezoidal, row stride ldm; bv: y; perm):
// J0 = L^T P^T, i.e. J0[k][perm[t]] = L[t][k], and r0 = y, rows rank..n-1 zero.  k_marg and the test kernel k_psd_factor share it.
template <int T>
__device__ __forceinline__ void marg_write_prior(double* J0, double* r0, const double* G, const double* bv, const int* perm,
                                                 const int n, const int ldm, const int rank) {
  const int tid = threadIdx.x;
  // (the block is cleared first: the loop below covers it only if perm is a permutation, and a column it leaves out must not
  //  keep the prior of the batch the context solved before -- DESIGN.md section 6, the open item of round 4)
  for (int it = tid; it < n * n; it += T) J0[it] = 0.0;
  __syncthreads();
  for (int it = tid; it < n * n; it += T) {
    const int k = it / n, t = it % n;   // J0[k][perm[t]] = L[t][k]
    J0[k * n + perm[t]] = (k < rank && t >= k) ? G[t * ldm + k] : 0.0;
  }
  for (int k = tid; k < n; k += T) r0[k] = k < rank ? bv[k] : 0.0;
}

// Test kernel of vpl_ba_debug_psd_factor: every form of the pivoted Cholesky factorisation on matrices the caller supplies, one
// work-group per case, through k_marg's own write-out and in its geometry (row stride n | 1, the scratch the routines ask for,
// the iflag / phase words).  form: 0 wave<16>, 1 wave<48>, 2 wave4<19, 4> (512 threads only), 3 the work-group version; the host
// refuses every other pairing of form, thread count and n.  A, J0: [case][MAXKEEP^2] holding n x n; b, r0, perm_out: [case][MAXKEEP].
// perm starts as zeros (in range: a store that does not land cannot send the write-out outside J0), J0 and r0 arrive filled with
// NaN from the host.  rank -1: wave4 gave up a wait; nothing else is written for that case.
// A geometry of its own, with the scratch extents ba_marg_layout.h names:
// G | Lo (the largest any form asks for: NMAX = MAXKEEP, wave4's meta words) | bv | col | red | perm
__host__ __device__ inline int psd_test_lds_doubles(int n) {
  const int nn = n < 2 ? 2 : n, ld = nn | 1;
  return nn * ld + psd_scratch_doubles(nn, ld, MAXKEEP, true) + 2 * MAXKEEP + MARG_RED_DOUBLES + MAXKEEP / 2;
}
template <int T>
__global__ __launch_bounds__(T) void k_psd_factor(const int form, const int* __restrict__ ns, const double* __restrict__ As,
                                                  const double* __restrict__ bs, const double* __restrict__ abs_tols,
                                                  const double* __restrict__ rel_tols, int* __restrict__ ranks,
                                                  int* __restrict__ perm_out, double* __restrict__ J0s, double* __restrict__ r0s) {
  extern __shared__ double sm[];
  __shared__ int s_flag[4], s_phase[4];
  const int tid = threadIdx.x, cs = blockIdx.x;
  const int n = ns[cs];
  const int nn = n < 2 ? 2 : n, ld = nn | 1;   // marg_layout's ldm
  double* G = sm;
  double* Lo = G + nn * ld;
  double* bv = Lo + nn * ld + MAXKEEP + PSD_WAVE4_META;   // psd_scratch_doubles(nn, ld, MAXKEEP, true), as pointer steps
  double* col = bv + MAXKEEP;
  double* red = col + MAXKEEP;
  int* perm = (int*)(red + MARG_RED_DOUBLES);
  const double* A = As + (size_t)cs * MAXKEEP * MAXKEEP;
  for (int it = tid; it < n * n; it += T) G[(it / n) * ld + it % n] = A[it];
  for (int i = tid; i < MAXKEEP; i += T) { bv[i] = i < n ? bs[(size_t)cs * MAXKEEP + i] : 0.0; perm[i] = 0; }
  __syncthreads();
  const double at = abs_tols[cs], rt = rel_tols[cs];
  int rank;
  if (form == 0) rank = psd_pivoted_cholesky_wave<16>(G, n, ld, perm, s_flag, rt, at, bv, Lo);
  else if (form == 1) rank = psd_pivoted_cholesky_wave<48>(G, n, ld, perm, s_flag, rt, at, bv, Lo);
  else if (form == 2) {
    if constexpr (T >= 512) rank = psd_pivoted_cholesky_wave4<19, 4>(G, n, ld, perm, s_flag, rt, at, bv, Lo, s_phase);
    else rank = -1;
  } else rank = psd_pivoted_cholesky(G, n, ld, perm, red, s_flag, rt, at, bv, col);
  if (tid == 0) ranks[cs] = rank;
  if (rank < 0) return;   // (work-group uniform)
  for (int i = tid; i < n; i += T) perm_out[(size_t)cs * MAXKEEP + i] = perm[i];
  marg_write_prior<T>(J0s + (size_t)cs * MAXKEEP * MAXKEEP, r0s + (size_t)cs * MAXKEEP, G, bv, perm, n, ld, rank);
}

}  // namespace vpl
