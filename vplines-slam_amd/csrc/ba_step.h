// The trust-region step of a window as three bodies of one launch shape (256 threads, two work-groups per CU, no scratch):
// k_step runs them one after the other in ONE launch per step (the default); k_schur / k_chol / k_back run the same bodies
// as three launches for the per-kernel attribution of the timing mode and for A/B runs (VPL_BA_STEP_FUSED=0).
// Each body is its early-outs, one carve of the LDS by ba_step_layout.h (the layout the host sized the dispatch with: regions,
// tenants, the slack) and the list of its phases; the barriers between the phases stand in the body, each with what it hands over.
//
//   k_schur  (~76 KB LDS at 200 points + 80 lines)  Jacobi scaling, dogleg diagonal / gradient, Cauchy point,
//            regularised landmark blocks, and the landmark elimination: the rows of X = C^-1 S [W | g | e] go from HBM
//            straight into the FP64 matrix cores -- the lane that supplies operand element (row, column) loads exactly that
//            element -- in the COMPACT coordinates of the rows' start frame (WS + 2 columns instead of 80), every wave on its
//            own span of rows.  No staging buffers, no work-group barriers in the product.
//   k_chol   (~62 KB LDS)  the reduced camera system.  The 99 speed/bias dims touch IMU
//            factors and the prior only: the blocks of frames 1..4 and 10..6 are eliminated first as two block chains (one
//            wave each, 9-row strips held in registers with the columns in the lanes), which leaves the DENSE system
//            [72 pose / extrinsic dims | speed/bias 0 | speed/bias 5 | rhs] = 91 rows = 6 tile columns instead of 11.
//   k_back   (~16 KB LDS)  landmark back-substitution, dogleg step, model cost change, candidate x (Plus).
//
// Any elimination order gives the same Gauss-Newton step up to rounding; the pieces of the step that
// do not depend on it are shared with the general path (ba_trust.h).  Windows the fast path does not cover -- a prior that
// holds a speed/bias block of another frame than 0, a factorisation that failed and is retried with a larger mu (ceres'
// LINEAR_SOLVER_FAILURE loop) -- are flagged in B.path and take k_solve (ba_solve.h), which is launched after k_step (three
// launches: between k_chol and k_back) and leaves at once for everybody else.
// Restates ceres-solver 1.12 DoglegStrategy::ComputeStep / SchurEliminator / TrustRegionMinimizer (third party, absent
// from the reference tree) for the configuration at vins_estimator/src/estimator.cpp:1207-1215.
#pragma once
#include "ba_common.h"
#include "ba_pack.h"
#include "ba_solve.h"
#include "ba_step_layout.h"

namespace vpl {

constexpr int SCHUR_THREADS = 256;
constexpr int CHOL_THREADS = 256;
constexpr int BACK_THREADS = 256;

__device__ __forceinline__ void lds_ticket_wait(int* t, int seq) {
  while (__hip_atomic_load(t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != seq) __builtin_amdgcn_s_sleep(1);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");   // (LDS only: global loads in flight stay in flight)
}
__device__ __forceinline__ void lds_ticket_pass(int* t, int seq, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  if (lane == 0) __hip_atomic_store(t, seq + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// vis index (0..73: 72 = rhs row, 73 = Cauchy row) of compact column c of a row whose track starts in frame s; -1: the slot
// of a frame past the window (always zero) or padding
__device__ __forceinline__ int compact2vis(int c, int s, int WS) {
  if (c < WS - 6) { const int v = 6 * s + c; return v < 66 ? v : -1; }
  if (c < WS) return 66 + (c - (WS - 6));
  return c < WS + 2 ? 72 + (c - WS) : -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// k_schur
// ---------------------------------------------------------------------------------------------------------------------
// NTC: 16-column tiles of the compact row (WS + 2 <= 16 NTC).  NTC = 3 covers tracks of up to 6 frames (the benchmark
// shape): 6 lower tiles = 48 accumulator registers per lane; NTC = 5 covers every track length (15 tiles).
// (CSQ_LD = 80, the row stride of the compact system in LDS, and its size CSQ_N: ba_step_layout.h)
// A WIDE chunk of k_schur_mixed (entries that hold a track of more than SCHUR_NARROW_FRAMES frames), out of line: its
// register allocation is its own, the narrow product loop of the caller keeps its zero scratch.
struct SchurWide {
  const int4* etab;
  const double *Wp, *Wl;
  int WS;
  const double *lC, *lS, *lE, *lG, *pS, *pE, *pG;
  double* Cacc;
  int* tick;
};
__device__ __noinline__ void schur_wide_chunk(const SchurWide& A, const int k0, const int k1, const int seq) {
  const int lane = threadIdx.x & 63, m = lane & 15, kk = lane >> 4;
  const int4* etab = A.etab;
  const double *Wp = A.Wp, *Wl = A.Wl, *lC = A.lC, *lS = A.lS, *lE = A.lE, *lG = A.lG, *pS = A.pS, *pE = A.pE, *pG = A.pG;
  double* Cacc = A.Cacc;
  int* tick = A.tick;
  const int WS = A.WS;
  auto fetch = [&](int k) {
    int4 e = etab[k];
    e.x = __builtin_amdgcn_readfirstlane(e.x); e.y = __builtin_amdgcn_readfirstlane(e.y); e.z = __builtin_amdgcn_readfirstlane(e.z);
    return e;
  };
  auto lm_id = [&](const int4 e) { return ((kk & 2 ? e.z : e.y) >> (16 * (kk & 1))) & 0xffff; };
  {
        // ---- a WIDE chunk: all NTW = 5 column tiles of the WS + 2 columns, ONE ROW OF TILES PER PASS over the chunk's entries
        // (pass ta: tiles (ta, 0 .. 4), the A operand is column tile ta, loaded as a sixth column): 5 accumulator tiles, 6
        // raw and 6 transformed columns = fewer registers than the narrow product loop, which therefore keeps its zero
        // scratch (all 15 tiles at once: 1.2 KB of scratch per lane for the whole kernel).  Wide chunks are the few entries
        // with long tracks; their rows are read five times.  Flush targets by arithmetic (no second 15 KB table in LDS).
        // The ticket is taken at the first pass's adds and passed on after the last's.
        constexpr int NTW = 5;
        const int sfr = fetch(k0).x & 15, s6 = 6 * sfr;
#pragma unroll 1
        for (int ta = 0; ta < NTW && 16 * ta < WS + 2; ++ta) {
          v4d accw[NTW];
#pragma unroll
          for (int t = 0; t < NTW; ++t) accw[t] = v4d{0, 0, 0, 0};
          auto col_of = [&](int t) { return 16 * (t < NTW ? t : ta) + m; };
          auto load_w = [&](const int4 e, double (&raw)[NTW + 1][4]) {
            const bool isl = (e.x & 32) != 0;
            const int idr = lm_id(e);
            const int id = idr != 0xffff ? idr : 0;
            const double* row = isl ? Wl + (unsigned)(id * 4 * WS) : Wp + (unsigned)(id * WS);
#pragma unroll
            for (int t = 0; t <= NTW; ++t) {
              const int c = min(col_of(t), WS - 1);
#pragma unroll
              for (int qd = 0; qd < 4; ++qd) raw[t][qd] = (qd == 0 || isl) ? row[(unsigned)((isl ? qd * WS : 0) + c)] : 0.0;
            }
          };
          auto xform_w = [&](const int4 e, const double (&raw)[NTW + 1][4], double (&x)[NTW + 1][4]) {
            const bool isl = (e.x & 32) != 0;
            const int idr = lm_id(e);
            const int id = idr != 0xffff ? idr : 0;
            const double pm = idr != 0xffff ? 1.0 : 0.0;
            double s4[4] = {0, 0, 0, 0}, ev[4] = {0, 0, 0, 0}, gv[4] = {0, 0, 0, 0};
            double c10 = 0, c20 = 0, c21 = 0, c30 = 0, c31 = 0, c32 = 0;
            if (isl) {
              const double* C = lC + id * 10;
#pragma unroll
              for (int a = 0; a < 4; ++a) { s4[a] = lS[4 * id + a] * pm; ev[a] = lE[4 * id + a] * pm; gv[a] = lG[4 * id + a] * pm; }
              c10 = C[1]; c20 = C[3]; c21 = C[4]; c30 = C[6]; c31 = C[7]; c32 = C[8];
            } else {
              s4[0] = pS[id] * pm; ev[0] = pE[id] * pm; gv[0] = pG[id] * pm;
            }
#pragma unroll
            for (int t = 0; t <= NTW; ++t) {
              const int c = col_of(t);
              const double wmv = c < WS ? 1.0 : 0.0, gmv = c == WS ? 1.0 : 0.0, emv = c == WS + 1 ? 1.0 : 0.0;
              // (same operations per element as the table-driven path: s * raw first, the triangular solve for the lines)
              const double x0 = s4[0] * raw[t][0];
              const double x1 = s4[1] * raw[t][1] - c10 * x0;
              const double x2 = s4[2] * raw[t][2] - c20 * x0 - c21 * x1;
              const double x3 = s4[3] * raw[t][3] - c30 * x0 - c31 * x1 - c32 * x2;
              x[t][0] = x0 * wmv + gv[0] * gmv + ev[0] * emv;
              x[t][1] = isl ? x1 * wmv + gv[1] * gmv + ev[1] * emv : 0.0;
              x[t][2] = isl ? x2 * wmv + gv[2] * gmv + ev[2] * emv : 0.0;
              x[t][3] = isl ? x3 * wmv + gv[3] * gmv + ev[3] * emv : 0.0;
            }
          };
          double rw[NTW + 1][4];
          load_w(fetch(k0), rw);
#pragma unroll 1
          for (int k = k0; k < k1; ++k) {
            const int4 e = fetch(k);
            double x[NTW + 1][4];
            xform_w(e, rw, x);
            load_w(fetch(min(k + 1, k1 - 1)), rw);
            const bool isl = (e.x & 32) != 0;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
              if (a == 0 || isl) {
#pragma unroll
                for (int tb = 0; tb < NTW; ++tb) accw[tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[NTW][a], x[tb][a], accw[tb], 0, 0, 0);
              }
            }
          }
          if (ta == 0) lds_ticket_wait(&tick[0], seq);
#pragma unroll
          for (int tb = 0; tb < NTW; ++tb) {
            const double vals[4] = {accw[tb].x, accw[tb].y, accw[tb].z, accw[tb].w};
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int ca = 16 * ta + kk + 4 * v, cb = 16 * tb + m;
              if (tb <= ta && ca >= cb && ca < WS + 2 && cb < WS) {
                const int a0 = compact2vis(ca, 0, WS), b0 = compact2vis(cb, 0, WS);
                const int stp = (ca < WS - 6 ? CSQ_LD : 0) + (cb < WS - 6 ? 1 : 0);
                // columns of frames past the window (6 s + c >= 66) hold exact zeros: kept out of the square
                const bool in_a = ca >= WS - 6 || s6 + ca < 66, in_b = cb >= WS - 6 || s6 + cb < 66;
                if (in_a && in_b) lds_add(&Cacc[a0 * CSQ_LD + b0 + s6 * stp], vals[v]);
              }
            }
          }
        }
        lds_ticket_pass(&tick[0], seq, lane);
  }
}

// MIXED (round 4; NTC = 3): the batch holds tracks of more than SCHUR_NARROW_FRAMES frames, so the compact rows in HBM are WS > 42
// doubles wide -- but most entries still hold 6-frame tracks only.  Their chunks run the 3-tile product in a NARROW VIEW of the
// row (the 36 pose columns of frames s .. s + 5, then the extrinsic block found at memory column WS - 6, g, e: 44 columns);
// the chunks the host flagged wide (bit 6 of the group) run all 15 tiles of the WS + 2 columns.  Before, one long track in the
// batch sent every entry through k_schur<5>: 120 accumulator + 120 prefetch registers (spills), 86 KB of LDS (one work-group
// per CU), 5 x the time.
constexpr int SCHUR_NARROW_FRAMES = 6;

// ---- the phases of schur_body, in its order; every thread of the work-group calls each ----

// the window's K-step table to LDS; the ticket and the failure flag start at zero
__device__ __forceinline__ void schur_copy_table(const DevBatch& B, const int w, int4* etab, int* tick, int* flag) {
  const int tid = threadIdx.x, T = SCHUR_THREADS;
  {
    const int4* ktab = (const int4*)B.sk_tab + (size_t)w * B.maxKS;
    for (int k = tid; k < B.maxKS; k += T) etab[k] = ktab[k];
  }
  if (tid == 0) { flag[0] = 0; tick[0] = 0; }
}

// camera part of the Cauchy denominator u^T Hcc u over the entries the factors can fill (B.nz_tab: 6147 of the 14706 of the
// packed triangle; everything else is a structural zero on this path), 12 loads in flight per thread; added to qq
__device__ __forceinline__ void schur_cauchy_camera(const DevBatch& B, const double* Hcc, const double* uc, double& qq) {
  const int tid = threadIdx.x, T = SCHUR_THREADS;
  {
    constexpr int NB = (NZ_N + SCHUR_THREADS - 1) / SCHUR_THREADS;     // 25 at 256 threads
    constexpr int HALF = (NB + 1) / 2;
#pragma unroll 1
    for (int h0 = 0; h0 < NB; h0 += HALF) {
      int code[HALF];
      double hh[HALF];
#pragma unroll
      for (int u = 0; u < HALF; ++u) {
        const int e = (h0 + u) * T + tid;
        code[u] = (h0 + u < NB && e < NZ_N) ? B.nz_tab[e] : -1;
      }
#pragma unroll
      for (int u = 0; u < HALF; ++u) hh[u] = code[u] >= 0 ? Hcc[code[u] & 0x3fff] : 0.0;
#pragma unroll
      for (int u = 0; u < HALF; ++u)
        if (code[u] >= 0) {
          const int r = (code[u] >> 14) & 255, c = code[u] >> 22;
          qq += (r == c ? 1.0 : 2.0) * uc[r] * hh[u] * uc[c];
        }
    }
  }
}

// regularised landmark blocks: points A = s^2 H + mu d^2 -> row scale s / sqrt(A); lines A_l = S H S + mu D^2 = C C^T (to lch
// for k_back).  Reads kP / kL; writes the constants of the row transform and raises flag[0] for a block that is not positive.
__device__ __forceinline__ void schur_landmark_constants(const int nP, const int nL, const double mu, const double* kP, const double* kL,
                                                         double* lch, double* pS, double* pE, double* pG, double* lC, double* lS,
                                                         double* lE, double* lG, int* flag) {
  const int tid = threadIdx.x, T = SCHUR_THREADS;
  for (int p = tid; p < nP; p += T) {
    const double s = kP[4 * p], d = kP[4 * p + 1], g = kP[4 * p + 2], h = kP[4 * p + 3];
    const double Al = s * s * h + mu * d * d;
    if (!(Al > 0.0)) flag[0] = 1;
    const double smv = s / sqrt(Al);
    pS[p] = smv;
    pE[p] = (s * g / d) / smv;
    pG[p] = smv * (g * d / s);               // g_p = g~ d / s (gradient_ = s g / d)
  }
  for (int l = tid; l < nL; l += T) {
    double Hl[16], s4[4], d4[4], g4[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) { s4[a] = kL[28 * l + a]; d4[a] = kL[28 * l + 4 + a]; g4[a] = kL[28 * l + 8 + a]; }
#pragma unroll
    for (int k = 0; k < 16; ++k) Hl[k] = kL[28 * l + 12 + k];
    double A[10];
    if (!line_block(s4, d4, g4, Hl, mu, l, lch, lC, lS, lE, A)) flag[0] = 1;
    {   // x_g = C^-1 S g_l by the same forward substitution the rows of W go through (g_l = g~ d / s)
      double xg[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        double s2 = (s4[a] / A[tri(a, a)]) * (g4[a] * d4[a] / s4[a]);
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) if (qd < a) s2 -= (A[tri(a, qd)] / A[tri(a, a)]) * xg[qd];
        xg[a] = s2;
        lG[4 * l + a] = s2;
      }
    }
  }
}

// the compact system starts at zero; the flush targets of view width WSv
template <int NLT>
__device__ __forceinline__ void schur_zero_and_targets(const int WSv, double* Cacc, int* ftab) {
  const int tid = threadIdx.x, T = SCHUR_THREADS;
  for (int i = tid; i < CSQ_N; i += T) Cacc[i] = 0.0;
  // Flush targets of the accumulator entries (tile t, register v, lane): entry (ca, cb) of the compact product of start
  // frame s goes to row va = map(ca), column vb = map(cb) of the 74 x 80 square, where a pose column maps to 6 s + c and an
  // extrinsic / g / e column to 66.. / 72 / 73: index = idx0 + 6 s * step with step in {0, 1, 80, 81}.  One int per entry in
  // LDS (idx0 | step << 16, -1 = not part of the system) instead of two dozen loop-invariant index registers per lane.
  for (int i = tid; i < NLT * 4 * 64; i += T) {
    const int ln = i & 63, v = (i >> 6) & 3, t = i >> 8;
    int ta = 0, tb = 0;
    tri_decode(t, ta, tb);
    const int ca = 16 * ta + (ln >> 4) + 4 * v, cb = 16 * tb + (ln & 15);
    int code = -1;
    if (ca >= cb && ca < WSv + 2 && cb < WSv) {
      const int a0 = compact2vis(ca, 0, WSv), b0 = compact2vis(cb, 0, WSv);
      const int step = (ca < WSv - 6 ? CSQ_LD : 0) + (cb < WSv - 6 ? 1 : 0);
      code = (a0 * CSQ_LD + b0) | step << 16;
    }
    ftab[i] = code;
  }
}

// X^T X on the matrix cores, operands straight from HBM, every wave on its own span of rows; a wave adds its tiles to Cacc
// when it holds the ticket.  No work-group barrier inside.
// v_mfma_f64_16x16x4: the lane (kk, m) supplies A[k = kk][m] and B[kk][m] of the K-step and holds C[kk + 4 v][m].  With
// x[t] = X[row kk of the K-step][16 t + m] the lower tiles of the compact product are C(ta, tb) += x[ta] (x) x[tb].
// The view the table-driven product works in: logical row width WSv, memory column of logical column c >= WSv - 6 is c + coff.
template <int NTC, bool MIXED>
__device__ __forceinline__ void schur_product(const DevBatch& B, const int w, const int WS, const int WSv, const int coff, const int4* etab,
                                              const int* ftab, double* Cacc, int* tick, const double* lC, const double* lS,
                                              const double* lE, const double* lG, const double* pS, const double* pE, const double* pG) {
  constexpr int NLT = NTC * (NTC + 1) / 2;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  {
    const int m = lane & 15, kk = lane >> 4;
    // the wave's row of the span / ticket table: one int per lane, read with v_readlane
    const int wrow = lane < SK_WSTRIDE ? B.sk_wave[((size_t)w * 8 + wv) * SK_WSTRIDE + lane] : -1;
    const int nchunk = __builtin_amdgcn_readlane(wrow, 0);
    auto fetch = [&](int k) {        // the entry is the same for every lane: scalar registers, uniform branches
      int4 e = etab[k];
      e.x = __builtin_amdgcn_readfirstlane(e.x); e.y = __builtin_amdgcn_readfirstlane(e.y); e.z = __builtin_amdgcn_readfirstlane(e.z);
      return e;
    };
    v4d acc[NLT];
#pragma unroll
    for (int t = 0; t < NLT; ++t) acc[t] = v4d{0, 0, 0, 0};
    const double* Wp = B.Wp + (size_t)w * B.maxP * WS;
    const double* Wl = B.Wl + (size_t)w * B.maxL * 4 * WS;
    const double* gpv = B.gp + (size_t)w * B.maxP;
    const double* glv = B.gl + (size_t)w * B.maxL * 4;
    // A table entry is one K-step: four point rows of one start frame, or the four rows of ONE line.  The lane (kk, m)
    // supplies X[row kk][16 t + m]: a point lane loads one value per column tile; a line lane needs rows 0..kk of the line
    // for the triangular solve with the line block's factor.  The factor of the line is the same for the whole wave: its
    // entries are moved to SCALAR registers (v_readfirstlane) -- as vector registers they, the raw rows and the accumulators
    // do not fit into the 128 registers that two work-groups per CU leave a lane.
    // Branch-free and unconditional: every load is issued with a clamped address, so that the 16 loads of a K-step leave back
    // to back and are waited for once.  The column classes (W column / g column / e column / padding) are applied as 0 / 1
    // MULTIPLIERS held in vector registers: as compare masks they are loop invariants in scalar register pairs, a dozen per
    // inlined copy of this code -- the scalar file overflows, the masks get spilled, and the scheduler, in register-pressure
    // mode, serialises every load behind its select.
    double wm[NTC], gm[NTC], em[NTC];
    int cl[NTC];
#pragma unroll
    for (int t = 0; t < NTC; ++t) {
      const int c = 16 * t + m;
      wm[t] = c < WSv ? 1.0 : 0.0;
      gm[t] = c == WSv ? 1.0 : 0.0;
      em[t] = c == WSv + 1 ? 1.0 : 0.0;
      cl[t] = c < WSv - 6 ? c : (c < WSv ? c + coff : WS - 1);
    }
    // A table entry is four landmarks of one start frame: four points = ONE K-step, four lines = FOUR K-steps (K-step a takes
    // row a of each line).  The lane (kk, m) works on landmark kk of the entry: a point lane loads one value per column tile,
    // a line lane the four rows of ITS line, solves the 4 x 4 triangular system once per column and supplies row a in
    // K-step a -- every loaded value is used once and the solve is not repeated per K-step.
    // (the g column of X is made once per landmark with the constants: the loop loads rows of W and nothing else)
    auto lm_id = [&](const int4 e) { return ((kk & 2 ? e.z : e.y) >> (16 * (kk & 1))) & 0xffff; };
    auto load_raw = [&](const int4 e, double (&raw)[NTC][4]) {
      const bool isl = (e.x & 32) != 0;
      const int idr = lm_id(e);
      const int id = idr != 0xffff ? idr : 0;
      if (isl) {
        const double* Wr = Wl + (unsigned)(id * 4 * WS);
#pragma unroll
        for (int t = 0; t < NTC; ++t)
#pragma unroll
          for (int qd = 0; qd < 4; ++qd) raw[t][qd] = Wr[(unsigned)(qd * WS + cl[t])];
      } else {
#pragma unroll
        for (int t = 0; t < NTC; ++t) raw[t][0] = Wp[(unsigned)(id * WS + cl[t])];
#pragma unroll
        for (int t = 0; t < NTC; ++t)       // (every element defined on both paths)
#pragma unroll
          for (int qd = 1; qd < 4; ++qd) raw[t][qd] = 0.0;
      }
    };
    // x[t][a] = X[row a of the lane's landmark][16 t + m]  (points: a = 0 only)
    auto transform = [&](const int4 e, const double (&raw)[NTC][4], double (&x)[NTC][4]) {
      const bool isl = (e.x & 32) != 0;
      const int idr = lm_id(e);
      const int id = idr != 0xffff ? idr : 0;
      const double pm = idr != 0xffff ? 1.0 : 0.0;
      if (isl) {
        const double* C = lC + id * 10;
        const double s0 = lS[4 * id] * pm, s1 = lS[4 * id + 1] * pm, s2 = lS[4 * id + 2] * pm, s3 = lS[4 * id + 3] * pm;
        const double c10 = C[1], c20 = C[3], c21 = C[4], c30 = C[6], c31 = C[7], c32 = C[8];
        double ev[4], gv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) { ev[a] = lE[4 * id + a] * pm; gv[a] = lG[4 * id + a] * pm; }
#pragma unroll
        for (int t = 0; t < NTC; ++t) {
          const double x0 = s0 * raw[t][0];
          const double x1 = s1 * raw[t][1] - c10 * x0;
          const double x2 = s2 * raw[t][2] - c20 * x0 - c21 * x1;
          const double x3 = s3 * raw[t][3] - c30 * x0 - c31 * x1 - c32 * x2;
          x[t][0] = x0 * wm[t] + gv[0] * gm[t] + ev[0] * em[t];
          x[t][1] = x1 * wm[t] + gv[1] * gm[t] + ev[1] * em[t];
          x[t][2] = x2 * wm[t] + gv[2] * gm[t] + ev[2] * em[t];
          x[t][3] = x3 * wm[t] + gv[3] * gm[t] + ev[3] * em[t];
        }
      } else {
        const double sp = pS[id] * pm, ep = pE[id] * pm, gq = pG[id] * pm;
#pragma unroll
        for (int t = 0; t < NTC; ++t) {
          x[t][0] = sp * raw[t][0] * wm[t] + gq * gm[t] + ep * em[t];
          x[t][1] = 0.0; x[t][2] = 0.0; x[t][3] = 0.0;
        }
      }
    };
    VPL_IVAL(st_flush); VPL_IVAL(st_wait); VPL_IVAL(st_xf); VPL_IVAL(st_mf); VPL_IVAL(st_ld);
    auto flush = [&](int g, int seq) {
      VPL_IVAL_START(tf0);
      const int s6 = 6 * (g & 15);
      // targets first (one batch of LDS reads), then the ticket, then 4 NLT hardware adds (ds_add_f64: no read-back round
      // trip).  Only the holder of the ticket adds, one add per address: the order of the terms of every sum is the ticket order.
      int code[NLT * 4];
#pragma unroll
      for (int i = 0; i < NLT * 4; ++i) code[i] = ftab[i * 64 + lane];
      lds_ticket_wait(&tick[0], seq);
      VPL_IVAL_ADD(st_wait, tf0);
#pragma unroll
      for (int t = 0; t < NLT; ++t) {
        const double vals[4] = {acc[t].x, acc[t].y, acc[t].z, acc[t].w};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int c2 = code[4 * t + v];
          if (c2 >= 0) lds_add(&Cacc[(c2 & 0xffff) + s6 * (c2 >> 16)], vals[v]);
        }
        acc[t] = v4d{0, 0, 0, 0};
      }
      lds_ticket_pass(&tick[0], seq, lane);
      VPL_IVAL_ADD(st_flush, tf0);
    };
    int nent = 0;
#pragma unroll 1
    for (int ch = 0; ch < nchunk; ++ch) {
      const int k0 = __builtin_amdgcn_readlane(wrow, __builtin_amdgcn_readfirstlane(1 + 3 * ch));
      const int k1 = __builtin_amdgcn_readlane(wrow, __builtin_amdgcn_readfirstlane(2 + 3 * ch));
      const int seq = __builtin_amdgcn_readlane(wrow, __builtin_amdgcn_readfirstlane(3 + 3 * ch));
      nent += k1 - k0;
      if (MIXED && (fetch(k0).x & 64)) {   // a WIDE chunk: out of line, with a register allocation of its own
        SchurWide A;
        A.etab = etab; A.Wp = Wp; A.Wl = Wl; A.WS = WS; A.lC = lC; A.lS = lS; A.lE = lE; A.lG = lG; A.pS = pS; A.pE = pE; A.pG = pG;
        A.Cacc = Cacc; A.tick = tick;
        schur_wide_chunk(A, k0, k1, seq);
        continue;
      }
      double raw0[NTC][4], raw1[NTC][4], raw2[NTC][4];
      constexpr int NPF = 3;
      load_raw(fetch(k0), raw0);
      load_raw(fetch(min(k0 + 1, k1 - 1)), raw1);
      load_raw(fetch(min(k0 + 2, k1 - 1)), raw2);
      const int gcur = fetch(k0).x;
      auto step = [&](int k, double (&rw)[NTC][4]) {
        const int4 e = fetch(k);
        VPL_IVAL_START(ts);
        double x[NTC][4];
        transform(e, rw, x);
        VPL_IVAL_LAP(st_xf, ts);
        load_raw(fetch(min(k + NPF, k1 - 1)), rw);      // (past the end: a harmless re-load of the last entry)
        VPL_IVAL_LAP(st_ld, ts);
        const bool isl = (e.x & 32) != 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          if (a == 0 || isl) {
            int t = 0;
#pragma unroll
            for (int ta = 0; ta < NTC; ++ta)
#pragma unroll
              for (int tb = 0; tb <= ta; ++tb, ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[ta][a], x[tb][a], acc[t], 0, 0, 0);
          }
        }
        VPL_IVAL_ADD(st_mf, ts);
      };
#pragma unroll 1
      for (int kb = k0; kb < k1; kb += NPF) {
        step(kb, raw0);
        if (kb + 1 < k1) step(kb + 1, raw1);
        if (kb + 2 < k1) step(kb + 2, raw2);
      }
      flush(gcur, seq);
    }
    VPL_IVAL_STORE(lane == 0 && wv < 2, B.dbg + (size_t)w * 64 + 30 + 6 * wv, st_xf, st_ld, st_mf, st_flush, st_wait, nent);
  }
}

// the compact system to B.sacc for k_chol; the Cauchy point's alpha; a failed landmark block sends the window to k_solve
__device__ __forceinline__ void schur_write_out(const DevBatch& B, const int w, TrState* tr, const double* Cacc, const double* uc, double* red,
                                                const int* flag, double a1, double q, double qq) {
  const int tid = threadIdx.x, T = SCHUR_THREADS;
  // Cauchy cross term (W^T u)_b u_c,b from the e-row of the compact system; alpha = |g~|^2 / (u^T H u)
  for (int b = tid; b < NV; b += T) qq += 2.0 * Cacc[(NV + 1) * CSQ_LD + b] * uc[vis2cam(b)];
  double* sacc = B.sacc + (size_t)w * SACC_N;
  for (int i = tid; i < SACC_N; i += T) {
    int a, b;
    tri_decode(i, a, b);
    sacc[i] = Cacc[a * CSQ_LD + b];
  }
  a1 = block_sum(a1, red);
  q = block_sum(q, red);
  qq = block_sum(qq, red);
  if (tid == 0) {
    tr->a1 = a1;
    tr->alpha = a1 / (q + qq);   // DoglegStrategy::ComputeCauchyPoint
    if (flag[0]) B.path[w] = 2;  // a landmark block is not positive definite: the retry loop lives in k_solve
  }
}

template <int NTC, bool MIXED = false>
__device__ __forceinline__ void schur_body(const DevBatch& B, const int w, double* sm) {
  static_assert(!MIXED || NTC == 3, "the narrow view is three column tiles");
  constexpr int T = SCHUR_THREADS;
  TrState* tr = &B.tr[w];
  if (tr->status != 0 || tr->reuse != 0 || B.path[w] != 0) return;
  count_active(B, 1);
  const int nP = B.nP[w], nL = B.nL[w];
  const int WS = B.WS;
  // the view the table-driven product works in: logical row width WSv, memory column of logical column c >= WSv - 6 is c + coff
  const int WSv = MIXED ? 6 * SCHUR_NARROW_FRAMES + 6 : WS;
  const int coff = WS - WSv;
  // regions and tenants: SchurLayoutT (ba_step_layout.h).  kP / kL and Cacc share the first region.
  const SchurLayoutT<double*> L = schur_layout_at(sm, B.maxP, B.maxL, B.maxKS, NTC);
  double *kP = L.kP.at, *kL = L.kL.at, *Cacc = L.Cacc.at, *pS = L.pS.at, *pE = L.pE.at, *lC = L.lC.at, *lS = L.lS.at, *lE = L.lE.at;
  double *lG = L.lG.at, *pG = L.pG.at, *uc = L.uc.at, *red = L.red.at;
  int *tick = (int*)L.tick.at, *flag = (int*)L.flag.at, *ftab = (int*)L.ftab.at;
  int4* etab = (int4*)L.etab.at;

  schur_copy_table(B, w, etab, tick, flag);
  const double* Hcc = B.Hcc + (size_t)w * NCP;
  double* lch = B.lchol + (size_t)w * B.maxL * 10;
  const double mu = tr->mu;
  const bool first = (tr->iter == 0);
  VPL_STAMP(B, w, 0);
  // ---- jacobi scaling (iteration 0 only), diagonal_, gradient_ ----
  double a1 = 0.0, q = 0.0;
  scale_and_gradient<T, false>(B, w, first, kP, kL, uc, nullptr, nullptr, a1, q);
  __syncthreads();   // uc, kP, kL complete
  double qq = 0.0;
  schur_cauchy_camera(B, Hcc, uc, qq);
  VPL_STAMP(B, w, 1);
  schur_landmark_constants(nP, nL, mu, kP, kL, lch, pS, pE, pG, lC, lS, lE, lG, flag);
  __syncthreads();   // constants complete; kP / kL are dead: their space becomes the compact system
  schur_zero_and_targets<NTC * (NTC + 1) / 2>(WSv, Cacc, ftab);
  __syncthreads();   // Cacc is zero, ftab and etab complete, tick and flag set
  VPL_STAMP(B, w, 2);
  schur_product<NTC, MIXED>(B, w, WS, WSv, coff, etab, ftab, Cacc, tick, lC, lS, lE, lG, pS, pE, pG);
  __syncthreads();   // every wave has added its tiles: Cacc complete
  VPL_STAMP(B, w, 3);
  schur_write_out(B, w, tr, Cacc, uc, red, flag, a1, q, qq);
  VPL_STAMP(B, w, 4);
}

template <int NTC>
__global__ __launch_bounds__(SCHUR_THREADS, 2) void k_schur(DevBatch B) {
  extern __shared__ double sm[];
  empty_next_order(B);
  schur_body<NTC>(B, ordered_window(B), sm);
}
__global__ __launch_bounds__(SCHUR_THREADS, 2) void k_schur_mixed(DevBatch B) {
  extern __shared__ double sm[];
  empty_next_order(B);
  schur_body<3, true>(B, ordered_window(B), sm);
}
inline size_t schur_smem(int maxP, int maxL, int ntc = 5) { return schur_lds_bytes(maxP, maxL, max_schur_ksteps(maxP, maxL), ntc); }

// ---------------------------------------------------------------------------------------------------------------------
// k_chol
// ---------------------------------------------------------------------------------------------------------------------
// Elimination order of the reduced camera system H~ = S (Hcc - Schur) S + mu D^2 (Jacobi-scaled space):
//   chain A: speed/bias blocks of the frames 1, 2, 3, 4 (ascending),  chain B: 10, 9, 8, 7, 6 (descending)
//   dense  : [72 pose / extrinsic dims (vis order) | speed/bias 0 (72..80) | speed/bias 5 (81..89) | rhs (90)]
// A chain block s_f touches, when its turn comes, only the next block of its chain, the poses its chain has met so far, the
// rhs and (chain A) speed/bias 0: at most 64 columns, one per lane.  The 9-row strip of the pivot block is held in
// registers (lane j = column j): nine right-looking steps turn it into X = L^-1 [D | R] -- L^T in the pivot lanes, the
// columns of the factor below it in the others.  Lane layouts (the two 9-lane slots alternate between pivot and next block):
//   chain A: slot a 0..8 | slot b 9..17 | speed/bias 0 18..26 | poses 0..5 27..62 | rhs 63
//   chain B: slot a 0..8 | slot b 9..17 | poses 5..10 18..53 | rhs 54
// tools/proto_chain.py is the NumPy statement of the same scheme (fronts, fill, back-substitution).
// (DN = 90 dense dims in DNT = 6 tiles per dimension; the chains' X rows, XROWS_A and XROWS_B of stride XLD, in dense
// coordinates: ba_step_layout.h)
constexpr int CHOL_MIN_WAVES = 2;
// position in a chain's X row of dense tile column J (J = 3 is not in chain A's rows, J = 0 not in chain B's)
__device__ __forceinline__ constexpr int xcol(int ch, int J) { return ch == 0 ? 16 * (J > 3 ? J - 1 : J) : 16 * (J - 1); }
// row I of tile t of the tile-major lower storage (t = I (I + 1) / 2 + J)
__device__ __forceinline__ constexpr int tile_row(int t) { return t < 1 ? 0 : t < 3 ? 1 : t < 6 ? 2 : t < 10 ? 3 : t < 15 ? 4 : 5; }

__device__ __forceinline__ int chain_frame(int ch, int b) { return ch == 0 ? 1 + b : 10 - b; }
// cam index of the column of `lane` in block b of chain ch; NC = rhs, -1 = none
__device__ __forceinline__ int chain_col(int ch, int b, int lane) {
  if (lane < 18) {
    const int ds = (b & 1) ? 9 : 0;                       // lanes of the pivot block
    const int f = chain_frame(ch, b);
    const int fr = (lane >= ds && lane < ds + 9) ? f : (ch == 0 ? f + 1 : f - 1);
    return 15 * fr + 6 + (lane < 9 ? lane : lane - 9);
  }
  if (ch == 0) {
    if (lane < 27) return 6 + (lane - 18);
    if (lane < 63) return 15 * ((lane - 27) / 6) + (lane - 27) % 6;
    return NC;
  }
  if (lane < 54) return 15 * (5 + (lane - 18) / 6) + (lane - 18) % 6;
  return lane == 54 ? NC : -1;
}
// dense index of a cam dim (NC = rhs), -1 for the speed/bias blocks the chains eliminate
__device__ __forceinline__ int cam2dense(int c) {
  if (c < 0) return -1;
  if (c == NC) return DN;
  const int v = cam2vis(c);
  if (v >= 0) return v;
  if (c < 15) return 72 + (c - 6);
  return (c >= 81 && c < 90) ? c : -1;
}
__device__ __forceinline__ int dense2cam(int d) { return d < NV ? vis2cam(d) : (d < 81 ? 6 + (d - 72) : d); }
// dense index of lane `lane` of a chain's X rows (the slot lanes hold speed/bias 5 in the chain's last block only; in the
// other blocks their X entries are stored as zeros)
__device__ __forceinline__ int chain_dense(int ch, int lane) {
  if (lane < 18) {
    const bool s5 = ch == 0 ? lane < 9 : lane >= 9;       // chain A ends with its next block in slot a, chain B in slot b
    return s5 ? 81 + (lane < 9 ? lane : lane - 9) : -1;
  }
  return cam2dense(chain_col(ch, 0, lane));
}

// ---- the phases of chol_body, in its order.  wv is the wave's ROLE (0, 1: the chains; 2, 3: their partners), see chol_body.
// One register array, two tenants, handed from phase to phase by reference: the chain waves keep X of every block for the
// back-substitution (Xs(b, k) = U[9 b + k]), the partner waves their tiles of the dense system (11 or 10 tiles x 4 = U[0..43]).
#define Xs(b, k) U[9 * (b) + (k)]

// scale, diagonal and a zero solution to LDS; the flags; X (both chains' rows, XA | XBm) starts at zero
__device__ __forceinline__ void chol_init(const double* gscale, const double* gdiag, double* scv, double* dgv, double* ycam, int* flag, double* X) {
  const int tid = threadIdx.x, T = CHOL_THREADS;
  for (int c = tid; c < 176; c += T) { scv[c] = c < NC ? gscale[c] : 0.0; dgv[c] = c < NC ? gdiag[c] : 1.0; ycam[c] = 0.0; }
  if (tid < 4) flag[tid] = 0;
  // the columns of the X rows no chain lane writes, and rows 45..47 of chain B (K padding)
  for (int i = tid; i < (XROWS_A + XROWS_B) * XLD; i += T) X[i] = 0.0;
}

// waves 0, 1: chain ch eliminates its speed/bias blocks; X of block b to U for the way back, to XA / XBm for the partner waves,
// who are told through flag[1 + ch]; 1 / L_kk to rsL
__device__ __forceinline__ void chol_chain_forward(const int wv, const int lane, const double* Hcc, const double* gc, const double* scv,
                                                   const double* dgv, const double mu, double* XA, double* XBm, double* rsL, int* flag,
                                                   double (&U)[45]) {
  {
    const int ch = wv, nblk = ch == 0 ? 4 : 5;
    double* Xout = ch == 0 ? XA : XBm;
    const int xd = chain_dense(ch, lane);                 // the lane's X entries go to dense column xd (none: -1)
    const int xp = xd < 0 ? -1 : xcol(ch, xd >> 4) + (xd & 15);
    bool bad = false;
    // original strip of block b: H~[pivot rows][lane's column]; nine independent loads per lane
    auto load_strip = [&](int b, double (&raw)[9]) {
      const int col = chain_col(ch, b, lane);
      const int f = chain_frame(ch, b);
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const int r = 15 * f + 6 + i;
        raw[i] = 0.0;
        if (col == NC) raw[i] = gc[r];
        else if (col >= 0) raw[i] = Hcc[col > r ? tri(col, r) : tri(r, col)];
      }
    };
    double rawn[9];
    load_strip(0, rawn);
#pragma unroll
    for (int b = 0; b < 5; ++b) {
      if (b < nblk) {
        const int ds = (b & 1) ? 9 : 0, ns = 9 - ds;
        const int col = chain_col(ch, b, lane);
        const int f = chain_frame(ch, b);
        double R[9];
        {
          const double scol = col == NC ? 1.0 : (col >= 0 ? scv[col] : 0.0);
#pragma unroll
          for (int i = 0; i < 9; ++i) {
            const int r = 15 * f + 6 + i;
            R[i] = rawn[i] * (scv[r] * scol);
            if (col == r) R[i] += mu * dgv[r] * dgv[r];
          }
        }
        if (b + 1 < nblk) load_strip(b + 1, rawn);     // in flight during this block's elimination
        if (b > 0) {
          // fill from the previous block: R[i][j] -= sum_k X[k][pivot lane i] X[k][j]; the lanes of the previous pivot slot
          // now hold the NEW next block, which the previous block did not touch
          const bool fresh = lane >= ns && lane < ns + 9;
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            const double xk = fresh ? 0.0 : Xs(b - 1, k);
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] -= readlane_f64(Xs(b - 1, k), ds + i) * xk;
          }
        }
        // nine right-looking steps; the row scaling by 1 / sqrt(pivot) is applied at the end (off the dependent chain)
        double piv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const double pk = readlane_f64(R[k], ds + k);
          piv[k] = pk;
          if (!(pk > 0.0)) bad = true;
          double rinv = __builtin_amdgcn_rcp(pk);
          rinv = fma(rinv, fma(-pk, rinv, 1.0), rinv);
          rinv = fma(rinv, fma(-pk, rinv, 1.0), rinv);
          const double fj = R[k] * rinv;
#pragma unroll
          for (int i = k + 1; i < 9; ++i) R[i] -= readlane_f64(R[i], ds + k) * fj;
        }
        const bool dcol = cam2dense(col) >= 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          // 1 / sqrt(pivot) by v_rsq_f64 + two Newton steps (an IEEE sqrt and divide are ~25 dependent instructions)
          double rs = __builtin_amdgcn_rsq(piv[k]);
          rs = rs * fma(-0.5 * piv[k] * rs, rs, 1.5);
          rs = rs * fma(-0.5 * piv[k] * rs, rs, 1.5);
          if (lane == 0) rsL[(5 * ch + b) * 9 + k] = rs;
          const double xv = R[k] * rs;
          Xs(b, k) = col >= 0 ? xv : 0.0;
          if (xp >= 0) Xout[(9 * b + k) * XLD + xp] = dcol ? xv : 0.0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) __hip_atomic_store(&flag[1 + ch], b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    if (bad && lane == 0) flag[0] = 1;
  }
}

// waves 2, 3: the dense system assembled in U and the chains' X^T X taken off it on the matrix cores, as their rows arrive
__device__ __forceinline__ void chol_partner_assemble(const int wv, const int lane, const double* Hcc, const double* gc, const double* sacc,
                                                      const double* scv, const double* dgv, const double mu, const double* XA,
                                                      const double* XBm, int* flag, double (&U)[45]) {
  {
    // partner waves: the dense system in registers, tile t = (I, J) of the tile-major lower storage -- wave 2 the even
    // tiles, wave 3 the odd ones.  Each chain's product is summed from zero on the matrix cores, K-step by K-step as its X
    // rows are finished, and then subtracted: (H~ - P_A) - P_B.  The K-steps, the products and the roundings of every
    // entry are those of the lane-coordinate products this replaced, whichever tile the entry lands in: the same bits.
    // The entries of H~ are loaded once chain A is done, while chain B eliminates its last block (held from the start,
    // they would not fit in the registers next to the accumulators).
    const int m = lane & 15, kk = lane >> 4;
    // entry (r, c) of H~ before the chains: (Hcc - Schur) in the scaled space + mu D^2 (speed/bias rows: no Schur term),
    // the rhs row (g - Schur) scaled; the rhs diagonal and the padding rows are an identity (never a pivot).  Diagonal
    // tiles are full squares: (r, c) and (c, r) get the same bits.
    auto h0 = [&](int r, int c) -> double {
      if (r < c) { const int t = r; r = c; c = t; }
      if (r > DN || c == DN) return r == c ? 1.0 : 0.0;
      const int cc = dense2cam(c);
      if (r == DN) return (gc[cc] - (c < NV ? sacc[tri(NV, c)] : 0.0)) * scv[cc];
      const int cr = dense2cam(r);
      double v = Hcc[cr >= cc ? tri(cr, cc) : tri(cc, cr)];
      if (r < NV) v -= sacc[tri(r, c)];
      v *= scv[cr] * scv[cc];
      if (r == c) v += mu * dgv[cr] * dgv[cr];
      return v;
    };
    const int p = __builtin_amdgcn_readfirstlane(wv - 2);
    v4d hs[11], acc[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) acc[i] = v4d{0, 0, 0, 0};
    int have = 0;
#pragma unroll 1
    for (int ks = 0; ks < XROWS_A / 4; ++ks) {          // chain A: dense tile columns 0, 1, 2, 4, 5
      const int need = min(4, (4 * ks + 3) / 9 + 1);
      while (have < need) {
        have = __hip_atomic_load(&flag[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (have >= need) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      }
      const double* row = XA + (4 * ks + kk) * XLD + m;
      double x[6];
#pragma unroll
      for (int J = 0; J < 6; ++J) x[J] = J == 3 ? 0.0 : row[xcol(0, J)];
#pragma unroll
      for (int t = 0; t < 21; ++t) {
        const int I = tile_row(t), J = t - I * (I + 1) / 2;
        if ((t & 1) != p || I == 3 || J == 3) continue;
        acc[t >> 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[I], x[J], acc[t >> 1], 0, 0, 0);
      }
    }
    // the assembled entries minus chain A's product
#pragma unroll
    for (int t = 0; t < 21; ++t) {
      if ((t & 1) != p) continue;
      const int I = tile_row(t), J = t - I * (I + 1) / 2;
      const int r = 16 * I + kk, c = 16 * J + m;
      const v4d h = v4d{h0(r, c), h0(r + 4, c), h0(r + 8, c), h0(r + 12, c)};
      hs[t >> 1] = (I == 3 || J == 3) ? h : h - acc[t >> 1];
      acc[t >> 1] = v4d{0, 0, 0, 0};
    }
    if (p) hs[10] = v4d{0, 0, 0, 0};
    have = 0;
#pragma unroll 1
    for (int ks = 0; ks < XROWS_B / 4; ++ks) {          // chain B: dense tile columns 1..5
      const int need = min(5, (4 * ks + 3) / 9 + 1);
      while (have < need) {
        have = __hip_atomic_load(&flag[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (have >= need) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      }
      const double* row = XBm + (4 * ks + kk) * XLD + m;
      double x[6];
#pragma unroll
      for (int J = 0; J < 6; ++J) x[J] = J == 0 ? 0.0 : row[xcol(1, J)];
#pragma unroll
      for (int t = 0; t < 21; ++t) {
        const int I = tile_row(t), J = t - I * (I + 1) / 2;
        if ((t & 1) != p || J == 0) continue;
        acc[t >> 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[I], x[J], acc[t >> 1], 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < 11; ++i) {
      const v4d h = hs[i] - acc[i];
      U[4 * i] = h.x; U[4 * i + 1] = h.y; U[4 * i + 2] = h.z; U[4 * i + 3] = h.w;
    }
  }
}

// the dense system from the partner waves' registers into LDS
__device__ __forceinline__ void chol_spill(const int wv, const int lane, double* S, const double (&U)[45]) {
  if (wv >= 2) {
    const int p = __builtin_amdgcn_readfirstlane(wv - 2);
    const int m = lane & 15, kk = lane >> 4;
#pragma unroll
    for (int t = 0; t < 21; ++t) {
      if ((t & 1) != p) continue;
      double* St = S + (t << 8);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int r = kk + 4 * v;
        // (rhs, rhs) is not part of the system: it keeps its unit diagonal
        St[tsw(r, m)] = (t == 20 && r == DN - 80 && m == DN - 80) ? 1.0 : U[4 * (t >> 1) + v];
      }
    }
  }
}

// waves 0, 1: the chains backwards, from the dense solution in ycam; every block's nine entries of the solution to ycam
__device__ __forceinline__ void chol_chain_backward(const int wv, const int lane, double* ycam, const double* rsL, const double (&U)[45]) {
  if (wv < 2) {
    const int ch = wv, nblk = ch == 0 ? 4 : 5;
#pragma unroll
    for (int b = 4; b >= 0; --b) {
      if (b < nblk) {
        const int ds = (b & 1) ? 9 : 0;
        const int col = chain_col(ch, b, lane);
        const int f = chain_frame(ch, b);
        const bool pivl = lane >= ds && lane < ds + 9;
        // t = z - sum over the other columns of X[.][j] y_j
        const double cf = col == NC ? 1.0 : ((col < 0 || pivl) ? 0.0 : -ycam[col]);
        double t[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) t[k] = wave_sum_dpp(Xs(b, k) * cf);
        // L^T y = t with L^T[k][j] = X[k][pivot lane j]
#pragma unroll
        for (int j = 8; j >= 0; --j) {
          const double yj = t[j] * rsL[(5 * ch + b) * 9 + j];
#pragma unroll
          for (int k = 0; k < j; ++k) t[k] -= readlane_f64(Xs(b, k), ds + j) * yj;
          t[j] = yj;
        }
        if (lane == 0) {
#pragma unroll
          for (int j = 0; j < 9; ++j) ycam[15 * f + 6 + j] = t[j];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      }
    }
  }
}

// outputs: S_c y_c for the landmark back-substitution, the Gauss-Newton step of the cam dims and its share of the dogleg sums
__device__ __forceinline__ void chol_outputs(const DevBatch& B, const int w, const double* ycam, const double* scv, const double* dgv,
                                             const double* ggrad, double* ggn, double* red) {
  const int tid = threadIdx.x, T = CHOL_THREADS;
  double a2 = 0.0, a3 = 0.0;
  double* ycs = B.ycs + (size_t)w * 176;
  for (int c = tid; c < 176; c += T) {
    double u = 0.0;
    if (c < NC) {
      const double y = ycam[c];
      u = scv[c] * y;
      const double gnv = -dgv[c] * y;
      ggn[c] = gnv;
      a2 += gnv * gnv;
      a3 += ggrad[c] * gnv;
    }
    ycs[c] = u;
  }
  a2 = block_sum(a2, red);
  a3 = block_sum(a3, red);
  if (tid == 0) { B.sx[(size_t)w * 8] = a2; B.sx[(size_t)w * 8 + 1] = a3; }
}
#undef Xs

__device__ __forceinline__ void chol_body(const DevBatch& B, const int w, double* sm) {
  const int tid = threadIdx.x, T = CHOL_THREADS;
  // Two work-groups share a CU, and the serial work of this kernel sits in "wave 0" and "wave 1" (the chains, the diagonal
  // tiles): with the same roles in both, the two chains of the two windows would share one SIMD while the SIMDs of the
  // partner waves idle.  Work-groups b and b + 256 are the ones that normally meet on a CU (round-robin over 8 XCDs x 32
  // CUs): every second group of 256 rotates its roles by two waves.
  const int lane = tid & 63, wv = ((tid >> 6) + ((blockIdx.x >> 8) & 1) * 2) & 3;
  TrState* tr = &B.tr[w];
  if (tr->status != 0 || tr->reuse != 0 || B.path[w] != 0) return;
  count_active(B, 1);
  // regions and tenants: CholLayoutT (ba_step_layout.h).  The chains' X rows XA | XBm and the dense system S share the first region.
  const CholLayoutT<double*> L = chol_layout_at(sm);
  double *XA = L.XA.at, *XBm = L.XBm.at, *S = L.S.at, *scv = L.scv.at, *dgv = L.dgv.at, *ycam = L.ycam.at, *yv = L.yv.at, *isd = L.isd.at;
  double *Linv = L.Linv.at, *red = L.red.at, *rsL = L.rsL.at;
  int* flag = (int*)L.flag.at;

  const size_t fb = (size_t)w * B.nfull;
  const double* gscale = B.scale + fb;
  const double* gdiag = B.diag + fb;
  const double* ggrad = B.grad + fb;
  double* ggn = B.gn + fb;
  const double* Hcc = B.Hcc + (size_t)w * NCP;
  const double* gc = B.gc + (size_t)w * NC;
  const double* sacc = B.sacc + (size_t)w * SACC_N;
  const double mu = tr->mu;
  chol_init(gscale, gdiag, scv, dgv, ycam, flag, XA);
  __syncthreads();   // scv, dgv complete; X and the flags are zero
  VPL_STAMP(B, w, 8);
  // the two chains (waves 0, 1); the dense system assembled and the chains' X^T X taken off it (waves 2, 3)
  double U[45];
#pragma unroll
  for (int i = 0; i < 45; ++i) U[i] = 0.0;
  if (wv < 2) chol_chain_forward(wv, lane, Hcc, gc, scv, dgv, mu, XA, XBm, rsL, flag, U);
  else chol_partner_assemble(wv, lane, Hcc, gc, sacc, scv, dgv, mu, XA, XBm, flag, U);
  __syncthreads();   // the X rows are dead: their space becomes the dense system
  VPL_STAMP(B, w, 9);
  chol_spill(wv, lane, S, U);
  __syncthreads();   // S complete
  VPL_STAMP(B, w, 10);
  // left-looking tile Cholesky of the dense system (tile_cholesky of ba_solve.h, 6 tile columns, 4 waves); the rhs row rides along
  if (!tile_cholesky(S, Linv, isd, flag, DNT, DN, CHOL_THREADS / 64, lane, wv, nullptr)) {
    // LINEAR_SOLVER_FAILURE: the retry with a larger mu is k_solve's loop
    if (tid == 0) B.path[w] = 2;
    return;
  }
  VPL_STAMP(B, w, 11);
  // back substitution L^T y = z of the dense part
  tile_back_substitute(S, isd, yv, DNT, DN, tid, T, lane, wv);
  for (int d = tid; d < DN; d += T) ycam[dense2cam(d)] = yv[d];
  __syncthreads();   // the dense solution is in ycam
  VPL_STAMP(B, w, 12);
  chol_chain_backward(wv, lane, ycam, rsL, U);
  __syncthreads();   // ycam complete
  chol_outputs(B, w, ycam, scv, dgv, ggrad, ggn, red);
  VPL_STAMP(B, w, 13);
}
__global__ __launch_bounds__(CHOL_THREADS, CHOL_MIN_WAVES) void k_chol(DevBatch B) {
  extern __shared__ double sm[];
  chol_body(B, ordered_window(B), sm);
}
inline size_t chol_smem() { return chol_lds_bytes(); }

// ---------------------------------------------------------------------------------------------------------------------
// k_back : landmark back-substitution y_l = A_l^-1 S_l (g_l - W_l S_c y_c), then DoglegStrategy::ComputeTraditionalDoglegStep,
// the model cost change and the candidate x (+) delta -- for a window that re-uses the Gauss-Newton step of a rejected
// iteration only the latter.
// ---------------------------------------------------------------------------------------------------------------------
// FUSED (k_step): k_solve runs AFTER this body and is the flag's last reader -- a window of the general path leaves without
// touching B.path, k_solve takes a one-iteration flag down itself.
// the phase of back_body that reads: track start frames, S_c y_c in vis order (W's column order), the cam part of the Gauss-Newton step
__device__ __forceinline__ void back_load(const DevBatch& B, const int w, const int nP, const int nL, const double* ggn, int* pSt, int* lSt,
                                          double* uc, double* lgn) {
  const int tid = threadIdx.x, T = BACK_THREADS;
  for (int p = tid; p < nP; p += T) pSt[p] = B.pt_start[(size_t)w * B.maxP + p];
  for (int l = tid; l < nL; l += T) lSt[l] = B.ln_start[(size_t)w * B.maxL + l];
  for (int c = tid; c < 176; c += T) uc[c] = c < NV ? B.ycs[(size_t)w * 176 + vis2cam(c)] : 0.0;   // vis order: W's column order
  for (int c = tid; c < NC; c += T) lgn[c] = ggn[c];
}

template <bool FUSED = false>
__device__ __forceinline__ void back_body(const DevBatch& B, const int w, double* sm) {
  const int tid = threadIdx.x, T = BACK_THREADS;
  TrState* tr = &B.tr[w];
  if (tr->status != 0) return;
  const int path = B.path[w];
  if (path != 0) {                       // k_solve does / did this window's whole step
    if (FUSED) return;
    __syncthreads();                     // (everybody has read the flag)
    if (tid == 0 && path == 2) B.path[w] = 0;
    return;
  }
  const int nP = B.nP[w], nL = B.nL[w];
  // regions: BackLayoutT (ba_step_layout.h); no region changes its tenant
  const BackLayoutT<double*> L = back_layout_at(sm, B.maxP, B.maxL, B.nfull);
  double *uc = L.uc.at, *lrhs = L.lrhs.at, *lgn = L.lgn.at, *gdelta = L.gdelta.at, *red = L.red.at;
  int *pSt = (int*)L.pSt.at, *lSt = (int*)L.lSt.at;
  double* ggn = B.gn + (size_t)w * B.nfull;
  const bool reuse0 = tr->reuse != 0;
  count_active(B, reuse0 ? 2 : 1);
  VPL_STAMP(B, w, 5);
  if (!reuse0) {
    const double mu = tr->mu;
    back_load(B, w, nP, nL, ggn, pSt, lSt, uc, lgn);
    __syncthreads();   // pSt, lSt, uc and the cam part of lgn complete
    double a2 = 0.0, a3 = 0.0;
    back_substitute_points<T, 4, false>(B, w, mu, uc, pSt, lgn, a2, a3);
    back_substitute_lines<T, 5, false>(B, w, uc, lSt, lrhs, lgn, a2, a3);
    a2 = block_sum(a2, red);
    a3 = block_sum(a3, red);
    if (tid == 0) {
      tr->a2 = a2 + B.sx[(size_t)w * 8];        // camera part from k_chol
      tr->a3 = a3 + B.sx[(size_t)w * 8 + 1];
      tr->reuse = 1;   // DoglegStrategy::ComputeStep sets reuse_ = true
    }
    __syncthreads();   // lgn complete, tr written
  }
  VPL_STAMP(B, w, 6);
  dogleg_step_and_candidate<T>(B, w, reuse0, lgn, gdelta, red);
}
#ifndef VPL_BACK_WAVES
#define VPL_BACK_WAVES 2          // A/B switch: waves per SIMD the register allocation of k_back is held to
#endif
__global__ __launch_bounds__(BACK_THREADS, VPL_BACK_WAVES) void k_back(DevBatch B) {
  extern __shared__ double sm[];
  back_body(B, ordered_window(B), sm);
}
inline size_t back_smem(int maxP, int maxL) { return back_lds_bytes(maxP, maxL); }

// ---------------------------------------------------------------------------------------------------------------------
// k_step : the three bodies above, one after the other, for the window of this work-group -- one launch per step.
// ---------------------------------------------------------------------------------------------------------------------
// Data flows from a window to the same window only, so the two device-wide joins of the three-launch form are work-group
// barriers here.  A body hands over through HBM exactly as between launches (B.path, sacc, ycs, sx, the scale / diag / grad
// vectors, tr: written by a few lanes, read by all): __syncthreads() is a release / acquire pair at work-group scope, which
// completes the stores of every wave before any wave of the work-group goes on to load.  One LDS block, the largest of the
// three layouts of ba_step_layout.h (step_lds_bytes); every body carves it for itself and initialises what it reads of it.  The general path follows this kernel (k_step -> k_solve ->
// k_cost), see back_body<true>.
static_assert(SCHUR_THREADS == CHOL_THREADS && CHOL_THREADS == BACK_THREADS, "k_step runs the three bodies with one work-group shape");
template <int NTC, bool MIXED>
__global__ __launch_bounds__(SCHUR_THREADS, 2) void k_step(DevBatch B) {
  extern __shared__ double sm[];
  empty_next_order(B);
  const int w = ordered_window(B);
  schur_body<NTC, MIXED>(B, w, sm);
  __syncthreads();
  chol_body(B, w, sm);
  __syncthreads();
  back_body<true>(B, w, sm);
}
inline size_t step_smem(int maxP, int maxL, int ntc = 5) { return step_lds_bytes(maxP, maxL, max_schur_ksteps(maxP, maxL), ntc); }

}  // namespace vpl
