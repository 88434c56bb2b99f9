// Loop detection (vpl_ld_*): PoseGraph::detectLoop (pose_graph/src/pose_graph.cpp:304-386) for n_db keyframe databases that
// share one vocabulary.  Per call and database, in the reference's order:
//   k_ld_descend  transform of every descriptor (TemplatedVocabulary.h:1217-1258) on the flat vocabulary of ld_vocab.h: 16 lanes
//                 per descriptor take the children of a step side by side (a strided loop for wider nodes) and reduce the key
//                 (distance << 32 | child position), so the first child wins a tie without a branch
//   k_ld_bag      the bag of words (:1065-1121, BowVector::normalize): the word ids sorted in LDS, runs collapsed, the weight of
//                 a run added once per occurrence (every addend of a run is the same leaf weight, so the descriptor order does not
//                 enter), the L1 norm summed by one lane in ascending word id, every value divided by it
//   k_ld_scatter  the query's position + 1 into a dense table by word id
//   k_ld_score    queryL1 (TemplatedDatabase.h:656-723): a wave per stored entry gathers the table at the entry's sorted word ids,
//                 64 at a time, and adds the hits in lane order = ascending word id, as the reference's walk over the query does
//   k_ld_decide   the best max_results by (raw score, entry id), -raw / 2, the rules of pose_graph.cpp:348-384; clears the table
//                 with the scatter's own list; db.add: the bag goes behind the stored ones -- only when no database of the call
//                 ran out of room
// All of it is f64 without a product; no sum is a tree, no atomics: two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vpl {

constexpr int LD_MAX_KEYPOINTS = 8192;   // a frame's word ids are sorted in LDS
constexpr int LD_MAX_RESULTS = 4;        // ids / scores of vpl_ld_result
constexpr int LD_LANES = 16;             // lanes per descriptor in the descent
constexpr int LD_EMPTY = 0x7fffffff;     // sorts behind every word id

struct LdVocabDev {
  int nFlat, nWords, weighting;
  const int *childBegin, *childCount, *word;   // [nFlat]
  const unsigned long long* desc;              // [nFlat][4]
  const double* wordWeight;                    // [nWords]
};

struct LdOut {   // one database's share of the copy back
  double scores[LD_MAX_RESULTS];
  int ids[LD_MAX_RESULTS];
  int loop_index, n_results, n_words, entry;
  int flag, have;   // 1: no keyframe left, 2: pool too small | entries / pool words in use
};

struct LdBatch {
  LdVocabDev V;
  int nDb, MK, maxKf, pool, maxResults, recent, doQuery;
  double neighbourScore, loopScore;
  const unsigned long long* brief;   // [nDb][MK][4]
  const int *counts, *frameIndex;    // [nDb]
  int* dWord;                        // [nDb][MK] word of every descriptor, -1 = none (stop word, empty vocabulary)
  int* qWord; double* qVal; int* qN; // the new bag [nDb][MK], its length [nDb]
  int* flag;                         // [nDb]
  int* table;                        // [nDb][nWords] position in the query + 1
  int *nEntries, *poolUsed;          // [nDb]
  int* entryOff;                     // [nDb][maxKf + 1]
  int* poolWord; double* poolVal;    // [nDb][pool]
  double* raw; int* hit;             // [nDb][maxKf]
  LdOut* out;                        // [nDb]
};

__device__ inline int ld_dist(unsigned long long a0, unsigned long long a1, unsigned long long a2, unsigned long long a3,
                              const unsigned long long* d) {
  return __builtin_popcountll(a0 ^ d[0]) + __builtin_popcountll(a1 ^ d[1]) + __builtin_popcountll(a2 ^ d[2]) + __builtin_popcountll(a3 ^ d[3]);
}

__global__ __launch_bounds__(256) void k_ld_descend(LdBatch B) {
  const int db = blockIdx.y, cnt = min(B.counts[db], B.MK);
  if ((int)blockIdx.x * (256 / LD_LANES) >= cnt) return;   // (the whole work-group; a skipped database has cnt < 0)
  const int i = blockIdx.x * (256 / LD_LANES) + (threadIdx.x / LD_LANES), l = threadIdx.x % LD_LANES;
  const bool valid = i < cnt;
  const LdVocabDev& V = B.V;
  unsigned long long q0 = 0, q1 = 0, q2 = 0, q3 = 0;
  if (valid) {
    const unsigned long long* q = B.brief + ((size_t)db * B.MK + i) * 4;
    q0 = q[0]; q1 = q[1]; q2 = q[2]; q3 = q[3];
  }
  int cur = 0;
  for (;;) {   // every lane of the wave takes every step, so the shuffles below never read a lane that has left
    const int n = valid ? V.childCount[cur] : 0;
    if (__ballot(n > 0) == 0) break;
    const int b = V.childBegin[cur];
    unsigned long long best = ~0ull;
    for (int j = l; j < n; j += LD_LANES) {
      const unsigned long long key = (unsigned long long)ld_dist(q0, q1, q2, q3, V.desc + (size_t)(b + j) * 4) << 32 | (unsigned)j;
      best = key < best ? key : best;
    }
    for (int m = LD_LANES / 2; m >= 1; m >>= 1) {
      const unsigned long long o = __shfl_xor(best, m, LD_LANES);
      best = o < best ? o : best;
    }
    if (n > 0) cur = b + (int)(best & 0xffffffffull);
  }
  if (valid && l == 0) {
    int w = V.nFlat > 1 ? V.word[cur] : -1;
    if (w >= 0 && !(V.wordWeight[w] > 0)) w = -1;   // a stop word
    B.dWord[(size_t)db * B.MK + i] = w;
  }
}

// dynamic LDS: double val[P] | int s[P] | int hp[P + 1], P = the power of two that holds MK
__global__ __launch_bounds__(256) void k_ld_bag(LdBatch B, int P) {
  extern __shared__ double ld_smem[];
  __shared__ int part[256];
  __shared__ int sM, sU;
  __shared__ double sNorm;
  const int db = blockIdx.x, tid = threadIdx.x;
  if (B.counts[db] < 0) return;
  const int n = min(B.counts[db], B.MK);
  double* val = ld_smem;
  int* s = (int*)(val + P);
  int* hp = s + P;
  int P2 = 1;
  while (P2 < n) P2 <<= 1;   // (<= P)
  const int* dw = B.dWord + (size_t)db * B.MK;
  for (int i = tid; i < P2; i += 256) { const int w = i < n ? dw[i] : -1; s[i] = w < 0 ? LD_EMPTY : w; }
  if (tid == 0) { sM = 0; sU = 0; }
  __syncthreads();
  for (int k = 2; k <= P2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P2; i += 256) {
        const int x = i ^ j;
        if (x > i) {
          const int a = s[i], b = s[x];
          if (((i & k) == 0) ? (a > b) : (a < b)) { s[i] = b; s[x] = a; }
        }
      }
      __syncthreads();
    }
  // run heads: rank by a scan over per-thread chunks
  const int chunk = (P2 + 255) / 256, lo = min(tid * chunk, P2), hi = min(lo + chunk, P2);
  int heads = 0;
  for (int i = lo; i < hi; ++i) {
    const int w = s[i];
    if (w != LD_EMPTY) {
      heads += (i == 0 || s[i - 1] != w) ? 1 : 0;
      if (i == P2 - 1 || s[i + 1] == LD_EMPTY) sM = i + 1;   // one element at most
    }
  }
  part[tid] = heads;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int add = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  int rank = part[tid] - heads;
  if (tid == 255) sU = part[255];
  for (int i = lo; i < hi; ++i) {
    const int w = s[i];
    if (w != LD_EMPTY && (i == 0 || s[i - 1] != w)) hp[rank++] = i;
  }
  __syncthreads();
  const int U = sU;
  if (tid == 0) hp[U] = sM;
  __syncthreads();
  const bool accumulate = B.V.weighting == 0 || B.V.weighting == 1;   // TF_IDF, TF: addWeight; IDF, BINARY: addIfNotExist
  int* qw = B.qWord + (size_t)db * B.MK;
  double* qv = B.qVal + (size_t)db * B.MK;
  for (int r = tid; r < U; r += 256) {
    const int w = s[hp[r]], c = hp[r + 1] - hp[r];
    const double wt = B.V.wordWeight[w];
    double v = wt;
    if (accumulate)
      for (int k = 1; k < c; ++k) v += wt;
    val[r] = v;
    qw[r] = w;
  }
  __syncthreads();
  if (tid == 0) {
    double norm = 0.0;
    for (int r = 0; r < U; ++r) norm += fabs(val[r]);
    sNorm = norm;
    B.qN[db] = U;
    B.flag[db] = B.nEntries[db] >= B.maxKf ? 1 : (B.poolUsed[db] + U > B.pool ? 2 : 0);
  }
  __syncthreads();
  const double norm = sNorm;
  for (int r = tid; r < U; r += 256) qv[r] = norm > 0.0 ? val[r] / norm : val[r];
}

__global__ __launch_bounds__(256) void k_ld_scatter(LdBatch B) {
  const int db = blockIdx.y;
  if (B.counts[db] < 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < B.qN[db]) B.table[(size_t)db * B.V.nWords + B.qWord[(size_t)db * B.MK + i]] = i + 1;
}

__global__ __launch_bounds__(256) void k_ld_score(LdBatch B) {
  const int db = blockIdx.y;
  if (B.counts[db] < 0) return;
  const int lane = threadIdx.x & 63, e = blockIdx.x * 4 + (threadIdx.x >> 6), nE = B.nEntries[db];
  if (e >= nE) return;   // (the whole wave)
  const int maxId = B.frameIndex[db] - B.recent;
  if (!(e < maxId || maxId == -1 || e == nE - 1)) {
    if (lane == 0) B.hit[(size_t)db * B.maxKf + e] = 0;
    return;
  }
  const int* off = B.entryOff + (size_t)db * (B.maxKf + 1) + e;
  const int o0 = off[0], o1 = off[1];
  const int* pw = B.poolWord + (size_t)db * B.pool;
  const double* pv = B.poolVal + (size_t)db * B.pool;
  const int* table = B.table + (size_t)db * B.V.nWords;
  const double* qv = B.qVal + (size_t)db * B.MK;
  double sum = 0.0;
  int any = 0;
  for (int base = o0; base < o1; base += 64) {
    const int idx = base + lane;
    double v = 0.0;
    bool h = false;
    if (idx < o1) {
      const int t = table[pw[idx]];
      if (t) {
        const double q = qv[t - 1], d = pv[idx];
        v = fabs(q - d) - fabs(q) - fabs(d);
        h = true;
      }
    }
    unsigned long long m = __ballot(h);
    any |= m != 0;
    const int vlo = __double2loint(v), vhi = __double2hiint(v);
    while (m) {   // the hits in lane order: ascending word id
      const int src = __builtin_ctzll(m);
      sum += __hiloint2double(__builtin_amdgcn_readlane(vhi, src), __builtin_amdgcn_readlane(vlo, src));
      m &= m - 1;
    }
  }
  if (lane == 0) { B.raw[(size_t)db * B.maxKf + e] = sum; B.hit[(size_t)db * B.maxKf + e] = any; }
}

__global__ __launch_bounds__(256) void k_ld_decide(LdBatch B) {
  __shared__ double rk[256];
  __shared__ int ri[256];
  __shared__ int selId[LD_MAX_RESULTS];
  __shared__ double selRaw[LD_MAX_RESULTS];
  const int db = blockIdx.x, tid = threadIdx.x;
  LdOut& O = B.out[db];
  if (B.counts[db] < 0) {
    if (tid == 0) {
      for (int k = 0; k < LD_MAX_RESULTS; ++k) { O.scores[k] = 0.0; O.ids[k] = -1; }
      O.loop_index = -1; O.n_results = 0; O.n_words = 0; O.entry = -1; O.flag = 0; O.have = B.nEntries[db];
    }
    return;
  }
  bool bad = false;
  for (int d = 0; d < B.nDb; ++d) bad |= B.counts[d] >= 0 && B.flag[d] != 0;
  const int nE = B.nEntries[db], used = B.poolUsed[db], U = B.qN[db];
  int nres = 0;
  if (B.doQuery) {
    const double* raw = B.raw + (size_t)db * B.maxKf;
    const int* hit = B.hit + (size_t)db * B.maxKf;
    for (int r = 0; r < B.maxResults; ++r) {
      double bk = 0.0;
      int bi = -1;
      for (int e = tid; e < nE; e += 256) {
        if (!hit[e]) continue;
        bool taken = false;
        for (int k = 0; k < r; ++k) taken |= selId[k] == e;
        if (taken) continue;
        const double v = raw[e];
        if (bi < 0 || v < bk) { bk = v; bi = e; }   // (ascending e: the smaller id stays on a tie)
      }
      rk[tid] = bk; ri[tid] = bi;
      __syncthreads();
      for (int d = 128; d >= 1; d >>= 1) {
        if (tid < d) {
          const int oi = ri[tid + d];
          const double ok = rk[tid + d];
          const int mi = ri[tid];
          if (oi >= 0 && (mi < 0 || ok < rk[tid] || (ok == rk[tid] && oi < mi))) { rk[tid] = ok; ri[tid] = oi; }
        }
        __syncthreads();
      }
      const int got = ri[0];
      if (tid == 0 && got >= 0) { selId[r] = got; selRaw[r] = rk[0]; }
      __syncthreads();
      if (got < 0) break;
      nres = r + 1;
    }
    int* table = B.table + (size_t)db * B.V.nWords;
    const int* qw = B.qWord + (size_t)db * B.MK;
    for (int i = tid; i < U; i += 256) table[qw[i]] = 0;
  }
  if (!bad) {   // db.add
    const int* qw = B.qWord + (size_t)db * B.MK;
    const double* qv = B.qVal + (size_t)db * B.MK;
    int* pw = B.poolWord + (size_t)db * B.pool + used;
    double* pv = B.poolVal + (size_t)db * B.pool + used;
    for (int i = tid; i < U; i += 256) { pw[i] = qw[i]; pv[i] = qv[i]; }
  }
  if (tid != 0) return;
  for (int k = 0; k < LD_MAX_RESULTS; ++k) { O.scores[k] = k < nres ? -selRaw[k] / 2.0 : 0.0; O.ids[k] = k < nres ? selId[k] : -1; }
  bool find = false;
  if (nres >= 1 && O.scores[0] > B.neighbourScore)
    for (int k = 1; k < nres; ++k) find |= O.scores[k] > B.loopScore;
  int loop = -1;
  if (find && B.frameIndex[db] > B.recent)
    for (int k = 0; k < nres; ++k)
      if (loop == -1 || (O.ids[k] < loop && O.scores[k] > B.loopScore)) loop = O.ids[k];
  O.loop_index = loop; O.n_results = nres; O.n_words = U; O.entry = bad ? -1 : nE;
  O.flag = B.flag[db]; O.have = B.flag[db] == 2 ? used : nE;
  if (!bad) {
    B.entryOff[(size_t)db * (B.maxKf + 1) + nE + 1] = used + U;
    B.nEntries[db] = nE + 1;
    B.poolUsed[db] = used + U;
  }
}

}  // namespace vpl
