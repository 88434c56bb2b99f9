// The staging arena of the bundle-adjustment context (vplines_ba.hip): one pinned host arena and one device arena, the copy
// kernel between the device arena and the batch's arrays, and the dry run that sizes them.  Knows nothing of vpl_ctx.
//   upload   : the host packs every array into the pinned arena, ONE hipMemcpyAsync moves it to the device arena, ONE kernel
//              (k_copy_segments) scatters the pieces into the batch's arrays;
//   download : one kernel gathers the result arrays into the device arena, ONE hipMemcpyAsync brings it to the pinned arena,
//              the host scatters into the caller's structs.
// Round 3 issued ~45 hipMemcpyAsync per upload and ~17 per download straight from / into pageable std::vectors and the
// caller's vpl_prior structs: each pageable copy above the runtime's staging threshold pins and unpins its pages (a kernel
// driver call that can quiesce the process's queues), which showed up as 26 ms instead of 1.4 in the solve leg of a
// 64-window call on the round-3 driver box.
// Through the arena go: the upload (ba_upload.h: vpl_ba_upload, vpl_ba_upload_chained and the upload inside every other window
// entry point), the chained upload's read-back of the resident block tables, vpl_ba_download and the prior fetch of
// vpl_ba_marginalize.  NOT through it: the result copies of the triangulation, onlyLineOpt and slide entry points
// (triangulate_impl, only_line_opt_impl, slide_window_impl), which still go into / come from heap vectors, i.e. pageable memory.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

struct CopySeg {
  const char* src;
  char* dst;
  unsigned bytes;
  unsigned u0;   // index of the segment's first 16-byte unit in the launch
};
static_assert(sizeof(CopySeg) == 24, "CopySeg layout");

// one thread per 16-byte unit; the segment of a unit by binary search over the (<= few thousand) prefix entries
__global__ __launch_bounds__(256) void k_copy_segments(const CopySeg* tab, int nseg, unsigned total_units) {
  for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < total_units; u += gridDim.x * 256u) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tab[mid].u0 <= u) lo = mid; else hi = mid - 1;
    }
    const CopySeg sg = tab[lo];
    const unsigned off = (u - sg.u0) * 16u;
    const unsigned rem = sg.bytes - off;
    const char* src = sg.src + off;
    char* dst = sg.dst + off;
    if (rem >= 16u && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
      *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    } else {   // tails and 4- / 8-byte aligned pieces (every array is made of 4- or 8-byte elements)
      const unsigned nb = rem < 16u ? rem : 16u;
      for (unsigned b = 0; b < nb; b += 4) *reinterpret_cast<uint32_t*>(dst + b) = *reinterpret_cast<const uint32_t*>(src + b);
    }
  }
}

template <typename T>
struct Span {   // a piece of the pinned arena with the few std::vector members the packing code uses
  T* p = nullptr;
  size_t n = 0;
  T& operator[](size_t i) const { return p[i]; }
  T* data() const { return p; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  T* begin() const { return p; }
  T* end() const { return p + n; }
};

// The arena's bound is never written down: a call runs its takes and segments once on a DRY stage, which only counts them,
// and reserves what that run used (stage_plan; the upload: upload_bound).  A take past the bound hands out host scratch and
// flags `overflow`, which stage_run refuses, so a wrong bound is an error and never a write past the arena.
struct Stage {
  char* h = nullptr;   // hipHostMalloc
  char* d = nullptr;   // hipMalloc
  size_t cap = 0, used = 0;
  std::vector<CopySeg> segs;
  unsigned units = 0;
  bool overflow = false;
  bool dry = false;                                  // sizing run: takes are empty pieces, nothing is allocated or written
  std::vector<std::unique_ptr<char[]>> spill;        // pieces taken past the bound

  hipError_t reserve(size_t need) {
    used = 0; segs.clear(); units = 0; overflow = false; spill.clear();
    if (need <= cap) return hipSuccess;
    release();
    const size_t want = need + need / 4 + (1u << 16);
    hipError_t e = hipHostMalloc((void**)&h, want, hipHostMallocDefault);
    if (e != hipSuccess) return e;
    e = hipMalloc((void**)&d, want);
    if (e != hipSuccess) return e;
    cap = want;
    return hipSuccess;
  }
  void release() {
    if (h) (void)hipHostFree(h);   // (the old arena is dropped either way)
    if (d) (void)hipFree(d);
    h = d = nullptr; cap = 0;
  }
  // what a reserve must cover for the takes and segments so far: the data, and the segment table stage_run appends
  size_t bound() const { return ((used + 63) & ~(size_t)63) + segs.size() * sizeof(CopySeg); }
  template <typename T>
  Span<T> take(size_t n) {   // uninitialised
    used = (used + 63) & ~(size_t)63;
    Span<T> sp;
    sp.n = n;
    if (!dry && used + n * sizeof(T) <= cap) sp.p = reinterpret_cast<T*>(h + used);
    else if (!dry) { overflow = true; spill.emplace_back(new char[n * sizeof(T) + 1]); sp.p = reinterpret_cast<T*>(spill.back().get()); }
    used += n * sizeof(T);
    return sp;
  }
  template <typename T>
  Span<T> take(size_t n, T fill) {
    Span<T> sp = take<T>(n);
    if (!dry) std::fill(sp.begin(), sp.end(), fill);
    return sp;
  }
  char* dev_of(const void* host_ptr) const { return d + (reinterpret_cast<const char*>(host_ptr) - h); }
  void seg(const void* src, void* dst, size_t bytes) {
    if (!bytes) return;
    CopySeg c{reinterpret_cast<const char*>(src), reinterpret_cast<char*>(dst), (unsigned)bytes, units};
    units += (unsigned)((bytes + 15) / 16);
    segs.push_back(c);
  }
  // upload: a piece of the arena (host address) to a device array
  template <typename T>
  void to_device(T* dev_dst, const T* host_src, size_t n) { seg(dev_of(host_src), dev_dst, n * sizeof(T)); }
  // download: a device array to a piece of the arena (host address)
  template <typename T>
  void from_device(T* host_dst, const T* dev_src, size_t n) { seg(dev_src, dev_of(host_dst), n * sizeof(T)); }
  template <typename T>
  void put(T* dev_dst, const Span<T>& src) { to_device(dev_dst, src.p, src.n); }
};

// sizes the arena by a dry run of `plan` (its takes and segments), reserves that, and runs `plan` on the arena
template <typename Plan>
static hipError_t stage_plan(Stage& S, const Plan& plan) {
  Stage dry;
  dry.dry = true;
  plan(dry);
  const hipError_t e = S.reserve(dry.bound());
  if (e == hipSuccess) plan(S);
  return e;
}

// appends the segment table to the arena, moves arena (upload: data + table, download: table only) and runs the copy kernel;
// upload_bytes (may be null): what an upload's one host-to-device copy moved
static hipError_t stage_run(Stage& S, hipStream_t stream, bool upload, size_t* upload_bytes = nullptr) {
  if (S.overflow) return hipErrorOutOfMemory;
  if (S.segs.empty()) return hipSuccess;
  const size_t data_end = S.used;
  Span<CopySeg> tab = S.take<CopySeg>(S.segs.size());
  if (S.overflow) return hipErrorOutOfMemory;
  std::memcpy(tab.p, S.segs.data(), S.segs.size() * sizeof(CopySeg));
  const size_t tab_off = reinterpret_cast<char*>(tab.p) - S.h;
  hipError_t e;
  if (upload && upload_bytes) *upload_bytes = S.used;
  if (upload) e = hipMemcpyAsync(S.d, S.h, S.used, hipMemcpyHostToDevice, stream);
  else e = hipMemcpyAsync(S.d + tab_off, S.h + tab_off, S.segs.size() * sizeof(CopySeg), hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) return e;
  const unsigned blocks = std::min<unsigned>((S.units + 255) / 256, 2048u);
  hipLaunchKernelGGL(k_copy_segments, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const CopySeg*>(S.d + tab_off),
                     (int)S.segs.size(), S.units);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (!upload) e = hipMemcpyAsync(S.h, S.d, data_end, hipMemcpyDeviceToHost, stream);
  return e;
}
