// Host plumbing shared by the two contexts (vpl_ctx: ba_ctx.h, used by vplines_ba.hip and its host headers ba_upload.h and
// ba_session.h; the front-end's: vplines_frontend.hip): the error path of an entry point and the guarded device arrays.  A context type Ctx provides `std::string err`, `int device`, `bool guards` and the allocation
// record `std::vector<vpl::DevAlloc> allocs`.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

namespace vpl {

template <typename Ctx>
static int fail(Ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

}  // namespace vpl

#define HIPCHK(ctx, call)                                                                         \
  do {                                                                                            \
    hipError_t e__ = (call);                                                                      \
    if (e__ != hipSuccess) return vpl::fail(ctx, VPL_E_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
  } while (0)

namespace vpl {

// One device array of a context: 64 pad bytes follow its payload (VPL_DEBUG_GUARDS=1: filled with 0xA5, debug_guards).  The
// owner is null for the context's own arrays and the session (vpl_odo, vpl_trk) for those a session took while it borrows the
// context: dfree_owner gives exactly those back, wherever they lie in the record.
struct DevAlloc {
  void* p;
  size_t bytes;
  const void* owner;
};

// One hipMalloc per array, zeroed, followed by 64 pad bytes.  The array is recorded as soon as it exists, so that free_arrays
// (or dfree_owner) releases it on any later failure.
template <typename Ctx, typename T>
static hipError_t dalloc(Ctx* c, T** p, size_t n, const void* owner = nullptr) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, n * sizeof(T) + 64);
  if (e != hipSuccess) return e;
  c->allocs.push_back(DevAlloc{q, n * sizeof(T), owner});
  *p = (T*)q;
  e = hipMemset(q, 0, n * sizeof(T) + 64);
  if (e == hipSuccess && c->guards) e = hipMemset((char*)q + n * sizeof(T), 0xA5, 64);
  return e;
}

// frees and forgets the arrays for which pred(record) holds; the others keep their order (teardown: nothing to report to)
template <typename Ctx, typename Pred>
static void dfree_if(Ctx* c, Pred pred) {
  for (const DevAlloc& a : c->allocs)
    if (pred(a)) (void)hipFree(a.p);
  c->allocs.erase(std::remove_if(c->allocs.begin(), c->allocs.end(), pred), c->allocs.end());
}
template <typename Ctx>
static void dfree_owner(Ctx* c, const void* owner) { dfree_if(c, [owner](const DevAlloc& a) { return a.owner == owner; }); }
template <typename Ctx>
static void dfree(Ctx* c, const void* ptr) { if (ptr) dfree_if(c, [ptr](const DevAlloc& a) { return a.p == ptr; }); }
template <typename Ctx>
static void free_arrays(Ctx* c) { dfree_if(c, [](const DevAlloc&) { return true; }); }

// Test access (vpl_ba_debug_allocs, vpl_fe_debug_allocs): the number of arrays in the record and their payload bytes
template <typename Ctx>
static int debug_allocs(Ctx* c, long long* n_arrays, long long* payload_bytes) {
  if (!c || !n_arrays || !payload_bytes) return VPL_E_INVALID;
  *n_arrays = (long long)c->allocs.size();
  *payload_bytes = 0;
  for (const DevAlloc& a : c->allocs) *payload_bytes += (long long)a.bytes;
  return VPL_OK;
}

// Debug aid of the randomised sweeps: how many arrays have had their pad written to (a kernel ran past the end of an array),
// the first one named in the context's last error by its allocation index and size.
template <typename Ctx>
static int debug_guards(Ctx* c) {
  if (!c) return VPL_E_INVALID;
  if (!c->guards) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  int bad = 0;
  unsigned char pad[64];
  for (size_t i = 0; i < c->allocs.size(); ++i) {
    const DevAlloc& a = c->allocs[i];
    HIPCHK(c, hipMemcpy(pad, (char*)a.p + a.bytes, 64, hipMemcpyDeviceToHost));
    bool hit = false;
    for (int k = 0; k < 64; ++k) hit |= pad[k] != 0xA5;
    if (hit && !bad++) c->err = "guard behind device array #" + std::to_string(i) + " (" + std::to_string(a.bytes) + " bytes) overwritten";
  }
  return bad;
}

}  // namespace vpl
