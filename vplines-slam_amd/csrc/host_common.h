// Host plumbing shared by the two contexts (vpl_ctx: ba_ctx.h, used by vplines_ba.hip and its host headers ba_upload.h and
// ba_session.h; the front-end's: vplines_frontend.hip): the error path of an entry point and the guarded device arrays.  A context type Ctx provides `std::string err`, `int device`, `bool guards` and the allocation
// record `std::vector<void*> allocs` / `std::vector<size_t> alloc_bytes`.
#pragma once
#include <hip/hip_runtime.h>

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

// One hipMalloc per array, zeroed, followed by 64 pad bytes (VPL_DEBUG_GUARDS=1 when the context is made: filled with 0xA5,
// checked by debug_guards).  allocs[i] is recorded as soon as it exists, so that free_arrays releases it on any later failure.
template <typename Ctx, typename T>
static hipError_t dalloc(Ctx* c, T** p, size_t n) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, n * sizeof(T) + 64);
  if (e != hipSuccess) return e;
  c->allocs.push_back(q);
  c->alloc_bytes.push_back(n * sizeof(T));
  *p = (T*)q;
  e = hipMemset(q, 0, n * sizeof(T) + 64);
  if (e == hipSuccess && c->guards) e = hipMemset((char*)q + n * sizeof(T), 0xA5, 64);
  return e;
}

template <typename Ctx>
static void free_arrays(Ctx* c) {
  for (void* p : c->allocs) (void)hipFree(p);   // (teardown: nothing to report to)
  c->allocs.clear();
  c->alloc_bytes.clear();
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
    HIPCHK(c, hipMemcpy(pad, (char*)c->allocs[i] + c->alloc_bytes[i], 64, hipMemcpyDeviceToHost));
    bool hit = false;
    for (int k = 0; k < 64; ++k) hit |= pad[k] != 0xA5;
    if (hit && !bad++) c->err = "guard behind device array #" + std::to_string(i) + " (" + std::to_string(c->alloc_bytes[i]) + " bytes) overwritten";
  }
  return bad;
}

}  // namespace vpl
