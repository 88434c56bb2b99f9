// What the LDS layouts (ba_marg_layout.h, ba_step_layout.h) are written with.  A layout is one text for two readers: P = int on
// the host (offsets in doubles from the start of the dynamic LDS: the size of the dispatch and the CPU checks read them) and
// P = double* on the device (the pointers a kernel body uses).  On the device the carve is then a chain of pointer increments, as
// it was when the bodies wrote it by hand, and the constant parts of an offset end up in the immediate field of the LDS
// instruction; taken as base + integer offset k_marg<512> ran 1.6 % slower at n = 75.  Plain C++: includes without HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VPL_LAYOUT_HD __host__ __device__
#else
#define VPL_LAYOUT_HD
#endif

namespace vpl {

// `len` doubles from `at` on.  An array of ints is a span too: 2 len ints, or n of them where a layout says so (LdsIntsT).
template <class P> struct LdsSpanT { P at; int len; };
// n ints from `at` on (`at` counts in doubles, as everywhere): ends in the middle of a double when n is odd
template <class P> struct LdsIntsT { P at; int n; };

// the next region: `len` doubles (n ints, rounded up to a double) from o on; o moves behind it
template <class P> VPL_LAYOUT_HD inline void lds_put(LdsSpanT<P>& s, P& o, int len) { s.at = o; s.len = len; o = o + len; }
// (the device steps over the ints themselves, as the bodies did by hand: o + (n + 1) / 2 is a signed division more)
VPL_LAYOUT_HD inline int lds_behind_ints(int o, int n) { return o + (n + 1) / 2; }
VPL_LAYOUT_HD inline double* lds_behind_ints(double* o, int n) { return (double*)((int*)o + n); }
template <class P> VPL_LAYOUT_HD inline void lds_put(LdsIntsT<P>& s, P& o, int n) { s.at = o; s.n = n; o = lds_behind_ints(o, n); }

// o rounded up to 16 bytes.  The host counts from a 16-byte aligned start; the device rounds the address it has.
VPL_LAYOUT_HD inline int lds_align16(int o) { return (o + 1) & ~1; }
VPL_LAYOUT_HD inline double* lds_align16(double* o) { return (double*)(((uintptr_t)o + 15) & ~(uintptr_t)15); }

}  // namespace vpl
