// lin_prh_n (csrc/ba_lin.h) on the host: the largest prior whose J0^T J0 k_lin keeps in LDS in a context of the given point and
// line capacity.  Arguments: pairs "max_points max_lines" as vpl_ctx_create takes them.  One line per pair:
// "<points as rounded by the context> <lines> <lin_prh_n> <1 when k_lin's fixed LDS part fits the budget>".
#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime.h>

#include "ba_lin.h"

int main(int argc, char** argv) {
  for (int i = 1; i + 1 < argc; i += 2) {
    const int P = (std::atoi(argv[i]) + 1) & ~1, L = std::atoi(argv[i + 1]);
    std::printf("%d %d %d %d\n", P, L, vpl::lin_prh_n(P, L), (int)(vpl::lin_smem_base(P, L) <= vpl::LIN_LDS_BUDGET));
  }
  return 0;
}
