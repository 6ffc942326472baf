// Instantiations of the implicit-GEMM conv kernel: frozen-inference forward convolutions
// (EPI_NORMACT: normalisation with frozen statistics + activation + residual join in the epilogue).
#include "conv_igemm_impl.h"

namespace fdt {
namespace conv {

bool launch_cases_infer(int pro, int epi, int act, const ConvArgs& a, int BM, int BN, int BK, int kg, bool pure,
                        hipStream_t st) {
#define FDT_CONV_CASE(P_, E_, A_) \
  if (pro == P_ && epi == E_ && act == A_) { launch_tile<P_, E_, A_>(a, BM, BN, BK, kg, pure, st); return true; }
  FDT_CONV_CASE(kProNone, kEpiNormAct, kActNone)
  FDT_CONV_CASE(kProNone, kEpiNormAct, kActRelu)
  FDT_CONV_CASE(kProNone, kEpiNormAct, kActCelu)
#undef FDT_CONV_CASE
  return false;
}

}  // namespace conv
}  // namespace fdt
