// Instantiations of the activation-stationary 1x1 kernel (conv_x1_impl.h): data gradients with the
// BN-backward fold prologue (JOINBWD with the ReLU bit mask / ADD / STORE epilogues).
#include "conv_x1_impl.h"

namespace fdt {
namespace conv {

bool x1_launch_fold(int pro, int epi, int act, const ConvArgs& a, int BM, int BN, int xn, size_t lds, hipStream_t st) {
#define FDT_X1_CASE(P_, E_, A_) \
  if (pro == P_ && epi == E_ && act == A_) return x1_launch_tile<P_, E_, A_>(a, BM, BN, xn, lds, st);
  FDT_X1_CASE(kProFold, kEpiJoinBwd, kActRelu)
  FDT_X1_CASE(kProFold, kEpiAdd, kActNone)
  FDT_X1_CASE(kProFold, kEpiStore, kActNone)
#undef FDT_X1_CASE
  return false;
}

}  // namespace conv
}  // namespace fdt
