// Host side of the activation-stationary 1x1 convolution (kg 10; kernel: conv_x1_impl.h) and its
// forward instantiations (EPI_STATS; the fold-prologue data gradients: conv_x1_inst_fold.hip).
#include "conv_x1_impl.h"

namespace fdt {
namespace conv {

bool x1_launch_stats(int pro, int epi, int act, const ConvArgs& a, int BM, int BN, int xn, size_t lds, hipStream_t st) {
#define FDT_X1_CASE(P_, E_, A_) \
  if (pro == P_ && epi == E_ && act == A_) return x1_launch_tile<P_, E_, A_>(a, BM, BN, xn, lds, st);
  FDT_X1_CASE(kProNone, kEpiStats, kActNone)
  FDT_X1_CASE(kProAffineAct, kEpiStats, kActRelu)
  FDT_X1_CASE(kProAffineAct, kEpiStats, kActNone)
#undef FDT_X1_CASE
  return false;
}

static bool x1_combo(int pro, int epi, int act) {
  return (pro == kProNone && epi == kEpiStats && act == kActNone) ||
         (pro == kProAffineAct && epi == kEpiStats && (act == kActRelu || act == kActNone)) ||
         (pro == kProFold && epi == kEpiJoinBwd && act == kActRelu) ||
         (pro == kProFold && (epi == kEpiAdd || epi == kEpiStore) && act == kActNone);
}

static size_t x1_lds_bytes(int pro, int epi, int Cx, int BN) {
  const int nprm = pro == kProFold ? 3 : (pro == kProAffineAct ? 2 : 0);
  return x1_hdr_bytes(nprm, epi == kEpiJoinBwd ? 3 : 2, Cx, BN) + x1_ring_bytes(BN) + x1_stage_bytes(BN);
}

bool x1_supported(int pro, int epi, int act, const ConvArgs& a, int BM, int BN, int xn, bool pure) {
  if (!pure || !x1_combo(pro, epi, act) || BN != 128 || a.K != a.Cx || a.Cout % BN) return false;
  // the resident fragments fill 128 VGPRs at BM * K = 128 * 256 = 64 * 512
  if (!((BM == 128 && (a.K == 64 || a.K == 128 || a.K == 256)) || (BM == 64 && a.K == 512))) return false;
  if (epi == kEpiJoinBwd && (a.jmask == nullptr || a.es != nullptr)) return false;  // ReLU bit-mask joins
  return xn >= 1 && a.nbn % xn == 0;
}

bool launch_x1(int pro, int epi, int act, const ConvArgs& a, int BM, int BN, int xn, bool pure, hipStream_t st) {
  if (!x1_supported(pro, epi, act, a, BM, BN, xn, pure)) return false;
  const size_t lds = x1_lds_bytes(pro, epi, a.Cx, BN);
  return x1_launch_stats(pro, epi, act, a, BM, BN, xn, lds, st) || x1_launch_fold(pro, epi, act, a, BM, BN, xn, lds, st);
}

}  // namespace conv
}  // namespace fdt
