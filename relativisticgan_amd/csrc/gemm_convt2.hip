// The MODE_CONVT2 instantiations of the implicit-GEMM kernel (gemm_body.h).
#include "gemm_body.h"

namespace rgan {

void launch_gemm_convt2(const GemmLaunch& l) { launch_mode<MODE_CONVT2>(l); }

}  // namespace rgan
