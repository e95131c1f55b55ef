// The MODE_WGRAD instantiations of the implicit-GEMM kernel (gemm_body.h).
#include "gemm_body.h"

namespace rgan {

void launch_gemm_wgrad(const GemmLaunch& l) { launch_mode<MODE_WGRAD>(l); }

}  // namespace rgan
