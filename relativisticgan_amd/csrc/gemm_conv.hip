// The MODE_CONV instantiations of the implicit-GEMM kernel (gemm_body.h).
#include "gemm_body.h"

namespace rgan {

void launch_gemm_conv(const GemmLaunch& l) { launch_mode<MODE_CONV>(l); }

}  // namespace rgan
