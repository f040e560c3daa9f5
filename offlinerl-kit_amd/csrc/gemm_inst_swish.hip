// gemm_inst_swish.hip — the Swish flavours of the tiled GEMM (csrc/gemm_kernel.h) used by the dynamics ensemble (csrc/dynamics.hip):
// forward bias + Swish (z kept for the backward) and the dgrad scaled by Swish'(z).
#include "gemm_kernel.h"

namespace orl {
template hipError_t launch_gemm<PA_PLAIN, PB_PLAIN, E_BIAS_SWISH>(int, const GemmP&, int, hipStream_t, bool, bool, int);
template hipError_t launch_gemm<PA_PLAIN, PB_PLAIN, E_SWISH_GRAD>(int, const GemmP&, int, hipStream_t, bool, bool, int);
}  // namespace orl
