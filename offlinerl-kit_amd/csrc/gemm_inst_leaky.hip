// gemm_inst_leaky.hip — the LeakyReLU(0.01) flavours of the tiled GEMM (csrc/gemm_kernel.h) used by the autoregressive policy
// (csrc/algo_autoreg.inc): forward bias + LeakyReLU and the dgrad scaled by LeakyReLU' read from the stored activation.
#include "gemm_kernel.h"

namespace orl {
template hipError_t launch_gemm<PA_PLAIN, PB_PLAIN, E_BIAS_LEAKY>(int, const GemmP&, int, hipStream_t, bool, bool, int);
template hipError_t launch_gemm<PA_PLAIN, PB_PLAIN, E_LEAKY_MASK>(int, const GemmP&, int, hipStream_t, bool, bool, int);
}  // namespace orl
