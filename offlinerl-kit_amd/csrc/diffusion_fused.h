// diffusion_fused.h — the split-fp16 sampling path of DiffusionBC (diffusion_fused.hip): one launch computes
//   tail(Mish(GroupNorm(X W^T + b)))   on column slabs made of whole groups   and/or   [Mish](X W^T + b)   on plain column slabs
// from fp32 activations (split into fp16 hi / lo planes while they are staged into LDS) and weights pre-split into planes once per
// EMA generation.  orl_diffusion_sample runs every Linear of a pass through it at sample precision 1 (diffusion.hip: diff_forward_split).
#pragma once
#include <hip/hip_runtime.h>

#include "gemm.h"
#include "reduce.h"

// widest GroupNorm group (channels) the fused kernel holds in one workgroup slab (include/orl_engine.h documents the same number)
#define ORL_DIFF_FUSED_MAX_GROUP 128

namespace orl {

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// nn.Mish: x tanh(softplus(x))
__device__ __forceinline__ float diff_mish(float x) { return x * tanhf(softplus(x)); }
#endif

enum { DFU_FLAG_ACT = 0, DFU_FLAG_W = 1, DFU_FLAGS = 2 };     // sticky range words: an activation / a weight left the fp16 planes' range

// a matrix read as one or two column ranges: columns [0, k0) of p0 (pitch s0), the rest of p1 (pitch s1); p1 null: everything of p0
struct DfuCols { const float* p0; int s0, k0; const float* p1; int s1; };

struct DfuP {
  int rows, K, Kp, N;              // Y [rows][N] = X [rows][K] W^T; Kp = K rounded up to 32: the pitch of a plane's row
  DfuCols A; int a_mish;           // X (a_mish: Mish applied to an element as it is staged)
  const hx_t* Bh; const hx_t* Bl;  // planes of W * ORL_WSCALE, [N][Kp], the K tail zero
  const float* bias;               // [N]
  // columns [0, Cn): GroupNorm over groups of cg channels (eps 1e-5), affine, Mish, then the FiLM tail (scale film[row][c], shift
  // film[row][Cn + c]) or the residual tail (+ res[row][c]); `gps` whole groups per workgroup slab
  int Cn, cg, gps, norm_slabs;
  const float* gamma; const float* beta;
  const float* film; int fp;
  DfuCols res;
  float* out; int op;
  // columns [Cn, N): bias only (plain_mish: Mish of it), column Cn + j to out2[row][j]
  int plain_mish;
  float* out2; int o2p;
  unsigned int* flags;             // [DFU_FLAGS]
};

// rows of 16 MA per workgroup, 64 NFW slab columns; the choice the launcher made for (rows, N, Cn, cg)
struct DfuTile { int ma, nfw; };
DfuTile dfu_pick_tile(int rows, int N, int Cn, int cg);
// fills Kp-independent geometry (gps, norm_slabs) from the tile and launches; p.Cn == 0: no norm part
hipError_t dfu_launch(DfuP p, hipStream_t st);
// W [N][K] fp32 -> the two planes [N][Kp]; raises flags[DFU_FLAG_W] when |w| ORL_WSCALE >= 65504 or w is not finite
hipError_t dfu_split_weights(const float* W, int N, int K, int Kp, hx_t* Bh, hx_t* Bl, unsigned int* flags, hipStream_t st);
// flags[which] = 0
hipError_t dfu_clear_flag(unsigned int* flags, int which, hipStream_t st);

}  // namespace orl
