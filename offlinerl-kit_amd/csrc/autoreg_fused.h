// autoreg_fused.h — the autoregressive behaviour policy's sampling at sample precision 1 (autoreg_fused.hip): one launch packs every
// layer's weights into fp16 hi / lo planes, one launch takes a row tile of one run through ALL act_dim passes and ALL layers of every pass
//   a_j = mean_j + e^logstd_j eps_j,  (mean_j, logstd_j) = leaky(W_L leaky(... leaky(W_0 [obs | a_<j, 0 | onehot_j] + b_0) ...) + b_L)
// on v_mfma_f32_16x16x32_f16 with split operands; no hidden activation, input row or tail value leaves the workgroup.  The engine runs
// orl_autoreg_sample and the sampling leg of orl_mbrcsl_rollout through it after orl_autoreg_set_sample_precision(1); training stays on
// the tiled GEMM.  The planes, their layout, the fragment dealing and the pack are the dynamics ensemble's (dynamics_fused.h), one copy.
#pragma once
#include "dynamics_fused.h"

// widest layer (obs_dim or hidden) the fused sampling kernel takes (include/orl_engine.h documents the same number)
#define ORL_AUTOREG_FUSED_MAX_WIDTH ORL_DYN_FUSED_MAX_WIDTH

namespace orl {

struct ArfP {
  // the net as the planes see it: K = 1 member, nl = L + 1 layers, width[0] = obs_dim (layer 0 packs only its observation columns),
  // width[1 .. L] the hidden widths, width[nl] = 2; n rows per run; flags [DYF_FLAGS].  X / OUT are not used.
  DyfP g;
  int A, in0;                          // act_dim; obs_dim + 2 A: the pitch of a row of layer 0's weight [H0][in0]
  const float* obs;                    // [R][n][obs_dim]
  const float* eps; long e_rs;         // [R][n][A] standard normals, run stride e_rs
  float* act;                          // [R][n][A]
};

// fills the plane layout (dyf_layout) of p.g; returns the halves of one plane of the whole object
long arf_layout(ArfP& p);
// rows per workgroup: dyf_pick_tile's rule on (row tiles x runs)
int arf_pick_tile(const ArfP& p);
// every layer's weights of every run -> the planes; raises flags[DYF_FLAG_W] when |w| ORL_WSCALE >= 65504 or w is not finite
hipError_t arf_pack(const ArfP& p, hipStream_t st);
// the fused sampling of p.g.n rows per run; raises flags[DYF_FLAG_ACT] when a split value (obs, hidden activation) is not finite or
// reaches 32768
hipError_t arf_sample(const ArfP& p, hipStream_t st);

}  // namespace orl
