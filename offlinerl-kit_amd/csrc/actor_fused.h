// actor_fused.h — the tanh-Gaussian actor's rollout sampling on split fp16 (actor_fused.hip): one launch packs every actor Linear into
// fp16 hi / lo planes, one launch takes a row tile of one run through the backbone, the stacked [mu ; sigma] head and the draw
//   h_{l+1} = relu(W_l h_l + b_l),  mu = W_mu h_L + b_mu,  ls = clamp(W_sigma h_L + b_sigma, -5, 2),  act = tanh(mu + e^ls eps)
// on v_mfma_f32_16x16x32_f16 with split operands; no hidden activation and no head value leaves the workgroup.  orl_actor_sample
// (actor_sample.inc) runs through it; training and every other forward of the actor stay where they were.  The planes, their layout, the
// fragment dealing and the pack are the dynamics ensemble's (dynamics_fused.h), one copy.
#pragma once
#include "dynamics_fused.h"

// widest layer (obs_dim or hidden) and the most action dimensions the fused actor kernel takes (include/orl_engine.h documents both):
// the head layer is 2 act_dim <= 64 columns, its fp32 staging block at 64 rows 16 KB next to the planes
#define ORL_ACTOR_FUSED_MAX_WIDTH ORL_DYN_FUSED_MAX_WIDTH
#define ORL_ACTOR_FUSED_MAX_ACT 32

namespace orl {

struct AcfP {
  // the net as the planes see it: K = 1 member, nl = L + 1 layers, width[0] = obs_dim, width[1 .. L] the hidden widths, width[nl] = 2 A
  // (the arena stores [mu ; sigma] as one [2A][H_L] matrix with one [2A] bias); R = the runs of THIS launch, params / Bh / Bl point at
  // the first of them; n rows per run; flags [DYF_FLAGS].  X / OUT are not used.
  DyfP g;
  int A, deterministic;
  const float* obs;                    // [R][n][obs_dim]
  const float* eps; long e_rs;         // [R][n][A] standard normals, run stride e_rs (not read when deterministic)
  const int* live;                     // [R] device: the rows of run r that count (null: n for every run); the rest are written as zeros
  float* act;                          // [R][n][A]
};

// fills the plane layout (dyf_layout) of p.g; returns the halves of one plane of the whole object
long acf_layout(AcfP& p);
// rows per workgroup: dyf_pick_tile's rule on (row tiles x runs), the staging block counted into the LDS
int acf_pick_tile(const AcfP& p);
// every layer's weights of the launch's runs -> the planes; raises flags[DYF_FLAG_W] when |w| ORL_WSCALE >= 65504 or w is not finite
hipError_t acf_pack(const AcfP& p, hipStream_t st);
// the fused sampling of p.g.n rows per run; raises flags[DYF_FLAG_ACT] when a split value (obs, hidden activation) is not finite or
// reaches 32768
hipError_t acf_sample(const AcfP& p, hipStream_t st);

}  // namespace orl
