// rnn_fused.h — the GRU stack of RNNDynamics' window forward at eval precision 1 (rnn_fused.hip): one launch packs [W_ih | W_hh] of every
// layer into fp16 hi / lo planes, one launch takes a row tile of sequences through ALL layers and ALL time steps on
// v_mfma_f32_16x16x32_f16 with split operands, the hidden states never leaving LDS.  rnn_dynamics.hip runs orl_rnn_forward,
// orl_rnn_forward_runs and orl_rnn_state_prime through it after orl_rnn_set_eval_precision(1); training and orl_rnn_state_step stay on the
// fp32 MFMA.
#pragma once
#include "dynamics_fused.h"          // the split helpers (orl_split4, ORL_WSCALE, ORL_MFMA_16x16x32, hx8), one copy

namespace orl {

__device__ __forceinline__ float rnn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

enum { RNF_FLAG_ACT = 0, RNF_FLAG_W = 1, RNF_FLAGS = 2 };     // sticky range words: an input / a weight left the fp16 planes' range
enum { RNF_MAX_LAYERS = 4, RNF_MAX_H = 512, RNF_WAVES = 8 };
enum { RNF_LDS_BYTES = 160 * 1024 };                          // of a gfx950 CU

struct RnfP {
  int L, H, in;                        // GRU layers, hidden units (a multiple of 4), layer 0's input width
  int rows, T;                         // sequences and their time steps
  int Hp, Kxp[RNF_MAX_LAYERS];         // H and layer l's input width rounded up to 32: a plane row of layer l holds Kxp[l] + Hp halves
  int G16;                             // 3H rounded up to 16: the rows of a layer's planes
  long poff[RNF_MAX_LAYERS];           // layer l's [G16][Kxp[l] + Hp] block inside one run's planes, in halves
  long prun;                           // halves of one run's planes (a multiple of 8)
  const float* params; long P;         // the parameter block of the launch's first run, run stride P
  long wih[RNF_MAX_LAYERS], whh[RNF_MAX_LAYERS], bih[RNF_MAX_LAYERS], bhh[RNF_MAX_LAYERS];   // [3H][in or H], [3H][H], [3H], [3H]
  hx_t* Bh; hx_t* Bl;                  // planes of w * ORL_WSCALE, [runs][layer][G16][Kxp + Hp], the k tails and the rows past 3H zero
  const float* X0; int xp; long x_rs;  // [rows * T][xp] per run (x_rs = 0: shared), row b * T + t
  float* HO; int hop; long ho_rs;      // [rows * T][hop]: the top layer's h_t
  float* st[2]; long st_rs, n_traj;    // priming: [runs][L][n_traj][H] in both state buffers, slot b <- h_{T-1} of sequence b; or null
  unsigned int* flags;                 // [RNF_FLAGS]
  int cus;                             // compute units of the device: the tile choice wants a workgroup for each
};

// fills Hp, Kxp, G16, poff and prun from L, H and in; returns prun
long rnf_layout(RnfP& p);
// LDS bytes of a workgroup of rt sequences: h planes [L][2][rt][Hp + 8] and layer 0's input planes [2][rt][Kxp[0] + 8]
size_t rnf_lds_bytes(const RnfP& p, int rt);
// sequences per workgroup for p.rows rows of `runs` runs: the largest of 64 / 32 / 16 whose planes fit RNF_LDS_BYTES and that still gives
// p.cus workgroups, else the smallest that fits; 0: none fits
int rnf_pick_tile(const RnfP& p, int runs);
// every layer's [W_ih | W_hh] of `runs` runs -> the planes; raises flags[RNF_FLAG_W] when |w| ORL_WSCALE >= 65504 or w is not finite
hipError_t rnf_pack(const RnfP& p, int runs, hipStream_t st);
// the fused GRU stack; raises flags[RNF_FLAG_ACT] when an input is not finite or reaches 32768
hipError_t rnf_forward(const RnfP& p, int runs, hipStream_t st);

}  // namespace orl
