// dynamics_fused.h — the forward-only pass of the dynamics ensemble at precision 1 (dynamics_fused.hip): one launch packs every layer's
// weights into fp16 hi / lo planes, one launch takes a row tile of one (run, member) through ALL layers
//   OUT = W_L swish(... swish(W_0 x + b_0) ...) + b_L
// on v_mfma_f32_16x16x32_f16 with split operands, the hidden activations never leaving LDS.  dynamics.hip runs step(), sample_next() and
// the step / sample enqueues of the device loops through it; training, validation and the adversarial update stay on the fp32 GEMM.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orl_engine.h"
#include "gemm.h"

// widest layer (input, hidden or output) the fused kernel takes: 4 waves x 8 fragments x 16 columns of accumulators, and two fp16
// planes of a 16-row tile at that width in 33 KB of LDS (include/orl_engine.h documents the same number)
#define ORL_DYN_FUSED_MAX_WIDTH 512

namespace orl {

enum { DYF_FLAG_ACT = 0, DYF_FLAG_W = 1, DYF_FLAGS = 2 };     // sticky range words: an activation / a weight left the fp16 planes' range
enum { DYF_MAX_LAYERS = ORL_MAX_HIDDEN + 1 };

struct DyfP {
  int R, K, nl;                        // runs, members, layers (hidden + output)
  int width[DYF_MAX_LAYERS + 1];       // width[l]: inputs of layer l; width[nl]: the outputs
  int Kp[DYF_MAX_LAYERS];              // width[l] rounded up to 32: the pitch of a plane row of layer l
  long poff[DYF_MAX_LAYERS];           // layer l's [out][Kp] block inside one member's planes, in halves
  long pmember;                        // halves of one member's planes (a multiple of 8)
  int Wp;                              // widest Kp: an LDS plane row holds Wp + 8 halves
  const float* params; long P;         // the parameter block, run stride P
  long w_off[DYF_MAX_LAYERS], b_off[DYF_MAX_LAYERS];      // EnsembleLinear weight [K][in][out] and bias [K][1][out] of layer l
  hx_t* Bh; hx_t* Bl;                  // planes of w * ORL_WSCALE, [R][K][layer][out][Kp], the K tail zero
  const float* X; long n; int xp;      // layer 0's input [R][n][xp], shared by the members
  float* OUT; int op;                  // [R][K][n][op]
  unsigned int* flags;                 // [DYF_FLAGS]
};

// the fragments [f0, f0 + cnt) of an N-column layer that wave `wave` of 4 multiplies (cnt may be 0)
__device__ __forceinline__ void dyf_wave_frags(int N, int wave, int& f0, int& cnt) {
  const int nfrag = (N + 15) >> 4, per = (nfrag + 3) >> 2;
  f0 = wave * per;
  cnt = max(0, min(per, nfrag - f0));
}

// The pack of one thread: 4 k of a plane row of (run r, member k), element e of pmember / 4.  KCONT = false: the weight of layer l is
// (in, out)-major (EnsembleLinear) and adjacent threads take adjacent output columns; KCONT = true: it is nn.Linear's [out][ld] with
// ld = ld0 for layer 0 (which packs only its first width[0] columns) and width[l] above, and adjacent threads take adjacent k.
template <bool KCONT>
__device__ __forceinline__ void dyf_pack_one(const DyfP& p, long e, int k, int r, int ld0) {
  if (e >= (p.pmember >> 2)) return;
  int l = 0;
  while (l + 1 < p.nl && e >= (p.poff[l + 1] >> 2)) ++l;
  const long le = e - (p.poff[l] >> 2);
  const int in = p.width[l], N = p.width[l + 1], q = p.Kp[l] >> 2;
  const int o = KCONT ? (int)(le / q) : (int)(le % N), kk = (KCONT ? (int)(le - (long)o * q) : (int)(le / N)) * 4;
  const int ld = l ? in : ld0;
  const float* const W = p.params + (long)r * p.P + p.w_off[l] + (KCONT ? (long)o * ld : (long)k * in * N + o);
  const long sk = KCONT ? 1 : N;
  f32x4 v;
  unsigned int bad = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = kk + j < in ? W[(long)(kk + j) * sk] * ORL_WSCALE : 0.f;
    bad |= !(fabsf(v[j]) < 65504.f);
  }
  hx4 h, lo;
  orl_split4(v, h, lo);
  const long at = ((long)r * p.K + k) * p.pmember + p.poff[l] + (long)o * p.Kp[l] + kk;
  *(hx4*)(p.Bh + at) = h;
  *(hx4*)(p.Bl + at) = lo;
  if (bad) p.flags[DYF_FLAG_W] = 1u;
}

// fills Kp, poff, pmember and Wp from nl and width; returns the halves of one plane of the whole object (R K pmember)
long dyf_layout(DyfP& p);
// rows per workgroup the launcher picks for n rows: the largest of 64 / 32 / 16 whose planes fit the LDS and that still gives 256
// workgroups, else 16
int dyf_pick_tile(const DyfP& p);
// every layer's weights -> the planes; raises flags[DYF_FLAG_W] when |w| ORL_WSCALE >= 65504 or w is not finite
hipError_t dyf_pack(const DyfP& p, hipStream_t st);
// the fused forward of p.n rows; raises flags[DYF_FLAG_ACT] when a split activation is not finite or reaches 32768
hipError_t dyf_forward(const DyfP& p, hipStream_t st);

}  // namespace orl
