// store.h — the HBM-resident row stores of the C ABI: the replay buffer (orl_buffer: a loaded dataset or a growable model-rollout ring)
// and the trajectory store of the RCSL rollout (orl_traj), both in store.hip.  Neither needs an Engine; this header is what the engine
// (engine.h) and DiffusionBC (diffusion.hip) see of them: the column set both hold, the sampling kernel the engine launches itself, the
// termination test its kernels share with the rollout append, and the few host calls the attach functions go through.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>

#include "devobj.h"
#include "rng.h"

namespace orl {

// ------------------------------------------------------------------------------------------------
// the termination test of utils/termination_fns.py on next_obs (policy/model_based/mopo.py:45-79): the numpy comparisons of the
// reference restated, every test below is false on NaN, like numpy's
// ------------------------------------------------------------------------------------------------
enum { ORL_TERM_NONE = 0, ORL_TERM_HALFCHEETAH, ORL_TERM_HOPPER, ORL_TERM_WALKER2D, ORL_TERM_ANT, ORL_TERM_HUMANOID, ORL_TERM_PEN, ORL_TERM_KINDS };
__device__ inline bool orl_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ inline bool orl_term_done(int kind, const float* x, int od) {
  switch (kind) {
    case ORL_TERM_HALFCHEETAH: {
      bool in = true;
      for (int c = 0; c < od; ++c) in = in && (x[c] > -100.f) && (x[c] < 100.f);
      return !in;
    }
    case ORL_TERM_HOPPER: {             // abs(next_obs[:, 1:] < 100): an upper bound only, on columns 1..
      bool ok = true;
      for (int c = 0; c < od; ++c) ok = ok && orl_finite(x[c]) && (c == 0 || x[c] < 100.f);
      return !(ok && x[0] > .7f && fabsf(x[1]) < .2f);
    }
    case ORL_TERM_WALKER2D: {
      bool in = true;
      for (int c = 0; c < od; ++c) in = in && (x[c] > -100.f) && (x[c] < 100.f);
      return !(in && x[0] > 0.8f && x[0] < 2.0f && x[1] > -1.0f && x[1] < 1.0f);
    }
    case ORL_TERM_ANT: {
      bool fin = true;
      for (int c = 0; c < od; ++c) fin = fin && orl_finite(x[c]);
      return !(fin && x[0] >= 0.2f && x[0] <= 1.0f);
    }
    case ORL_TERM_HUMANOID: return (x[0] < 1.0f) || (x[0] > 2.0f);      // NaN: not done
    case ORL_TERM_PEN: return x[26] < 0.075f;                           // (od >= 27: term_refusal on the host)
    default: return false;
  }
}
// The one host-side refusal of a termination kind: 0, or -1 with "<who>: unknown termination kind" resp. "<who>: termination kind K reads
// observation column C, the <what> has N columns" as the error text (`od` = the N observation columns of `what`).
int term_refusal(const std::string& who, int term_kind, int od, const char* what);

// ------------------------------------------------------------------------------------------------
// the five columns of a row store: SoA in HBM, rows padded to 16 B (obs / next_obs pitch OP, act pitch AP, pad columns zero)
// ------------------------------------------------------------------------------------------------
// one model ring as the samplers see it: the arrays and the device cell that holds the current size.  With per-run model rings
// (orl_engine_attach_model_buffers) a table of these, one per run, sits in engine-owned device memory: the captured graph holds the
// table's address, the rings grow behind it.
struct ModelSrc { const float *obs, *nobs, *act, *rew, *term; const long long* n; };
// (r = blockIdx.y: block-uniform, the table entry comes by scalar loads; `one` is the single ring of the launch parameters, which
// k_prepare hands over field by field: a reference to the parameter block itself put its 2 KB job table into scratch memory)
__device__ inline ModelSrc orl_model_src(const ModelSrc* tab, int r, ModelSrc one) { return tab ? tab[r] : one; }

struct Rows {
  float *obs = nullptr, *nobs = nullptr, *act = nullptr, *rew = nullptr, *term = nullptr;
  int od = 0, ad = 0, OP = 0, AP = 0;
  void set_dims(int obs_dim, int act_dim) { od = obs_dim; ad = act_dim; OP = rup4(obs_dim); AP = rup4(act_dim); }
  // every host loop over the columns goes through this table, in the argument order of the C ABI: obs, act, next_obs, rew, term
  struct Col { float** p; int dim, pitch; };
  std::array<Col, 5> cols() { return {{{&obs, od, OP}, {&act, ad, AP}, {&nobs, od, OP}, {&rew, 1, 1}, {&term, 1, 1}}}; }
  int alloc_rows(long n);         // frees what is there, then n zero-filled rows
  void free_cols();
  // rows [row0, row0 + n) <- packed sources / -> packed host destinations (a null one is skipped), in the order of cols()
  int copy_in(long row0, const float* const src[5], long n, hipMemcpyKind kind);
  int copy_out(long row0, float* const dst[5], long n);
};

struct Buffer : Rows {      // HBM-resident replay buffer (buffer/buffer.py)
  int dev = 0;
  long n = 0;
  long long* idx = nullptr; long idx_cap = 0;
  unsigned long long counter = 0;
  // max |obs|, |next_obs|, |act| ([0]) and max |rew| ([1]: RCSL engines, the column holds the return-to-go, an MFMA operand) of
  // generation absmax_gen[.]: engines at precision 1 ask for them (buffer_absmax)
  float absmax[2] = {-1.f, -1.f}; unsigned long long absmax_gen[2] = {~0ull, ~0ull};
  unsigned long long gen = 0;   // bumped by every orl_buffer_load / orl_buffer_reserve: engines re-capture graphs that hold the old dataset pointers / size
  // growable ring (orl_buffer_reserve): `cap` rows allocated once, rows land at (ptr + i) % cap, n = min(n + i, cap) as in add_batch
  // (buffer.py:52-70).  d_n mirrors n in a device cell: kernels that sample the ring as the MODEL source read the size from it, so a
  // captured graph stays valid while the ring grows.
  long cap = 0, ptr = 0;
  long long* d_n = nullptr;
  // the rollout append keeps its scratch with the FIRST ring of the call: [runs] ring table, [runs] alive counts, [runs] reward sums
  // (the two read back in one copy), then [runs][blocks] reward sums and alive counts
  void* runs_scratch = nullptr; long runs_scratch_runs = 0, runs_scratch_blocks = 0;
  ModelSrc model_src() const { return ModelSrc{obs, nobs, act, rew, term, d_n}; }
  ~Buffer();
};

struct Traj : Rows {        // HBM-resident trajectory store of the RCSL rollout (policy/rcsl/rcsl.py:57-120): orl_traj
  int dev = 0;
  long n_traj_cap = 0, cap = 0;           // sizes given at creation: trajectories, rows
  long n_traj = 0, rows = 0, live = 0;    // of the current rollout: trajectories, rows appended, trajectories still running
  int half = 0;                           // which of the two live arrays holds the running trajectories
  bool finished = false;                  // rtg[] is valid for rows [0, rows)
  // counted steps (orl_traj_append_step_counted) count on the device: until a refresh `live` is an upper bound and `rows` is stale
  long rows_bound = 0;                    // upper bound on the rows written: rows + the bounds enqueued since the last refresh
  bool stale = false;
  int* tidx = nullptr; double *acc = nullptr, *rtg = nullptr;
  double* returns = nullptr;
  int* live_idx[2] = {nullptr, nullptr}; double* live_acc[2] = {nullptr, nullptr};
  int* blk_cnt = nullptr; double* blk_rew = nullptr;      // per-block scratch: max(blocks of a step, blocks of an export)
  long long* cells = nullptr; double* rew_total = nullptr; // the result and count cells (store.hip: CELL_*), the running reward sum
  ~Traj();
};

// ------------------------------------------------------------------------------------------------
// replay gather (buffer.py:96-106).  idx == nullptr -> Philox indices (np.random.randint(0, size, B) restated on device).
// One thread per (row, column) of the widest array; consecutive lanes read consecutive floats of a row
// (coalesced within the row) and rows are independent random 64-128 B segments.
// grid (ceil(B*W/256), R) with W = max(OP, AP).  (static: the engine's sampling launch and the store's each carry a copy)
// ------------------------------------------------------------------------------------------------
struct GatherP {
  Rows src; long n;                            // the dataset and its size
  int B, W;
  const long long* idx; long idx_rs;           // [R][B] or null
  float *b_obs, *b_nobs, *b_act, *b_rew, *b_term;  // destinations
  long obs_rs, nobs_rs, act_rs, rew_rs, term_rs;   // run strides of the destinations
  int d_op, d_ap;                                  // destination row pitches (>= od / ad; extra columns zeroed)
  unsigned long long seed;
  const unsigned long long* gstep;
  unsigned long long counter;                      // used when gstep == nullptr
  // second source (orl_engine_attach_model_buffer): batch rows [real_rows, B) come from the model ring, whose current size is read from
  // its device cell (the ring grows between replays of a captured graph); m.obs == nullptr: one source, the path above
  ModelSrc m;
  int real_rows;
  const ModelSrc* m_tab;                           // per-run model rings (orl_engine_attach_model_buffers), or null: the ring above for every run
};
static __global__ void k_gather(GatherP p) {
  const int r = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int row = t / p.W, c = t - row * p.W;
  if (row >= p.B) return;
  // the source of a batch row is a function of the row alone: real rows first, model rows behind them (mopo.py:81-84); the row keeps
  // its Philox counter, only the range and the base pointers change
  const bool mdl = p.m.obs && row >= p.real_rows;
  const ModelSrc m = orl_model_src(p.m_tab, r, p.m);
  const float *s_obs = mdl ? m.obs : p.src.obs, *s_nobs = mdl ? m.nobs : p.src.nobs, *s_act = mdl ? m.act : p.src.act;
  const float *s_rew = mdl ? m.rew : p.src.rew, *s_term = mdl ? m.term : p.src.term;
  const int OP = p.src.OP, AP = p.src.AP, od = p.src.od, ad = p.src.ad;
  long j;
  if (p.idx) j = p.idx[(long)r * p.idx_rs + row];
  else {
    const unsigned long long ctr = p.gstep ? *p.gstep : p.counter;
    const long n = mdl ? (long)*m.n : p.n;
    Philox ph(p.seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(r + 1));
    uint32_t o[4];
    ph((uint32_t)row, 0x51u, (uint32_t)ctr, 0x1D5u ^ (uint32_t)(ctr >> 32), o);
    j = (long)(((unsigned long long)o[0] * (unsigned long long)n) >> 32);
  }
  if (c < p.d_op) {
    const float vo = c < od ? s_obs[j * OP + c] : 0.f, vn = c < od ? s_nobs[j * OP + c] : 0.f;
    p.b_obs[(long)r * p.obs_rs + (long)row * p.d_op + c] = vo;
    p.b_nobs[(long)r * p.nobs_rs + (long)row * p.d_op + c] = vn;
  }
  if (c < p.d_ap) p.b_act[(long)r * p.act_rs + (long)row * p.d_ap + c] = c < ad ? s_act[j * AP + c] : 0.f;
  if (c == 0) { p.b_rew[(long)r * p.rew_rs + row] = s_rew[j]; p.b_term[(long)r * p.term_rs + row] = s_term[j]; }
}

// one draw of `batch` rows into packed device arrays on `stream`: the rows idx[] or, without, Philox draws keyed by (seed, row, the
// buffer's draw counter), which advances.  orl_buffer_sample and the RAMBO device loop share it
int buffer_gather(Buffer& b, const long long* idx_dev, int batch, uint64_t seed, float* obs_out, float* act_out, float* next_obs_out,
                  float* rew_out, float* term_out, hipStream_t stream);
// max |x| over the obs / next_obs / act arrays (reward = false) or over the reward column (true) of the buffer's current generation:
// one reduction over the HBM arrays per generation (40 us), then the cached value.  A NaN sticks.
int buffer_absmax(Buffer& b, bool reward, float* out);

}  // namespace orl

struct orl_buffer {
  orl::Buffer b;
};
struct orl_traj {
  orl::Traj t;
};
