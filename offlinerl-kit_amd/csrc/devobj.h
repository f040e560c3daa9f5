// devobj.h — the host layer under every device object of the C ABI (engine.h, dynamics.hip, diffusion.hip): error plumbing, the
// tracked allocator, the parameter block's tensor table, flat-block transfers, call staging, the GemmP of a linear layer's three
// products from matrix views with their workspace matrices and tile choice, and the learn-epoch driver.  A new stand-alone model starts from these instead of copying them ("Device-object layer").
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/orl_engine.h"
#include "gemm.h"

namespace orl {

void set_error(const std::string& msg);   // engine.hip: the text orl_last_error() returns
int fail(const std::string& msg);         // set_error, returns -1
// store.hip: the dataset rows a DiffusionBC gathers (device, dims, pitches, size, the obs / act arrays)
void buffer_view(const orl_buffer* b, int* dev, int* od, int* ad, int* OP, int* AP, long* n, const float** obs, const float** act);

// While a lease lives, the launches of an orl_dynamics (dynamics.hip) go to `loop_stream` -- the engine's, so that one stream orders a
// whole device loop; the destructor hands the object's own stream back on every return path.
struct DynStreamLease {
  orl_dynamics* d;
  hipStream_t own;
  DynStreamLease(orl_dynamics* d, hipStream_t loop_stream);
  ~DynStreamLease();
};

// The adversarial pair of an orl_dynamics (dynamics.hip) as the RAMBO device loop drives it under a DynStreamLease (algo_rambo.inc:
// Engine::rambo_loop): the launches of orl_dynadv_forward / orl_dynadv_update on device arrays, without their staging, synchronisation
// and metric read-back.  loop_begin (before the lease) uploads the optimizer's step counts, update_enqueue(step) is Adam step
// t0 + step + 1, loop_end adds the steps done to the host's count.
struct DynAdvInfo {
  int dev, R, od, ad, Ba, Bs;
  bool on;                 // orl_dynadv_configure has run
  hipStream_t stream;      // the object's own stream
  const float* metrics;    // device [R][4] of the last update: all_loss, sl_loss, adv_loss, mean log_prob
};
int dynadv_info(orl_dynamics* d, DynAdvInfo* out);
int dynadv_loop_begin(orl_dynamics* d);
int dynadv_forward_enqueue(orl_dynamics* d, const float* obs, const float* act, const float* sl_obs, const float* sl_act,
                           const float* sl_next_obs, const float* sl_rew, float* next_obs, float* reward);
int dynadv_update_enqueue(orl_dynamics* d, const float* advantage, int step);
void dynadv_loop_end(orl_dynamics* d, long steps_done);

// The trajectory store (store.hip) as the MBRCSL rollout loop drives it (algo_autoreg.inc: Engine::mbrcsl_loop):
// orl_traj_append_step_counted's two launches on `stream` (`who` prefixes the refusals), and what the loop checks and reads of the store
// -- `survivors` is the device cell that holds the survivor count of the last step enqueued.
struct TrajInfo { int dev, od, ad; long n_traj_cap, cap; const long long* survivors; };
int traj_info(orl_traj* t, TrajInfo* out);
int traj_append_enqueue(orl_traj* t, hipStream_t stream, int term_kind, const float* obs, const float* act, const float* next_obs,
                        const float* rew, long bound, float* alive_next_obs, const char* who);

// orl_dyn_step (dynamics.hip) as the same loop drives it under a DynStreamLease: device rows in, next_obs / reward out, no staging and
// no synchronisation.  loop_begin (before the lease, on the object's own stream) grows the step workspaces for n_max rows, every
// enqueue advances the call counter as orl_dyn_step does.
struct DynStepInfo { int dev, R, od, ad; bool with_reward; hipStream_t stream; };
int dynstep_info(orl_dynamics* d, DynStepInfo* out);
int dynstep_loop_begin(orl_dynamics* d, long n_max);
int dynstep_enqueue(orl_dynamics* d, const float* obs, const float* act, long n, int mode, float coef, float* next_obs, float* reward);

// orl_dynsample_next (dynamics.hip) as the MOBILE device loop drives it under a DynStreamLease (algo_mobile.inc: Engine::mobile_loop):
// the input rows are the policy engine's pitched batch slots (row b of run r at obs + r obs_rs + b obs_pitch), and the S * E * n samples
// go straight into the operands of the penalty pass -- xs [R][S E n][OP] and the observation columns of xl [R][S E n][XP], pads zeroed,
// the action columns of xl left alone -- instead of a packed [R][S E n][od] array.  No staging and no synchronisation; the step
// workspaces are grown before the loop (dynstep_loop_begin), every enqueue advances the sample call counter as orl_dynsample_next does
// and takes its refusals (`who` prefixes them).
struct DynSampleInfo { int dev, R, od, ad, n_elites; bool with_reward; hipStream_t stream; };
int dynsample_info(orl_dynamics* d, DynSampleInfo* out);
struct DynSampleRows {
  const float* obs; long obs_rs; int obs_pitch;
  const float* act; long act_rs; int act_pitch;
  long n; int num_samples;
  float* xs; long xs_rs; int OP;
  float* xl; long xl_rs; int XP;
};
int dynsample_enqueue(orl_dynamics* d, const DynSampleRows& rows, const char* who);

#define ORL_HIP(expr)                                                                           \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) {                                                                      \
      ::orl::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                       \
      return -1;                                                                                 \
    }                                                                                            \
  } while (0)
// one kernel launch on `stream` with `lds` dynamic LDS bytes, and its check (engine.hip's ORL_LAUNCH is the profiled one)
#define DEV_LAUNCH(stream, kernel, grid, block, lds, ...)                                        \
  do {                                                                                           \
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                           \
    if (hipGetLastError() != hipSuccess) return ::orl::fail(#kernel ": launch failed");          \
  } while (0)

static inline int rup4(int x) { return (x + 3) & ~3; }

// The frame of a device loop: a run of launches on one stream between two timing events, with one host synchronisation at its end.
// begin: `stream` waits for what each of `wait_for` holds so far, then the start event is recorded.  end(rc of the launches, ...):
// records the stop event, synchronises once -- also when the launches failed: those made so far ran -- and returns -1 for rc != 0 or,
// with "<who>: <hip error>", for a failed synchronisation; on success *elapsed_ms (may be null) is the time between the two events.
struct LoopScope {
  hipStream_t stream = nullptr;
  hipEvent_t a = nullptr, b = nullptr, order = nullptr;
  ~LoopScope() { for (hipEvent_t x : {a, b, order}) if (x) hipEventDestroy(x); }
  int begin(hipStream_t s, std::initializer_list<hipStream_t> wait_for) {
    stream = s;
    ORL_HIP(hipEventCreate(&a));
    ORL_HIP(hipEventCreate(&b));
    if (wait_for.size()) ORL_HIP(hipEventCreateWithFlags(&order, hipEventDisableTiming));
    for (hipStream_t w : wait_for) {
      ORL_HIP(hipEventRecord(order, w));
      ORL_HIP(hipStreamWaitEvent(stream, order, 0));
    }
    ORL_HIP(hipEventRecord(a, stream));
    return 0;
  }
  int end(int rc, const char* who, float* elapsed_ms) {
    const hipError_t re = rc ? hipSuccess : hipEventRecord(b, stream);
    const hipError_t se = hipStreamSynchronize(stream);
    if (rc) return -1;
    if (re != hipSuccess || se != hipSuccess) return fail(std::string(who) + ": " + hipGetErrorString(re != hipSuccess ? re : se));
    float ms = 0.f;
    ORL_HIP(hipEventElapsedTime(&ms, a, b));
    if (elapsed_ms) *elapsed_ms = ms;
    return 0;
  }
};

// Device allocations of one object.  alloc: zero-filled, an empty request gets 16 bytes; `who` prefixes the error texts.
struct DevAllocs {
  const char* who;
  std::vector<void*> ptrs;
  template <class T>
  int alloc(T** p, size_t count) {
    const size_t bytes = sizeof(T) * count, nb = bytes ? bytes : 16;
    if (hipMalloc((void**)p, nb) != hipSuccess) return fail(std::string(who) + ": hipMalloc of " + std::to_string(bytes) + " bytes failed");
    if (hipMemset(*p, 0, nb) != hipSuccess) return fail(std::string(who) + ": hipMemset failed");
    // the fill runs on the null stream and need not have finished when hipMemset returns; the objects' own streams are non-blocking, so
    // a kernel of theirs that writes the new array is not ordered behind it (a late fill would zero what the kernel wrote)
    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(std::string(who) + ": hipMemset failed");
    ptrs.push_back(*p);
    return 0;
  }
  void free(void* p) {
    if (!p) return;
    for (auto it = ptrs.begin(); it != ptrs.end(); ++it)
      if (*it == p) { ptrs.erase(it); break; }
    hipFree(p);
  }
  template <class... T>
  void release(T**... ps) { ((free(*ps), *ps = nullptr), ...); }
  // grow on demand: when n elements do not fit, wait for the stream, then replace *p by a fresh array of n and record the capacity
  template <class T>
  int grow(T** p, long* cap, long n, hipStream_t stream) {
    if (n <= *cap) return 0;
    ORL_HIP(hipStreamSynchronize(stream));
    release(p);
    *cap = 0;
    if (alloc(p, (size_t)n)) return -1;
    *cap = n;
    return 0;
  }
  void free_all() {
    for (void* p : ptrs) hipFree(p);
    ptrs.clear();
  }
};

// The tensors of a parameter block in state_dict order: what orl_net_tensor / orl_dyn_tensor / orl_diffusion_tensor answer from.
struct TensorInfo {
  std::string name;
  long off;
  int ndim;
  long shape[4];
};
struct TensorTable {
  std::vector<TensorInfo> rows;
  long off = 0;      // running offset of add()
  int size() const { return (int)rows.size(); }
  // a tensor at an offset the caller laid out
  void put(const std::string& name, long at, std::initializer_list<long> shape) {
    TensorInfo t{name, at, (int)shape.size(), {1, 1, 1, 1}};
    int i = 0;
    for (long s : shape) t.shape[i++] = s;
    rows.push_back(t);
  }
  long align4() { return off = (off + 3) & ~3L; }
  // the next tensor of a packed block, returns its offset.  align_start: it begins on 4 floats (16 bytes); pad_size: it also ends there
  long add(const std::string& name, std::initializer_list<long> shape, bool align_start, bool pad_size) {
    if (align_start) align4();
    const long at = off;
    long n = 1;
    for (long s : shape) n *= s;
    put(name, at, shape);
    off += n;
    if (pad_size) align4();
    return at;
  }
  // 1 when idx is out of range (the entry point words its own error); shape slots past ndim read 1
  int query(int idx, char* name, int name_cap, int64_t* offset, int32_t* ndim, int64_t shape[4]) const {
    if (idx < 0 || idx >= size()) return 1;
    const TensorInfo& t = rows[idx];
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", t.name.c_str());
    if (offset) *offset = t.off;
    if (ndim) *ndim = t.ndim;
    if (shape) for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
    return 0;
  }
};

// a flat float block to / from the host once the stream has drained
static inline int block_to_host(hipStream_t stream, float* host, const float* dev, long floats) {
  ORL_HIP(hipStreamSynchronize(stream));
  ORL_HIP(hipMemcpy(host, dev, sizeof(float) * floats, hipMemcpyDeviceToHost));
  return 0;
}
static inline int block_from_host(hipStream_t stream, float* dev, const float* host, long floats) {
  ORL_HIP(hipStreamSynchronize(stream));
  ORL_HIP(hipMemcpy(dev, host, sizeof(float) * floats, hipMemcpyHostToDevice));
  return 0;
}

// Staging of a call's arrays.  In: a host array is copied to `stage` on the stream and p repointed there; a device array (on_device)
// or a null one stays.  stage_dst: where the kernel writes an output; out: the staged output copied back to the host on the stream.
template <class T>
static int stage_in(hipStream_t stream, const T*& p, T* stage, size_t count, int on_device) {
  if (on_device || !p) return 0;
  ORL_HIP(hipMemcpyAsync(stage, p, sizeof(T) * count, hipMemcpyHostToDevice, stream));
  p = stage;
  return 0;
}
template <class T>
static T* stage_dst(T* user, T* stage, int on_device) { return user && !on_device ? stage : user; }
template <class T>
static int stage_out(hipStream_t stream, T* user, const T* stage, size_t count, int on_device) {
  if (on_device || !user) return 0;
  ORL_HIP(hipMemcpyAsync(user, stage, sizeof(T) * count, hipMemcpyDeviceToHost, stream));
  return 0;
}

// ---- a linear layer's products on the tiled GEMM (gemm.h) ----
// [z0][z1][rows][pitch] matrix (strides s0, s1; both 0: one matrix) or a column slice of one; lim = floats readable from p within a row
struct DevMat {
  float* p = nullptr;
  long s0 = 0, s1 = 0;
  int pitch = 0, lim = 0;
  DevMat cols(int c0) const { DevMat m = *this; m.p += c0; m.lim -= c0; return m; }
  ZPtr z() const { return {p, s0, s1}; }
};
// weight and bias of a layer (or their gradients) batched like the matrices.  in_major: EnsembleLinear's (in, out)-major weight,
// else nn.Linear's (out, in)-major one (the l.ens distinction of Engine::linear_fwd)
struct LinearP {
  ZOut w, b;
  int in, out;
  bool in_major;
  int members;       // z1 extent (GemmP::nz1)
};
static inline GemmP gemm_zero() {
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.ksplit = 1;
  return p;
}
// Y = X W + b.  Epilogue fields (z_out), tile choice and a_kpad are the caller's.  In the forward and the dgrad b_rlim is set exactly
// where the weight's rows are contiguous along N: it lets launch_gemm pick the 4-row block loader.
static inline GemmP linear_fwd_p(const DevMat& X, int M, const LinearP& l, const DevMat& Y) {
  GemmP p = gemm_zero();
  p.A = X.z(); p.a_sr = X.pitch; p.a_sk = 1;
  p.B = {l.w.p, l.w.s0, l.w.s1};
  if (l.in_major) { p.b_sr = 1; p.b_sk = l.out; p.b_rlim = l.out & ~3; }
  else { p.b_sr = l.in; p.b_sk = 1; }
  p.C = Y.p; p.c_s0 = Y.s0; p.c_s1 = Y.s1; p.c_sr = Y.pitch; p.c_sn = 1;
  p.M = M; p.N = l.out; p.K = l.in; p.nz1 = l.members;
  p.bias = {l.b.p, l.b.s0, l.b.s1};
  return p;
}
// dX = dY W^T (the caller adds aux for a masked epilogue)
static inline GemmP linear_dgrad_p(const DevMat& dY, int M, const LinearP& l, const DevMat& dX) {
  GemmP p = gemm_zero();
  p.A = dY.z(); p.a_sr = dY.pitch; p.a_sk = 1;
  p.B = {l.w.p, l.w.s0, l.w.s1};
  if (l.in_major) { p.b_sr = l.out; p.b_sk = 1; }
  else { p.b_sr = 1; p.b_sk = l.in; p.b_rlim = l.in & ~3; }
  p.C = dX.p; p.c_s0 = dX.s0; p.c_s1 = dX.s1; p.c_sr = dX.pitch; p.c_sn = 1;
  p.M = M; p.N = l.in; p.K = l.out; p.nz1 = l.members;
  return p;
}
// dW = X^T dY in the weight's own layout and db = the column sums of dY, into the gradient blocks g.w / g.b
static inline GemmP linear_wgrad_p(const DevMat& dY, const DevMat& X, int M, const LinearP& g) {
  GemmP p = gemm_zero();
  p.A = dY.z(); p.a_sr = 1; p.a_sk = dY.pitch; p.a_rlim = dY.lim & ~3;
  p.B = X.z(); p.b_sr = 1; p.b_sk = X.pitch; p.b_rlim = X.lim & ~3;
  p.ones_row = 1 << 30;
  p.M = g.out; p.N = g.in; p.K = M; p.nz1 = g.members;
  p.C = g.w.p; p.c_s0 = g.w.s0; p.c_s1 = g.w.s1;
  if (g.in_major) { p.c_sr = 1; p.c_sn = g.out; }
  else { p.c_sr = g.in; p.c_sn = 1; }
  p.bias_out = g.b.p; p.bo_s0 = g.b.s0; p.bo_s1 = g.b.s1;
  return p;
}
static inline int gemm_done(hipError_t e, const char* what) {
  return e == hipSuccess ? 0 : fail(std::string(what) + " gemm: " + hipGetErrorString(e));
}
// a zero-filled [runs][rows][rup4(cols)] matrix (s0: the run stride) in place of whatever v held
static inline int dev_mat(DevAllocs& mem, DevMat& v, long rows, int cols, int runs = 1) {
  mem.free(v.p);
  v.pitch = v.lim = rup4(cols);
  v.s0 = rows * v.pitch;
  return mem.alloc(&v.p, (size_t)runs * rows * v.pitch);
}
// Tile choice of the forward and dgrad products.  pick_cfg's rule for long reductions (K >= 1024 -> 256 x 128 tiles) is meant for
// split weight gradients; at 256 rows it leaves a 1024-wide layer with 8 workgroups.  Few rows: 16 x 64 tiles while they give at most
// four rounds of workgroups on the 256 CUs, 64 x 64 beyond; many rows (a large sampling batch): the 64 x 256 forward tile.
static inline int linear_cfg(int M, int N) {
  if (N <= 16) return CFG_TALL;
  if (M >= 2048 && N >= 128) return CFG_BIG;
  const long small_tiles = (long)((M + 15) / 16) * ((N + 63) / 64);
  return (M <= 32 || small_tiles <= 1024) ? CFG_SMALL : CFG_MID;
}
// blocks of 256 threads over n elements
static inline int ew_grid(long n) { return (int)((n + 255) / 256); }

// One epoch of R runs in steps of B rows, without a host round trip: run r visits the rows orders[r][0 .. n_rows) of its n_data (host
// indices are checked, device ones are the kernels' to clamp).  The orders go to idx_d ([R][n_rows], grown on demand) in one copy,
// enqueue(idx_d + s B, rows, loss_steps + s R) queues step s (run r's indices start r n_rows entries past the pointer it is given), and
// the [steps][R] losses come back after one synchronisation.  `what` names the entry point in the errors.
template <class Enqueue>
static int learn_epoch_steps(hipStream_t stream, DevAllocs& mem, long long** idx_d, long* idx_cap, float** loss_steps, long* loss_cap, int B,
                             long n_data, int R, const char* what, const int64_t* orders, int64_t n_rows, int on_device, float* losses_out,
                             Enqueue enqueue) {
  const std::string w(what);
  if (!orders || n_rows < 1) return fail(w + ": bad arguments");
  if (!on_device)
    for (int64_t i = 0; i < R * n_rows; ++i)
      if (orders[i] < 0 || orders[i] >= n_data) return fail(w + ": row index out of range");
  const long steps = (long)((n_rows + B - 1) / B);
  if (mem.grow(idx_d, idx_cap, (long)R * std::max<long>((long)n_rows, B), stream)) return -1;
  if (mem.grow(loss_steps, loss_cap, steps * R, stream)) return -1;
  ORL_HIP(hipMemcpyAsync(*idx_d, orders, sizeof(int64_t) * R * n_rows, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  for (long s = 0; s < steps; ++s) {
    const int rows = (int)std::min<int64_t>(B, n_rows - s * B);
    if (enqueue(*idx_d + s * B, rows, *loss_steps + s * R)) return -1;
  }
  ORL_HIP(hipStreamSynchronize(stream));
  if (losses_out) ORL_HIP(hipMemcpy(losses_out, *loss_steps, sizeof(float) * steps * R, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace orl
