// store.hip — the row stores of the C ABI (store.h): orl_buffer_* (a loaded dataset or a growable model-rollout ring) and orl_traj_*
// (the trajectory store of the RCSL rollout), with the kernels only they launch.
#include "store.h"

#include <limits.h>
#include <math.h>

namespace orl {

// ------------------------------------------------------------------------------------------------
// one model-rollout step's bookkeeping (policy/model_based/mopo.py:45-79) on the device, ONE core for the ring's rollout append and
// the trajectory store's step: the termination test of utils/termination_fns.py on next_obs, all n transitions appended to the store,
// the next_obs rows of the transitions that did NOT terminate compacted densely and IN THEIR ORIGINAL ORDER (the dynamics' Philox draws
// are keyed by row position), their count and the float64 sum of the rewards.  Two passes over ceil(n / 256) blocks: term_count writes
// the 0 / 1 terminals and per-block (alive count, reward sum); the second turns the counts of the blocks in front of it into its
// offset and ranks its own rows with wave ballots (orl_stable_rank), copies (scatter_rows) and sums the blocks (block_totals).  A fixed
// block order, no tickets: the result does not depend on which block runs first.  Sources are packed [n][od] / [n][ad] arrays (not
// 16-byte aligned at od = 17), so the copies are coalesced scalar loads; the pad columns of the stored rows are written as zeros.
// ------------------------------------------------------------------------------------------------
// where source row i of a call lands: a compile-time choice, so only the ring pays the 64-bit remainder
struct RingRow { long ptr, cap; __device__ long operator()(long i) const { return (ptr + i) % cap; } };
struct FlatRow { long row0; __device__ long operator()(long i) const { return row0 + i; } };

// First pass, one call per kernel by EVERY thread of a 256-thread block (barrier inside): the verdict of row i = blockIdx.x * 256 +
// threadIdx.x into term[at(i)], then this block's alive count and reward sum -- lanes by the shuffle tree o = 32 .. 1, waves as
// ((w0 + w1) + w2) + w3 -- into *blk_cnt / *blk_rew.
template <class RowMap>
__device__ inline void term_count(int kind, const float* s_nobs, const float* s_rew, int od, long n, float* term, RowMap at, int* blk_cnt,
                                  double* blk_rew) {
  __shared__ int sh_a[4];
  __shared__ double sh_r[4];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool alive = false;
  double rw = 0.0;
  if (i < n) {
    const bool done = orl_term_done(kind, s_nobs + i * od, od);
    term[at(i)] = done ? 1.0f : 0.0f;
    alive = !done;
    rw = (double)s_rew[i];
  }
  const unsigned long long m = __ballot(alive);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rw += __shfl_down(rw, o, 64);
  if ((threadIdx.x & 63) == 0) { sh_a[threadIdx.x >> 6] = __popcll(m); sh_r[threadIdx.x >> 6] = rw; }
  __syncthreads();
  if (threadIdx.x == 0) {
    *blk_cnt = sh_a[0] + sh_a[1] + sh_a[2] + sh_a[3];
    *blk_rew = ((sh_r[0] + sh_r[1]) + sh_r[2]) + sh_r[3];
  }
}
// The stable rank of a flagged row among ALL flagged rows of a launch of 256-thread blocks, -1 for a row that is not flagged: the flagged
// rows of the blocks in front (blk_cnt[0 .. blockIdx.x), written by the counting pass; integers, so the order of the sum does not
// matter), those of the waves in front within the block, and the wave-ballot rank (64 lanes, 64-bit masks).  Every thread of the block
// calls it, once per kernel (it owns its shared memory and has barriers inside).  k_roll_scatter, k_traj_scatter and k_traj_export
// compact with it.
__device__ inline int orl_stable_rank(bool flag, const int* blk_cnt) {
  __shared__ int sh_part[256];
  __shared__ int sh_w[4];
  const int tid = threadIdx.x;
  int part = 0;
  for (int b = tid; b < (int)blockIdx.x; b += 256) part += blk_cnt[b];
  sh_part[tid] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sh_part[tid] += sh_part[tid + o];
    __syncthreads();
  }
  const int blk_off = sh_part[0];
  const unsigned long long m = __ballot(flag);
  const int lane = tid & 63, w = tid >> 6;
  if (lane == 0) sh_w[w] = __popcll(m);
  __syncthreads();
  int woff = 0;
  for (int k = 0; k < w; ++k) woff += sh_w[k];
  return flag ? blk_off + woff + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}
// Second pass, again one call per kernel by every thread of the block (barrier inside): the block's rows of a call of n into the store
// `d` at rows at(.) -- obs / next_obs with zeroed pad columns, act, the reward -- and the next_obs of the rows with a rank (`rank`: this
// thread's row, from orl_stable_rank) into alive_nobs[rank].
template <class RowMap>
__device__ inline void scatter_rows(const Rows& d, RowMap at, const float* s_obs, const float* s_act, const float* s_nobs, const float* s_rew,
                                    long n, int rank, float* alive_nobs) {
  __shared__ int sh_dst[256];
  const int tid = threadIdx.x;
  const long b0 = (long)blockIdx.x * 256, i = b0 + tid;
  sh_dst[tid] = rank;
  __syncthreads();
  const int rows = (int)(n - b0 < 256 ? n - b0 : 256);
  for (int e = tid; e < rows * d.OP; e += 256) {
    const int row = e / d.OP, c = e - row * d.OP;
    const long src = (b0 + row) * d.od + c, dst = at(b0 + row) * d.OP + c;
    d.obs[dst] = c < d.od ? s_obs[src] : 0.f;
    d.nobs[dst] = c < d.od ? s_nobs[src] : 0.f;
  }
  for (int e = tid; e < rows * d.AP; e += 256) {
    const int row = e / d.AP, c = e - row * d.AP;
    d.act[at(b0 + row) * d.AP + c] = c < d.ad ? s_act[(b0 + row) * d.ad + c] : 0.f;
  }
  for (int e = tid; e < rows * d.od; e += 256) {
    const int row = e / d.od, c = e - row * d.od;
    const int dd = sh_dst[row];
    if (dd >= 0) alive_nobs[(long)dd * d.od + c] = s_nobs[(b0 + row) * d.od + c];
  }
  if (i < n) d.rew[at(i)] = s_rew[i];
}
// the totals of a call, by one thread: blocks in index order starting from 0.0 (a few hundred terms at 50 000 rows)
__device__ inline void block_totals(const int* blk_cnt, const double* blk_rew, int nb, long long* n_alive, double* rew_sum) {
  long long na = 0; double rs = 0.0;
  for (int b = 0; b < nb; ++b) { na += blk_cnt[b]; rs += blk_rew[b]; }
  *n_alive = na; *rew_sum = rs;
}

// The ring's rollout append (orl_buffer_append_rollout, orl_buffer_append_rollout_runs): blockIdx.y is the run, the sources are
// [runs][row_stride][dim] arrays of which run r owns the first n rows of its ring entry, and the ring of a run is read from a table in
// device memory (uploaded per call: at 128 runs it does not fit the kernel arguments) or, for the single ring, from the launch
// parameters.  A block whose first row lies at or past its run's row count leaves before any barrier (the test is uniform per block);
// the per-block scratch is [runs][gridDim.x] and the totals of a run are summed over the blocks that had rows, in block order.
struct RollRing {
  Rows c; long cap, ptr;                 // the ring
  long n;                                // rows of this call
  long long* size_cell; long long size;  // the ring's device size cell and its value after this call
};
struct RollP {
  int kind;
  const float *obs, *act, *nobs, *rew;   // packed [runs][row_stride][od], [..][ad], [..][od], [runs][row_stride]
  long row_stride;
  RollRing ring;                         // tab == nullptr: the one ring (gridDim.y == 1)
  const RollRing* tab;                   // [gridDim.y], device memory
  float* alive_nobs;                     // [runs][row_stride][od] packed, run r compacted into its own block; must not overlap nobs
  int* blk_alive; double* blk_rew;       // [gridDim.y][gridDim.x] scratch
  long long* n_alive_out; double* rew_sum_out;   // [gridDim.y]
};
__global__ void k_roll_term(RollP p) {
  const int r = blockIdx.y;
  const RollRing g = p.tab ? p.tab[r] : p.ring;
  if ((long)blockIdx.x * 256 >= g.n) return;
  const long cell = (long)r * gridDim.x + blockIdx.x;
  term_count(p.kind, p.nobs + (long)r * p.row_stride * g.c.od, p.rew + (long)r * p.row_stride, g.c.od, g.n, g.c.term, RingRow{g.ptr, g.cap},
             p.blk_alive + cell, p.blk_rew + cell);
}
__global__ void k_roll_scatter(RollP p) {
  const int r = blockIdx.y;
  const RollRing g = p.tab ? p.tab[r] : p.ring;
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;      // reports the run's totals and publishes the ring's new size
  long long na = 0; double rs = 0.0;
  if ((long)blockIdx.x * 256 < g.n) {
    const long s_od = (long)r * p.row_stride * g.c.od, i = (long)blockIdx.x * 256 + threadIdx.x;
    const int* blk_alive = p.blk_alive + (long)r * gridDim.x;
    const RingRow at{g.ptr, g.cap};
    const bool alive = i < g.n && g.c.term[at(i)] == 0.0f;
    scatter_rows(g.c, at, p.obs + s_od, p.act + (long)r * p.row_stride * g.c.ad, p.nobs + s_od, p.rew + (long)r * p.row_stride, g.n,
                 orl_stable_rank(alive, blk_alive), p.alive_nobs + s_od);
    if (first) block_totals(blk_alive, p.blk_rew + (long)r * gridDim.x, (int)((g.n + 255) / 256), &na, &rs);
  }                                       // (a run without rows: its block 0 still reports, zeros)
  if (first) { p.n_alive_out[r] = na; p.rew_sum_out[r] = rs; *g.size_cell = g.size; }
}

// ------------------------------------------------------------------------------------------------
// the trajectory store (orl_traj): the bookkeeping of the RCSL rollout (policy/rcsl/rcsl.py:57-120) on the device.  A row carries, next to
// the transition, its trajectory, the return accumulated BEFORE it and -- after k_traj_finish -- its return-to-go; returns / accumulated
// returns are float64 because the host keeps them in np.zeros arrays (float64 + float32 promoted, one add per step: the same rounding).
// A step is the launch pair of the ring rollout on flat rows: k_traj_term, then k_traj_scatter, which adds the stable compaction of the
// live (trajectory, accumulated return) pairs into the other half of the ping-pong arrays.  A trajectory has at most one live row, so
// returns[] is updated by a plain read-add-store.  The export is the same two-pass compaction over the stored rows: k_traj_count /
// k_traj_total count (the host refuses a ring that is too small before a row is written), k_traj_export scatters.  Fixed block order
// everywhere, no tickets, no atomics.
// ------------------------------------------------------------------------------------------------
enum { CELL_LIVE = 3, CELL_ROWS = 5, CELL_OVERFLOW = 7, TRAJ_CELLS = 8 };
struct TrajP {
  Rows c; int* tidx; double *acc, *rtg;                                  // the rows: [cap][OP], [cap][OP], [cap][AP], [cap] each
  double* returns;                                                       // [n_traj]
  long n_traj;
  const int* live_idx; const double* live_acc;                           // the live trajectories of this step, [n]
  int* next_idx; double* next_acc;                                       // ... of the next one (the other half)
  int kind;
  const float *s_obs, *s_act, *s_nobs, *s_rew;                           // packed sources [n][od], [n][ad], [n][od], [n]
  long row0, n;                                                          // step: rows [row0, row0 + n) are appended; finish / export: rows [0, n)
  long cap; int half;                                                    // counted step: the store's row capacity, the parity of the step
  float* alive_nobs;
  int* blk_cnt; double* blk_rew;                                         // per-block scratch
  long long* cells;                                                      // [0] survivors of the step, [1] rows kept, [2] trajectories kept,
                                                                         // [3 + h] live count, [5 + h] rows written (h: step parity), [7] overflow
  double* rew_total;                                                     // running sum of every appended reward
  int use_thr; double thr;                                               // export: keep rows of trajectories with returns > thr
  Rows d; long d_row0;                                                   // export: the destination ring (same pitches) and its first free row
};
__global__ void k_traj_reset(TrajP p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < p.n_traj) { p.returns[i] = 0.0; p.next_idx[i] = (int)i; p.next_acc[i] = 0.0; }
  if (i == 0) { *p.rew_total = 0.0; p.cells[CELL_LIVE + (p.half ^ 1)] = p.n_traj; p.cells[CELL_ROWS + (p.half ^ 1)] = 0; p.cells[CELL_OVERFLOW] = 0; }
}
// The rows of a step and where they go.  Host-counted (orl_traj_append_step): both by value.  COUNTED (orl_traj_append_step_counted): the
// launch covers p.n rows, a host-known upper bound; the live count and the rows written so far come from the cells of the step's parity,
// which no block of this step writes (block 0 of k_traj_scatter publishes the next step's values into the other pair while blocks of
// its launch may still be reading).  The count is clamped to the bound and to the room left; either clamp raises the sticky overflow cell.
struct StepRows { long row0, n; bool over; };
template <bool COUNTED>
__device__ inline StepRows step_rows(const TrajP& p) {
  if (!COUNTED) return {p.row0, p.n, false};
  const long live = (long)p.cells[CELL_LIVE + p.half], row0 = (long)p.cells[CELL_ROWS + p.half];
  long n = live < p.n ? live : p.n;
  if (n > p.cap - row0) n = p.cap - row0;
  if (n < 0) n = 0;
  return {row0, n, n != live};
}
template <bool COUNTED>
__global__ void k_traj_term(TrajP p) {
  const StepRows s = step_rows<COUNTED>(p);
  term_count(p.kind, p.s_nobs, p.s_rew, p.c.od, s.n, p.c.term, FlatRow{s.row0}, p.blk_cnt + blockIdx.x, p.blk_rew + blockIdx.x);
}
template <bool COUNTED>
__global__ void k_traj_scatter(TrajP p) {
  const StepRows s = step_rows<COUNTED>(p);
  p.row0 = s.row0; p.n = s.n;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const FlatRow at{p.row0};
  const bool alive = i < p.n && p.c.term[at(i)] == 0.0f;
  const int d = orl_stable_rank(alive, p.blk_cnt);
  scatter_rows(p.c, at, p.s_obs, p.s_act, p.s_nobs, p.s_rew, p.n, d, p.alive_nobs);
  if (i < p.n) {
    const int t = p.live_idx[i];
    const double a = p.live_acc[i], r = (double)p.s_rew[i];
    p.tidx[at(i)] = t;
    p.acc[at(i)] = a;
    p.returns[t] = p.returns[t] + r;        // (the only live row of trajectory t)
    if (d >= 0) { p.next_idx[d] = t; p.next_acc[d] = a + r; }
  }
  if (i == 0) {
    long long na; double rs;
    block_totals(p.blk_cnt, p.blk_rew, (int)gridDim.x, &na, &rs);
    p.cells[0] = na;
    p.cells[CELL_LIVE + (p.half ^ 1)] = na;
    p.cells[CELL_ROWS + (p.half ^ 1)] = p.row0 + p.n;
    if (s.over) p.cells[CELL_OVERFLOW] = 1;
    *p.rew_total = *p.rew_total + rs;
  }
}
__global__ void k_traj_finish(TrajP p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < p.n) p.rtg[i] = p.returns[p.tidx[i]] - p.acc[i];
}
// orl_traj_live: the live trajectory indices, widened to int64 (an index tensor for a per-trajectory table)
__global__ void k_traj_live(const int* __restrict__ live_idx, long n, long long* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = live_idx[i];
}
// (a NaN return is not above any threshold, as in numpy)
__device__ inline bool orl_traj_keep(int use_thr, double thr, const double* returns, int t) { return !use_thr || returns[t] > thr; }
__global__ void k_traj_count(TrajP p) {
  __shared__ int sh_a[4];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const bool keep = i < p.n && orl_traj_keep(p.use_thr, p.thr, p.returns, p.tidx[i]);
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) sh_a[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) p.blk_cnt[blockIdx.x] = sh_a[0] + sh_a[1] + sh_a[2] + sh_a[3];
}
// one block: the kept rows (the sum of k_traj_count's `nblk` block counts) and the kept trajectories
__global__ void k_traj_total(TrajP p, long nblk) {
  __shared__ long long sh_r[256], sh_t[256];
  const int tid = threadIdx.x;
  long long r = 0, t = 0;
  for (long b = tid; b < nblk; b += 256) r += p.blk_cnt[b];
  for (long j = tid; j < p.n_traj; j += 256) t += orl_traj_keep(p.use_thr, p.thr, p.returns, (int)j) ? 1 : 0;
  sh_r[tid] = r; sh_t[tid] = t;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { sh_r[tid] += sh_r[tid + o]; sh_t[tid] += sh_t[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) { p.cells[1] = sh_r[0]; p.cells[2] = sh_t[0]; }
}
// kept rows -> ring rows d_row0 + rank (the host has checked that they fit without wrapping), rew := (float)rtg
__global__ void k_traj_export(TrajP p) {
  __shared__ int sh_dst[256];
  const int tid = threadIdx.x;
  const long b0 = (long)blockIdx.x * 256, i = b0 + tid;
  const int OP = p.c.OP, AP = p.c.AP;
  const bool keep = i < p.n && orl_traj_keep(p.use_thr, p.thr, p.returns, p.tidx[i]);
  const int d = orl_stable_rank(keep, p.blk_cnt);
  sh_dst[tid] = d;
  __syncthreads();
  const int rows = (int)(p.n - b0 < 256 ? p.n - b0 : 256);
  for (int e = tid; e < rows * OP; e += 256) {
    const int row = e / OP, c = e - row * OP;
    const int dd = sh_dst[row];
    if (dd >= 0) {
      const long src = (b0 + row) * OP + c, dst = (p.d_row0 + dd) * OP + c;
      p.d.obs[dst] = p.c.obs[src];
      p.d.nobs[dst] = p.c.nobs[src];
    }
  }
  for (int e = tid; e < rows * AP; e += 256) {
    const int row = e / AP, c = e - row * AP;
    const int dd = sh_dst[row];
    if (dd >= 0) p.d.act[(p.d_row0 + dd) * AP + c] = p.c.act[(b0 + row) * AP + c];
  }
  if (d >= 0) { p.d.rew[p.d_row0 + d] = (float)p.rtg[i]; p.d.term[p.d_row0 + d] = p.c.term[i]; }
}

// normalize_obs (buffer.py:88-94): per-column mean / population std in double, then in-place scaling
__global__ void k_colstats(const float* x, long n, int pitch, int dim, double* sums /*[2*dim]*/) {
  __shared__ double sh[2][256];
  const int c = blockIdx.y;
  double s = 0.0, q = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const double v = x[i * pitch + c];
    s += v; q += v * v;
  }
  sh[0][threadIdx.x] = s; sh[1][threadIdx.x] = q;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { sh[0][threadIdx.x] += sh[0][threadIdx.x + o]; sh[1][threadIdx.x] += sh[1][threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { atomicAdd(&sums[c], sh[0][0]); atomicAdd(&sums[dim + c], sh[1][0]); }
}
__global__ void k_normalize(float* x, float* y, long n, int pitch, int dim, const float* mean, const float* stdv) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long i = t / dim; const int c = (int)(t - i * dim);
  if (i >= n) return;
  x[i * pitch + c] = (x[i * pitch + c] - mean[c]) / stdv[c];
  y[i * pitch + c] = (y[i * pitch + c] - mean[c]) / stdv[c];
}
// max |x| of a dataset array (buffer_absmax)
__global__ void k_absmax(const float* x, long n, unsigned int* out_bits) {
  float m = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float a = fabsf(x[i]);
    m = (a > m || a != a) ? a : m;                                            // a NaN sticks
  }
  atomicMax(out_bits, __float_as_uint(m));                                    // non-negative floats (and NaNs above them) order like their bit patterns
}

// ------------------------------------------------------------------------------------------------
// host side: the column set
// ------------------------------------------------------------------------------------------------
int term_refusal(const std::string& who, int term_kind, int od, const char* what) {
  if (term_kind < 0 || term_kind >= ORL_TERM_KINDS) return fail(who + ": unknown termination kind");
  const int need = term_kind == ORL_TERM_PEN ? 27 : ((term_kind == ORL_TERM_HOPPER || term_kind == ORL_TERM_WALKER2D) ? 2 : 1);
  if (od >= need) return 0;
  char msg[256];
  snprintf(msg, sizeof(msg), "%s: termination kind %d reads observation column %d, the %s has %d columns", who.c_str(), term_kind, need - 1, what, od);
  return fail(msg);
}

template <class T>
static int alloc_zeroed(T** p, size_t n) {
  ORL_HIP(hipMalloc((void**)p, sizeof(T) * n));
  ORL_HIP(hipMemset(*p, 0, sizeof(T) * n));
  return 0;
}
void Rows::free_cols() {
  for (const Col& k : cols()) if (*k.p) { hipFree(*k.p); *k.p = nullptr; }
}
int Rows::alloc_rows(long n) {
  free_cols();
  for (const Col& k : cols()) if (alloc_zeroed(k.p, (size_t)n * k.pitch)) return -1;
  return 0;
}
// n rows between a padded and a packed array (either direction): one 2-D copy, a flat one where the row has no padding
static int copy_rows(float* dst, int dst_pitch, const float* src, int src_pitch, int dim, long n, hipMemcpyKind kind) {
  if (dst_pitch == dim && src_pitch == dim) ORL_HIP(hipMemcpy(dst, src, sizeof(float) * n * dim, kind));
  else ORL_HIP(hipMemcpy2D(dst, sizeof(float) * dst_pitch, src, sizeof(float) * src_pitch, sizeof(float) * dim, n, kind));
  return 0;
}
int Rows::copy_in(long row0, const float* const src[5], long n, hipMemcpyKind kind) {
  int k = 0;
  for (const Col& c : cols())
    if (copy_rows(*c.p + row0 * c.pitch, c.pitch, src[k++], c.dim, c.dim, n, kind)) return -1;
  return 0;
}
int Rows::copy_out(long row0, float* const dst[5], long n) {
  int k = 0;
  for (const Col& c : cols())
    if (float* d = dst[k++]; d && copy_rows(d, c.dim, *c.p + row0 * c.pitch, c.pitch, c.dim, n, hipMemcpyDeviceToHost)) return -1;
  return 0;
}

Buffer::~Buffer() {
  hipSetDevice(dev);
  free_cols();
  if (idx) hipFree(idx);
  if (d_n) hipFree(d_n);
  if (runs_scratch) hipFree(runs_scratch);
}
Traj::~Traj() {
  hipSetDevice(dev);
  free_cols();
  for (void* p : {(void*)tidx, (void*)acc, (void*)rtg, (void*)returns, (void*)live_idx[0], (void*)live_idx[1], (void*)live_acc[0],
                  (void*)live_acc[1], (void*)blk_cnt, (void*)blk_rew, (void*)cells, (void*)rew_total})
    if (p) hipFree(p);
}

// diffusion.hip: the dataset rows a DiffusionBC gathers (device, dims, pitches, size, the obs / act arrays)
void buffer_view(const orl_buffer* b, int* dev, int* od, int* ad, int* OP, int* AP, long* n, const float** obs, const float** act) {
  *dev = b->b.dev; *od = b->b.od; *ad = b->b.ad; *OP = b->b.OP; *AP = b->b.AP; *n = b->b.n; *obs = b->b.obs; *act = b->b.act;
}

int buffer_gather(Buffer& b, const long long* idx_dev, int batch, uint64_t seed, float* obs_out, float* act_out, float* next_obs_out,
                  float* rew_out, float* term_out, hipStream_t stream) {
  GatherP g;
  memset(&g, 0, sizeof(g));
  g.src = b; g.n = b.n;
  g.B = batch; g.W = std::max(b.od, b.ad);
  g.idx = idx_dev; g.idx_rs = batch;
  g.b_obs = obs_out; g.b_nobs = next_obs_out; g.b_act = act_out; g.b_rew = rew_out; g.b_term = term_out;
  g.d_op = b.od; g.d_ap = b.ad;
  g.seed = seed; g.gstep = nullptr; g.counter = b.counter++;
  hipLaunchKernelGGL(k_gather, dim3((unsigned)(((long)batch * g.W + 255) / 256), 1), dim3(256), 0, stream, g);
  ORL_HIP(hipGetLastError());
  return 0;
}

int buffer_absmax(Buffer& b, bool reward, float* out) {
  const int w = reward ? 1 : 0;
  if (b.absmax_gen[w] != b.gen) {
    ORL_HIP(hipSetDevice(b.dev));
    unsigned int* d = nullptr;
    if (alloc_zeroed(&d, 1)) return -1;
    if (reward) hipLaunchKernelGGL(k_absmax, dim3(512), dim3(256), 0, 0, (const float*)b.rew, b.n, d);
    else {
      hipLaunchKernelGGL(k_absmax, dim3(1024), dim3(256), 0, 0, (const float*)b.obs, b.n * b.OP, d);
      hipLaunchKernelGGL(k_absmax, dim3(1024), dim3(256), 0, 0, (const float*)b.nobs, b.n * b.OP, d);
      hipLaunchKernelGGL(k_absmax, dim3(512), dim3(256), 0, 0, (const float*)b.act, b.n * b.AP, d);
    }
    unsigned int bits = 0;
    ORL_HIP(hipMemcpy(&bits, d, sizeof(bits), hipMemcpyDeviceToHost));
    hipFree(d);
    memcpy(&b.absmax[w], &bits, sizeof(float));
    b.absmax_gen[w] = b.gen;
  }
  *out = b.absmax[w];
  return 0;
}

// n rows were appended: the ring's host-side pointer and size move on, the cached ranges are stale
static void ring_advance(Buffer& b, long n) {
  b.ptr = (b.ptr + n) % b.cap;
  b.n = std::min(b.n + n, b.cap);
  b.absmax_gen[0] = b.absmax_gen[1] = ~0ull;
}
static int ring_publish(Buffer& b) {
  const long long nn = b.n;
  ORL_HIP(hipMemcpy(b.d_n, &nn, sizeof(nn), hipMemcpyHostToDevice));
  ORL_HIP(hipDeviceSynchronize());        // the appended rows and the new size are visible to every stream of the process
  return 0;
}

// One rollout step of n_runs rings.  `one`: the single-ring entry point -- its messages carry no "run r", and the ring travels in the
// launch parameters instead of an uploaded table.  Per call: the two launches, one read of the results, one device synchronise.
static int append_rollout(const char* F, bool one, orl_buffer* const* rings, int n_runs, int term_kind, const float* obs, const float* act,
                          const float* next_obs, const float* rew, long row_stride, const int64_t* n, float* alive_next_obs,
                          int64_t* n_alive, double* rew_sum) {
  const std::string f(F);
  char msg[224];
  if (term_refusal(f, term_kind, INT_MAX, "buffer")) return -1;      // (the kind alone: that text names no run)
  if (alive_next_obs == next_obs) return fail(f + ": alive_next_obs must not overlap next_obs");
  long nmax = 0;
  for (int r = 0; r < n_runs; ++r) {
    const std::string w = one ? f : f + ": run " + std::to_string(r);
    if (!rings[r]) return fail(w + ": null ring");
    const Buffer &b = rings[r]->b, &b0 = rings[0]->b;
    for (int q = 0; q < r; ++q)
      if (rings[q] == rings[r]) return fail(w + ": the ring of run " + std::to_string(q) + " again (one ring per run)");
    if (b.cap < 1) return fail(w + ": not a ring (orl_buffer_reserve first)");
    if (b.od != b0.od || b.ad != b0.ad || b.dev != b0.dev) {
      snprintf(msg, sizeof(msg), "%s: dims / device (%d, %d, device %d) differ from run 0's (%d, %d, device %d)", w.c_str(), b.od, b.ad, b.dev,
               b0.od, b0.ad, b0.dev);
      return fail(msg);
    }
    if (n[r] < 0 || n[r] > row_stride) {
      snprintf(msg, sizeof(msg), "%s: %lld rows do not fit the row stride %lld", w.c_str(), (long long)n[r], (long long)row_stride);
      return fail(msg);
    }
    if (n[r] > b.cap) return fail(w + ": more rows than the ring's capacity");
    if (term_refusal(w, term_kind, b.od, "buffer")) return -1;
    nmax = std::max(nmax, (long)n[r]);
  }
  Buffer& b0 = rings[0]->b;
  ORL_HIP(hipSetDevice(b0.dev));
  const long R = n_runs, blocks = std::max(1L, (nmax + 255) / 256);
  if (R > b0.runs_scratch_runs || blocks > b0.runs_scratch_blocks) {
    const long cr = std::max(R, b0.runs_scratch_runs), cb = std::max(blocks, b0.runs_scratch_blocks);
    if (b0.runs_scratch) hipFree(b0.runs_scratch);
    b0.runs_scratch = nullptr; b0.runs_scratch_runs = 0; b0.runs_scratch_blocks = 0;
    ORL_HIP(hipMalloc(&b0.runs_scratch, cr * (sizeof(RollRing) + 16) + cr * cb * 12));
    b0.runs_scratch_runs = cr; b0.runs_scratch_blocks = cb;
  }
  // (every piece is a multiple of 8 bytes long except the last)
  RollRing* tab = (RollRing*)b0.runs_scratch;
  long long* out_n = (long long*)(tab + b0.runs_scratch_runs);
  double* out_rew = (double*)(out_n + R);
  double* blk_rew = (double*)(out_n + 2 * b0.runs_scratch_runs);
  int* blk_alive = (int*)(blk_rew + b0.runs_scratch_runs * b0.runs_scratch_blocks);
  std::vector<RollRing> host(R);
  for (int r = 0; r < n_runs; ++r) {
    const Buffer& b = rings[r]->b;
    host[r] = RollRing{b, b.cap, b.ptr, (long)n[r], b.d_n, std::min(b.n + (long)n[r], b.cap)};
  }
  RollP p;
  memset(&p, 0, sizeof(p));
  p.kind = term_kind; p.obs = obs; p.act = act; p.nobs = next_obs; p.rew = rew; p.row_stride = row_stride;
  if (one) p.ring = host[0];
  else {
    ORL_HIP(hipMemcpy(tab, host.data(), sizeof(RollRing) * R, hipMemcpyHostToDevice));
    p.tab = tab;
  }
  p.alive_nobs = alive_next_obs; p.blk_alive = blk_alive; p.blk_rew = blk_rew; p.n_alive_out = out_n; p.rew_sum_out = out_rew;
  hipLaunchKernelGGL(k_roll_term, dim3((unsigned)blocks, (unsigned)R), dim3(256), 0, 0, p);
  hipLaunchKernelGGL(k_roll_scatter, dim3((unsigned)blocks, (unsigned)R), dim3(256), 0, 0, p);
  ORL_HIP(hipGetLastError());
  std::vector<long long> res(2 * R);          // [R] alive counts, then [R] reward sums (doubles): one read for both
  ORL_HIP(hipMemcpy(res.data(), out_n, sizeof(long long) * 2 * R, hipMemcpyDeviceToHost));
  for (int r = 0; r < n_runs; ++r) {
    n_alive[r] = res[r];
    memcpy(&rew_sum[r], &res[R + r], sizeof(double));
    ring_advance(rings[r]->b, n[r]);            // (the kernel published the same size to the ring's device cell)
  }
  ORL_HIP(hipDeviceSynchronize());            // the appended rows and the new sizes are visible to every stream of the process
  return 0;
}

static TrajP traj_params(Traj& t) {
  TrajP p;
  memset(&p, 0, sizeof(p));
  p.c = t; p.tidx = t.tidx; p.acc = t.acc; p.rtg = t.rtg;
  p.returns = t.returns; p.n_traj = t.n_traj;
  p.live_idx = t.live_idx[t.half]; p.live_acc = t.live_acc[t.half]; p.next_idx = t.live_idx[t.half ^ 1]; p.next_acc = t.live_acc[t.half ^ 1];
  p.blk_cnt = t.blk_cnt; p.blk_rew = t.blk_rew; p.cells = t.cells; p.rew_total = t.rew_total;
  p.cap = t.cap; p.half = t.half;
  return p;
}

// the two launches of a step on `stream`; COUNTED: p.n is the bound that sizes the grid
template <bool COUNTED>
static int traj_step_launches(const TrajP& p, hipStream_t stream) {
  const unsigned blocks = (unsigned)((p.n + 255) / 256);
  DEV_LAUNCH(stream, k_traj_term<COUNTED>, dim3(blocks), dim3(256), 0, p);
  DEV_LAUNCH(stream, k_traj_scatter<COUNTED>, dim3(blocks), dim3(256), 0, p);
  return 0;
}
// what a step refuses whoever counts its rows
static int traj_step_refusal(const Traj& t, const std::string& who, int term_kind, const float* next_obs, const float* alive_next_obs, long n) {
  if (t.rows_bound + n > t.cap) {
    char msg[224];
    snprintf(msg, sizeof(msg), "%s: %lld rows + %lld more than the store's capacity %lld", who.c_str(), (long long)t.rows_bound, (long long)n,
             (long long)t.cap);
    return fail(msg);
  }
  if (term_refusal(who, term_kind, t.od, "buffer")) return -1;
  if (alive_next_obs == next_obs) return fail(who + ": alive_next_obs must not overlap next_obs");
  return 0;
}
// the host's rows / live after counted steps: one read of the cells once the device has drained.  -1 also when a counted step overflowed
static int traj_refresh(Traj& t, const char* who) {
  if (!t.stale) return 0;
  ORL_HIP(hipDeviceSynchronize());
  long long c[TRAJ_CELLS];
  ORL_HIP(hipMemcpy(c, t.cells, sizeof(c), hipMemcpyDeviceToHost));
  t.live = (long)c[CELL_LIVE + t.half]; t.rows = t.rows_bound = (long)c[CELL_ROWS + t.half];
  t.stale = false;
  if (c[CELL_OVERFLOW])
    return fail(std::string(who) + ": a counted step found more live trajectories than its bound, or rows beyond the capacity (orl_traj_reset clears)");
  return 0;
}

// orl_traj_append_step_counted on `stream` (declared in devobj.h: the MBRCSL rollout loop places it on the policy engine's stream)
int traj_append_enqueue(orl_traj* h, hipStream_t stream, int term_kind, const float* obs, const float* act, const float* next_obs,
                        const float* rew, long bound, float* alive_next_obs, const char* who) {
  Traj& t = h->t;
  if (traj_step_refusal(t, who, term_kind, next_obs, alive_next_obs, bound)) return -1;
  TrajP p = traj_params(t);
  p.kind = term_kind; p.s_obs = obs; p.s_act = act; p.s_nobs = next_obs; p.s_rew = rew; p.n = bound; p.alive_nobs = alive_next_obs;
  if (traj_step_launches<true>(p, stream)) return -1;
  // (the host keeps upper bounds until traj_refresh: survivors <= min(live, bound), rows <= the sum of the bounds)
  t.rows_bound += bound; t.live = std::min(t.live, bound); t.half ^= 1; t.finished = false; t.stale = true;
  return 0;
}
int traj_info(orl_traj* h, TrajInfo* o) {
  if (!h || !o) return fail("traj_info: null handle");
  const Traj& t = h->t;
  o->dev = t.dev; o->od = t.od; o->ad = t.ad; o->n_traj_cap = t.n_traj_cap; o->cap = t.cap; o->survivors = t.cells;
  return 0;
}

}  // namespace orl

// =================================================================================================
// C ABI
// =================================================================================================
using namespace orl;

extern "C" {

// ---- replay buffer ----
int orl_buffer_create(int32_t obs_dim, int32_t act_dim, int32_t device, orl_buffer** out) {
  if (!out || obs_dim < 1 || act_dim < 1) return fail("orl_buffer_create: bad arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device available: the replay buffer lives in MI355X HBM");
  if (device < 0 || device >= ndev) return fail("bad device ordinal");
  orl_buffer* h = new orl_buffer();
  h->b.dev = device;
  h->b.set_dims(obs_dim, act_dim);
  *out = h;
  return 0;
}
void orl_buffer_destroy(orl_buffer* h) { delete h; }
int orl_buffer_load(orl_buffer* h, const float* obs, const float* act, const float* next_obs, const float* rew, const float* term, int64_t n) {
  Buffer& b = h->b;
  if (n <= 0) return fail("empty dataset");
  ORL_HIP(hipSetDevice(b.dev));
  const float* src[5] = {obs, act, next_obs, rew, term};
  if (b.alloc_rows(n) || b.copy_in(0, src, n, hipMemcpyHostToDevice)) return -1;
  b.n = n;
  b.cap = 0; b.ptr = 0;  // (a loaded dataset is not a ring)
  if (b.d_n) { const long long nn = n; ORL_HIP(hipMemcpy(b.d_n, &nn, sizeof(nn), hipMemcpyHostToDevice)); }
  b.gen++;               // the arrays moved: engines that captured them re-capture (orl_learn_n)
  return 0;
}

// ---- growable ring ----
int orl_buffer_reserve(orl_buffer* h, int64_t capacity) {
  if (!h || capacity < 1) return fail("orl_buffer_reserve: bad arguments");
  Buffer& b = h->b;
  ORL_HIP(hipSetDevice(b.dev));
  ORL_HIP(hipDeviceSynchronize());
  if (b.alloc_rows(capacity)) return -1;
  if (!b.d_n) ORL_HIP(hipMalloc((void**)&b.d_n, sizeof(long long)));
  b.cap = capacity; b.ptr = 0; b.n = 0;
  b.gen++;
  return ring_publish(b);
}
int orl_buffer_append(orl_buffer* h, const float* obs, const float* act, const float* next_obs, const float* rew, const float* term,
                      int64_t n, int on_device) {
  if (!h || !obs || !act || !next_obs || !rew || !term || n < 1) return fail("orl_buffer_append: bad arguments");
  Buffer& b = h->b;
  if (b.cap < 1) return fail("orl_buffer_append: not a ring (orl_buffer_reserve first)");
  if (n > b.cap) return fail("orl_buffer_append: more rows than the ring's capacity");
  ORL_HIP(hipSetDevice(b.dev));
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  // rows [0, n) of the packed sources -> ring rows (ptr + i) % cap: at most two contiguous pieces
  const long first = std::min((long)n, b.cap - b.ptr);
  const float* src[5] = {obs, act, next_obs, rew, term};
  const float* rest[5] = {obs + first * b.od, act + first * b.ad, next_obs + first * b.od, rew + first, term + first};
  if (b.copy_in(b.ptr, src, first, kind) || (n > first && b.copy_in(0, rest, n - first, kind))) return -1;
  ring_advance(b, n);
  return ring_publish(b);
}
int orl_buffer_append_rollout(orl_buffer* h, int32_t term_kind, const float* obs, const float* act, const float* next_obs, const float* rew,
                              int64_t n, float* alive_next_obs, int64_t* n_alive, double* rew_sum) {
  const char* F = "orl_buffer_append_rollout";
  if (!h || !obs || !act || !next_obs || !rew || !alive_next_obs || !n_alive || !rew_sum || n < 1) return fail(std::string(F) + ": bad arguments");
  return append_rollout(F, true, &h, 1, term_kind, obs, act, next_obs, rew, n, &n, alive_next_obs, n_alive, rew_sum);
}
int orl_buffer_append_rollout_runs(orl_buffer* const* rings, int32_t n_runs, int32_t term_kind, const float* obs, const float* act,
                                   const float* next_obs, const float* rew, int64_t row_stride, const int64_t* n, float* alive_next_obs,
                                   int64_t* n_alive, double* rew_sum) {
  const char* F = "orl_buffer_append_rollout_runs";
  if (!rings || n_runs < 1 || !obs || !act || !next_obs || !rew || !alive_next_obs || !n || !n_alive || !rew_sum || row_stride < 1)
    return fail(std::string(F) + ": bad arguments");
  return append_rollout(F, false, rings, n_runs, term_kind, obs, act, next_obs, rew, row_stride, n, alive_next_obs, n_alive, rew_sum);
}
int orl_buffer_read(orl_buffer* h, int64_t row0, int64_t n, float* obs, float* act, float* next_obs, float* rew, float* term) {
  if (!h || n < 1 || row0 < 0 || !obs || !act || !next_obs || !rew || !term) return fail("orl_buffer_read: bad arguments");
  Buffer& b = h->b;
  const long rows = b.cap > 0 ? b.cap : b.n;
  if (!b.obs || row0 + n > rows) return fail("orl_buffer_read: rows beyond the store");
  ORL_HIP(hipSetDevice(b.dev));
  ORL_HIP(hipDeviceSynchronize());
  float* dst[5] = {obs, act, next_obs, rew, term};
  return b.copy_out(row0, dst, n);
}
int64_t orl_buffer_size(orl_buffer* h) { return h->b.n; }

int orl_buffer_normalize_obs(orl_buffer* h, float eps, float* mean_out, float* std_out) {
  Buffer& b = h->b;
  if (!b.obs || b.n < 1) return fail("normalize_obs: empty buffer");
  ORL_HIP(hipSetDevice(b.dev));
  double* sums = nullptr;
  if (alloc_zeroed(&sums, 2 * (size_t)b.od)) return -1;
  hipLaunchKernelGGL(k_colstats, dim3(128, b.od), dim3(256), 0, 0, (const float*)b.obs, b.n, b.OP, b.od, sums);
  std::vector<double> hs(2 * b.od);
  ORL_HIP(hipMemcpy(hs.data(), sums, sizeof(double) * 2 * b.od, hipMemcpyDeviceToHost));
  hipFree(sums);
  std::vector<float> mean(b.od), sd(b.od);
  for (int c = 0; c < b.od; ++c) {
    const double m = hs[c] / (double)b.n;
    double var = hs[b.od + c] / (double)b.n - m * m;
    if (var < 0) var = 0;
    mean[c] = (float)m;
    sd[c] = (float)sqrt(var) + eps;        // buffer.py:90: std + eps
  }
  float* dm = nullptr;                     // [2][od]: mean, then std
  ORL_HIP(hipMalloc((void**)&dm, sizeof(float) * 2 * b.od));
  const float* ds = dm + b.od;
  ORL_HIP(hipMemcpy(dm, mean.data(), sizeof(float) * b.od, hipMemcpyHostToDevice));
  ORL_HIP(hipMemcpy(dm + b.od, sd.data(), sizeof(float) * b.od, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_normalize, dim3((unsigned)((b.n * b.od + 255) / 256)), dim3(256), 0, 0, b.obs, b.nobs, b.n, b.OP, b.od,
                     (const float*)dm, ds);
  ORL_HIP(hipDeviceSynchronize());
  hipFree(dm);
  b.absmax_gen[0] = ~0ull;                 // the values changed in place (same arrays: captured graphs stay valid, the cached range does not)
  if (mean_out) memcpy(mean_out, mean.data(), sizeof(float) * b.od);
  if (std_out) memcpy(std_out, sd.data(), sizeof(float) * b.od);
  return 0;
}
int orl_buffer_sample(orl_buffer* h, const int64_t* idx, int32_t batch, uint64_t seed, float* obs_out, float* act_out,
                      float* next_obs_out, float* rew_out, float* term_out) {
  Buffer& b = h->b;
  if (!b.obs || b.n < 1) return fail("sample: empty buffer");
  if (batch < 1 || !obs_out || !act_out || !next_obs_out || !rew_out || !term_out) return fail("sample: bad arguments");
  ORL_HIP(hipSetDevice(b.dev));
  if (idx) {
    for (int i = 0; i < batch; ++i) if (idx[i] < 0 || idx[i] >= b.n) return fail("sample index out of range");
    if (b.idx_cap < batch) {
      if (b.idx) hipFree(b.idx);
      ORL_HIP(hipMalloc((void**)&b.idx, sizeof(long long) * batch));
      b.idx_cap = batch;
    }
    ORL_HIP(hipMemcpy(b.idx, idx, sizeof(long long) * batch, hipMemcpyHostToDevice));
  }
  if (buffer_gather(b, idx ? b.idx : nullptr, batch, seed, obs_out, act_out, next_obs_out, rew_out, term_out, 0)) return -1;
  ORL_HIP(hipStreamSynchronize(0));
  return 0;
}

// ---- trajectory store (the RCSL rollout) ----
int orl_traj_create(int32_t obs_dim, int32_t act_dim, int32_t device, int64_t n_traj, int64_t capacity_rows, orl_traj** out) {
  if (!out || obs_dim < 1 || act_dim < 1 || n_traj < 1 || capacity_rows < 1 || n_traj > 0x7fffffffLL || capacity_rows > 0x7fffffffLL)
    return fail("orl_traj_create: bad arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device available: the trajectory store lives in MI355X HBM");
  if (device < 0 || device >= ndev) return fail("bad device ordinal");
  ORL_HIP(hipSetDevice(device));
  orl_traj* h = new orl_traj();
  Traj& t = h->t;
  t.dev = device;
  t.set_dims(obs_dim, act_dim);
  t.n_traj_cap = n_traj; t.cap = capacity_rows;
  const long blocks = (std::max((long)n_traj, (long)capacity_rows) + 255) / 256;
  if (t.alloc_rows(t.cap) || alloc_zeroed(&t.tidx, t.cap) || alloc_zeroed(&t.acc, t.cap) || alloc_zeroed(&t.rtg, t.cap) ||
      alloc_zeroed(&t.returns, n_traj) || alloc_zeroed(&t.live_idx[0], n_traj) || alloc_zeroed(&t.live_idx[1], n_traj) ||
      alloc_zeroed(&t.live_acc[0], n_traj) || alloc_zeroed(&t.live_acc[1], n_traj) || alloc_zeroed(&t.blk_cnt, blocks) ||
      alloc_zeroed(&t.blk_rew, blocks) || alloc_zeroed(&t.cells, TRAJ_CELLS) || alloc_zeroed(&t.rew_total, 1)) {
    delete h;
    *out = nullptr;
    return -1;
  }
  *out = h;
  return orl_traj_reset(h, n_traj);
}
void orl_traj_destroy(orl_traj* h) { delete h; }
int orl_traj_reset(orl_traj* h, int64_t n_traj) {
  if (!h || n_traj < 1) return fail("orl_traj_reset: bad arguments");
  Traj& t = h->t;
  if (n_traj > t.n_traj_cap) {
    char msg[160];
    snprintf(msg, sizeof(msg), "orl_traj_reset: %lld trajectories, the store was created for %lld", (long long)n_traj, (long long)t.n_traj_cap);
    return fail(msg);
  }
  ORL_HIP(hipSetDevice(t.dev));
  t.n_traj = n_traj; t.rows = t.rows_bound = 0; t.live = n_traj; t.half = 1; t.finished = false; t.stale = false;
  TrajP p = traj_params(t);                 // (half = 1: the kernel fills the `next` half, 0, which then becomes the current one)
  hipLaunchKernelGGL(k_traj_reset, dim3((unsigned)((n_traj + 255) / 256)), dim3(256), 0, 0, p);
  ORL_HIP(hipGetLastError());
  t.half = 0;
  return 0;
}
int orl_traj_append_step(orl_traj* h, int32_t term_kind, const float* obs, const float* act, const float* next_obs, const float* rew, int64_t n,
                         float* alive_next_obs, int64_t* n_alive) {
  if (!h || !obs || !act || !next_obs || !rew || !alive_next_obs || !n_alive || n < 1) return fail("orl_traj_append_step: bad arguments");
  Traj& t = h->t;
  char msg[200];
  if (t.stale)
    return fail("orl_traj_append_step: the row counts are on the device after orl_traj_append_step_counted; orl_traj_live or orl_traj_finish "
                "refreshes the host's before a host-counted step");
  if (n != t.live) {
    snprintf(msg, sizeof(msg), "orl_traj_append_step: %lld rows, %lld trajectories are live", (long long)n, (long long)t.live);
    return fail(msg);
  }
  if (traj_step_refusal(t, "orl_traj_append_step", term_kind, next_obs, alive_next_obs, n)) return -1;
  ORL_HIP(hipSetDevice(t.dev));
  TrajP p = traj_params(t);
  p.kind = term_kind; p.s_obs = obs; p.s_act = act; p.s_nobs = next_obs; p.s_rew = rew; p.row0 = t.rows; p.n = n; p.alive_nobs = alive_next_obs;
  if (traj_step_launches<false>(p, 0)) return -1;
  long long na = 0;
  ORL_HIP(hipMemcpy(&na, t.cells, sizeof(na), hipMemcpyDeviceToHost));      // the one read of a step: it sizes the next one
  t.rows += n; t.rows_bound = t.rows; t.live = na; t.half ^= 1; t.finished = false;
  *n_alive = na;
  return 0;
}
int orl_traj_append_step_counted(orl_traj* h, int32_t term_kind, const float* obs, const float* act, const float* next_obs, const float* rew,
                                 int64_t bound, float* alive_next_obs) {
  if (!h || !obs || !act || !next_obs || !rew || !alive_next_obs || bound < 1) return fail("orl_traj_append_step_counted: bad arguments");
  ORL_HIP(hipSetDevice(h->t.dev));
  return traj_append_enqueue(h, 0, term_kind, obs, act, next_obs, rew, (long)bound, alive_next_obs, "orl_traj_append_step_counted");
}
int orl_traj_finish(orl_traj* h, int64_t* rows, double* reward_sum, double* returns_host) {
  if (!h) return fail("orl_traj_finish: bad arguments");
  Traj& t = h->t;
  ORL_HIP(hipSetDevice(t.dev));
  if (traj_refresh(t, "orl_traj_finish")) return -1;
  if (t.rows > 0) {
    TrajP p = traj_params(t);
    p.n = t.rows;
    hipLaunchKernelGGL(k_traj_finish, dim3((unsigned)((t.rows + 255) / 256)), dim3(256), 0, 0, p);
    ORL_HIP(hipGetLastError());
  }
  ORL_HIP(hipDeviceSynchronize());
  t.finished = true;
  if (rows) *rows = t.rows;
  if (reward_sum) ORL_HIP(hipMemcpy(reward_sum, t.rew_total, sizeof(double), hipMemcpyDeviceToHost));
  if (returns_host) ORL_HIP(hipMemcpy(returns_host, t.returns, sizeof(double) * t.n_traj, hipMemcpyDeviceToHost));
  return 0;
}
int64_t orl_traj_live(orl_traj* h, int64_t* out_device) {
  if (!h || !out_device) return fail("orl_traj_live: bad arguments");
  Traj& t = h->t;
  if (hipSetDevice(t.dev) != hipSuccess) return fail("orl_traj_live: hipSetDevice failed");
  if (traj_refresh(t, "orl_traj_live")) return -1;
  if (t.live > 0) {
    hipLaunchKernelGGL(k_traj_live, dim3((unsigned)((t.live + 255) / 256)), dim3(256), 0, 0, t.live_idx[t.half], t.live, (long long*)out_device);
    if (hipGetLastError() != hipSuccess) return fail("orl_traj_live: launch failed");
  }
  return t.live;
}
int orl_traj_read(orl_traj* h, int64_t row0, int64_t n, float* obs, float* act, float* next_obs, float* rew, float* term, int32_t* traj_idx,
                  double* acc_ret, double* rtg) {
  if (!h || n < 0 || row0 < 0) return fail("orl_traj_read: bad arguments");
  Traj& t = h->t;
  if (t.stale) return fail("orl_traj_read: the row counts are on the device after orl_traj_append_step_counted (orl_traj_live or orl_traj_finish first)");
  if (row0 + n > t.rows) return fail("orl_traj_read: rows beyond the store");
  if (rtg && !t.finished) return fail("orl_traj_read: the returns-to-go exist after orl_traj_finish");
  if (n == 0) return 0;
  ORL_HIP(hipSetDevice(t.dev));
  ORL_HIP(hipDeviceSynchronize());
  float* dst[5] = {obs, act, next_obs, rew, term};
  if (t.copy_out(row0, dst, n)) return -1;
  if (traj_idx) ORL_HIP(hipMemcpy(traj_idx, t.tidx + row0, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (acc_ret) ORL_HIP(hipMemcpy(acc_ret, t.acc + row0, sizeof(double) * n, hipMemcpyDeviceToHost));
  if (rtg) ORL_HIP(hipMemcpy(rtg, t.rtg + row0, sizeof(double) * n, hipMemcpyDeviceToHost));
  return 0;
}
int orl_traj_export(orl_traj* h, int use_threshold, double threshold, orl_buffer* dst, int64_t* rows_kept, int64_t* traj_kept) {
  if (!h || !dst) return fail("orl_traj_export: bad arguments");
  Traj& t = h->t;
  Buffer& b = dst->b;
  char msg[224];
  if (!t.finished) return fail("orl_traj_export: the returns-to-go exist after orl_traj_finish");
  if (b.cap < 1) return fail("orl_traj_export: the destination is not a ring (orl_buffer_reserve first)");
  if (b.od != t.od || b.ad != t.ad || b.dev != t.dev) {
    snprintf(msg, sizeof(msg), "orl_traj_export: the ring's dims / device (%d, %d, device %d) differ from the store's (%d, %d, device %d)", b.od, b.ad,
             b.dev, t.od, t.ad, t.dev);
    return fail(msg);
  }
  ORL_HIP(hipSetDevice(t.dev));
  long long res[2] = {0, 0};
  TrajP p = traj_params(t);
  p.n = t.rows; p.use_thr = use_threshold ? 1 : 0; p.thr = threshold;
  const long blocks = (t.rows + 255) / 256;
  if (blocks > 0) {
    hipLaunchKernelGGL(k_traj_count, dim3((unsigned)blocks), dim3(256), 0, 0, p);
    ORL_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_traj_total, dim3(1), dim3(256), 0, 0, p, blocks);
  ORL_HIP(hipGetLastError());
  ORL_HIP(hipMemcpy(res, t.cells + 1, sizeof(res), hipMemcpyDeviceToHost));
  if (res[0] > b.cap - b.n) {               // (an RCSL dataset does not wrap; nothing has been written)
    snprintf(msg, sizeof(msg), "orl_traj_export: %lld rows to keep, the ring has room for %lld (capacity %lld, size %lld)", res[0],
             (long long)(b.cap - b.n), (long long)b.cap, (long long)b.n);
    return fail(msg);
  }
  if (rows_kept) *rows_kept = res[0];
  if (traj_kept) *traj_kept = res[1];
  if (res[0] == 0) return 0;
  p.d = b; p.d_row0 = b.ptr;                // (size < capacity: ptr == size)
  hipLaunchKernelGGL(k_traj_export, dim3((unsigned)blocks), dim3(256), 0, 0, p);
  ORL_HIP(hipGetLastError());
  ring_advance(b, res[0]);
  return ring_publish(b);
}

}  // extern "C"
