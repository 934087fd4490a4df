// retime.hip — the kernels of retiming a recording: the
// recording's own latents z_p resampled along time, token by token, at frame
// positions only the device knows (prefix sums of MAS' durations and of the
// plan below, computed inside the same graph).
//
//   vits_retime_plan  old durations + speed / per-token scale / pins / target
//                     -> new durations, in integers
//   vits_retime_warp  z_p of the recording -> z_p of the retimed take: the
//                     centre-aligned piecewise-linear map of each token's new
//                     frames onto its old ones
//
// All lengths are read on the device; the calls keep no host pointer and can
// be captured.  include/vits_amd.h states the arithmetic.
#include "common.h"

// The header states every product and sum of this file as an fp32 operation
// of its own: no contraction into fma anywhere below (edit.hip's reason).
#pragma clang fp contract(off)

namespace {

constexpr int RT_MAX_TX = 4096;
constexpr int RT_MAX_DUR = 1 << 18;  // the clamp of the _int entry points (misc.hip)
constexpr int RT_MAX_LEN = 1 << 18;  // t_rec, t_y and y_len_old
constexpr int RT_MAX_TARGET = 1 << 24;
constexpr int RT_MAX_STAGES = 8;
constexpr int RW_T = 64;  // frames per workgroup of the warp

struct RtStages {
  int32_t mult[RT_MAX_STAGES];
  int n;
};

__device__ __forceinline__ int rt_clamp_dur(int d) { return min(max(d, 0), RT_MAX_DUR); }

// misc.hip's dp_block_sum / dp_block_excl, restated (those live in misc.hip's
// unnamed namespace).  Every thread of the 256 must call them.
__device__ __forceinline__ long long rt_block_sum(long long v, long long* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const long long r = red[0];
  __syncthreads();  // red is reused
  return r;
}

// exclusive prefix of v over the threads of the workgroup; `all` = the sum
__device__ __forceinline__ long long rt_block_excl(long long v, long long* red, long long& all) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const long long a = tid >= o ? red[tid - o] : 0;
    __syncthreads();
    red[tid] += a;
    __syncthreads();
  }
  const long long ex = tid > 0 ? red[tid - 1] : 0;
  all = red[255];
  __syncthreads();  // red is reused
  return ex;
}

// q of a free token: its old frames times its scale, in 1/256 frames.  The
// product of an integer <= 2^18 and an fp32 has at most 42 significant bits:
// exact in double, and so is the shift by 8.
__device__ __forceinline__ long long rt_weight(int d_old, float tok_scale, float rate) {
  float s = tok_scale * rate;
  s = fminf(fmaxf(s, 0.00390625f), 256.f);  // NaN -> 2^-8
  return llrint((double)d_old * (double)s * 256.0);
}

// ---------------------------------------------------------------------------
// Plan: one workgroup per row, a thread owns `per` consecutive tokens.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void retime_plan_kernel(
    const int32_t* __restrict__ dur_old, int64_t dur_old_bstride,
    const int32_t* __restrict__ x_len, int t_x, const int32_t* __restrict__ y_len_old,
    const int32_t* __restrict__ given, const float* __restrict__ tok_scale,
    const float* __restrict__ rates, const int32_t* __restrict__ target,
    int32_t* __restrict__ dur_new, int32_t* __restrict__ meta, int batch) {
  __shared__ long long red[256];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int nx = x_len ? min(max(x_len[b], 0), t_x) : t_x;
  const int32_t* orow = dur_old + (int64_t)b * dur_old_bstride;
  const int32_t* grow = given ? given + (int64_t)b * t_x : nullptr;
  const float* srow = tok_scale ? tok_scale + (int64_t)b * t_x : nullptr;
  int32_t* drow = dur_new + (int64_t)b * t_x;
  const int per = (t_x + 255) / 256;
  const int x0 = tid * per;
  const int x1 = min(x0 + per, nx);  // this thread's tokens: [x0, x1)
  const long long T = target ? target[b] : 0;
  const bool has_target = T > 0;
  const float rate = has_target ? 1.0f : (rates ? rates[b] : 1.0f);

  // 1) the sum of the old durations, P and this thread's share of Q
  long long sum_old = 0, pinned = 0, q_local = 0;
  for (int x = x0; x < x1; ++x) {
    const int d = rt_clamp_dur(orow[x]);
    const int g = grow ? grow[x] : -1;
    sum_old += d;
    if (g >= 0) pinned += min(g, RT_MAX_DUR);
    else q_local += rt_weight(d, srow ? srow[x] : 1.0f, rate);
  }
  sum_old = rt_block_sum(sum_old, red);
  pinned = rt_block_sum(pinned, red);
  long long q_all = 0;
  const long long q_before = rt_block_excl(q_local, red, q_all);

  // 2) E and whether the row is served (uniform over the workgroup)
  const long long ty = y_len_old[b];
  const long long E = has_target ? T - pinned : (q_all + 128) >> 8;
  const bool bad = sum_old != ty || ty > RT_MAX_LEN || E < 0 || T > RT_MAX_TARGET ||
                   (has_target && q_all == 0 && E != 0);
  const long long qd = q_all > 0 ? q_all : 1;  // (no free frame: every B is 0)

  // 3) the durations
  long long sum = 0;
  long long Q = q_before;
  long long b_prev = bad ? 0 : (Q * E + qd / 2) / qd;  // (a bad row's product may not fit)
  for (int x = x0; x < min(x0 + per, t_x); ++x) {
    int d = 0;
    if (x < nx) {
      const int d_old = rt_clamp_dur(orow[x]);
      const int g = grow ? grow[x] : -1;
      if (bad) {
        d = d_old;
      } else if (g >= 0) {
        d = min(g, RT_MAX_DUR);
      } else {
        Q += rt_weight(d_old, srow ? srow[x] : 1.0f, rate);
        const long long b_x = (Q * E + qd / 2) / qd;
        d = (int)(b_x - b_prev);
        b_prev = b_x;
      }
    }
    drow[x] = d;
    sum += d;
  }
  sum = rt_block_sum(sum, red);
  if (tid == 0) {
    meta[b] = (int32_t)(sum > 0x7FFFFFFFll ? 0x7FFFFFFFll : sum);
    meta[batch + b] = bad ? 1 : 0;
  }
}

// edit.hip's ep_scan, restated: the inclusive scan of one row's clamped
// durations by the whole workgroup; returns the total.  Every thread must
// call it; cum is valid on return.
__device__ __forceinline__ int rt_scan(const int32_t* __restrict__ dur, int nx, int t_x, int* cum,
                                       int* part) {
  const int tid = threadIdx.x;
  const int per = (t_x + 255) / 256;
  const int xb0 = tid * per;
  int local = 0;
  for (int i = 0; i < per; ++i) {
    const int x = xb0 + i;
    if (x < t_x) {
      local += x < nx ? rt_clamp_dur(dur[x]) : 0;
      cum[x] = local;
    }
  }
  part[tid] = local;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  const int base = tid > 0 ? part[tid - 1] : 0;
  for (int i = 0; i < per; ++i) {
    const int x = xb0 + i;
    if (x < t_x) cum[x] += base;
  }
  const int total = part[255];
  __syncthreads();  // part is reused by the next scan
  return total;
}

// ---------------------------------------------------------------------------
// Warp: workgroup = (RW_T frames, row).  A lane = one output frame; the four
// waves of the workgroup take every fourth channel, so consecutive lanes
// write consecutive addresses and read near-consecutive ones (a token's new
// frames map monotonically onto its old ones).  Each thread finds its
// frame's owner and weights once, before its loop over the channels.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void retime_warp_kernel(
    const float* __restrict__ z_rec, int t_rec, const int32_t* __restrict__ dur_old,
    int64_t dur_old_bstride, const int32_t* __restrict__ dur_new, int64_t dur_new_bstride,
    const int32_t* __restrict__ x_len, int t_x, const int32_t* __restrict__ y_len_old,
    float* __restrict__ z, int channels, int t_y, int batch, int32_t* __restrict__ lens,
    int32_t* __restrict__ meta, const RtStages st) {
  __shared__ int cum_old[RT_MAX_TX];
  __shared__ int cum_new[RT_MAX_TX];
  __shared__ int part[256];
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int nx = x_len ? min(max(x_len[b], 0), t_x) : t_x;
  const int32_t* orow = dur_old + (int64_t)b * dur_old_bstride;
  const int32_t* nrow = dur_new + (int64_t)b * dur_new_bstride;
  rt_scan(orow, nx, t_x, cum_old, part);
  const int total = rt_scan(nrow, nx, t_x, cum_new, part);
  const int ty = y_len_old[b];
  const int status = (total > t_y || ty <= 0 || ty > t_rec) ? -1 : 0;
  const int y_new = status == 0 ? total : 0;
  if (blockIdx.x == 0) {
    if (tid < st.n) lens[tid * batch + b] = y_new * st.mult[tid];
    if (tid == 0) {
      meta[b] = total;
      meta[batch + b] = status;
    }
  }
  const int tl = tid & (RW_T - 1);
  const int t = blockIdx.x * RW_T + tl;
  if (t >= t_y) return;  // (no barrier below)
  int j0 = 0, j1 = 0;
  float w = 0.f;
  const bool live = t < y_new;
  if (live) {
    int lo = 0, hi = t_x - 1;  // the owner: the first x with cum_new[x] > t
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cum_new[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int i = lo;
    const int dn = rt_clamp_dur(nrow[i]);  // >= 1: the token owns frame t
    const int dold = rt_clamp_dur(orow[i]);
    const int k = t - (cum_new[i] - dn);
    const int c_old = cum_old[i] - dold;
    const long long num = (long long)(2 * k + 1) * dold - dn;
    const int den = 2 * dn;
    long long qf = num / den;
    if (num % den < 0) --qf;  // floor
    const int r = (int)(num - qf * den);
    const long long p = c_old + qf;
    j0 = (int)min(max(p, 0ll), (long long)ty - 1);
    j1 = (int)min(max(p + 1, 0ll), (long long)ty - 1);
    if (r == 0) j1 = j0;
    w = __fdiv_rn((float)r, (float)den);
  }
  // both frames are loaded unconditionally (j1 is a valid frame, mostly of
  // j0's cache line) so that the loads of several channels are in flight
#pragma unroll 4
  for (int c = tid / RW_T; c < channels; c += 256 / RW_T) {
    const int64_t row = (int64_t)b * channels + c;
    float v = 0.f;
    if (live) {
      const float a = z_rec[row * t_rec + j0];
      const float d = z_rec[row * t_rec + j1] - a;
      const float p = w * d;
      v = j1 != j0 ? a + p : a;
    }
    z[row * t_y + t] = v;
  }
}

}  // namespace

extern "C" int vits_retime_plan(const int32_t* dur_old, int64_t dur_old_bstride,
                                const int32_t* x_len, int t_x, const int32_t* y_len_old,
                                const int32_t* given, const float* tok_scale, const float* rate,
                                const int32_t* target, int32_t* dur_new, int32_t* meta, int batch,
                                void* stream) {
  VITS_CHECK_ARG(dur_old && y_len_old && dur_new && meta && batch > 0 && t_x > 0);
  if (t_x > RT_MAX_TX) return VITS_E_UNSUP;
  VITS_CHECK_SHAPE(dur_old_bstride >= t_x);
  hipLaunchKernelGGL(retime_plan_kernel, dim3(batch), dim3(256), 0, as_stream(stream), dur_old,
                     dur_old_bstride, x_len, t_x, y_len_old, given, tok_scale, rate, target,
                     dur_new, meta, batch);
  return vits_launch_status();
}

extern "C" int vits_retime_warp(const float* z_p_rec, int t_rec, const int32_t* dur_old,
                                int64_t dur_old_bstride, const int32_t* dur_new,
                                int64_t dur_new_bstride, const int32_t* x_len, int t_x,
                                const int32_t* y_len_old, float* z, int batch, int channels,
                                int t_y, int32_t* lens, const int32_t* stage_mult, int n_stage,
                                int32_t* meta, void* stream) {
  VITS_CHECK_ARG(z_p_rec && dur_old && dur_new && y_len_old && z && lens && meta && batch > 0 &&
                 channels > 0 && t_y > 0 && t_rec > 0 && t_x > 0);
  VITS_CHECK_ARG(n_stage >= 1 && n_stage <= RT_MAX_STAGES && (n_stage == 1 || stage_mult));
  VITS_CHECK_ARG(((uintptr_t)z & 3) == 0 && ((uintptr_t)z_p_rec & 3) == 0);
  if (t_x > RT_MAX_TX || t_rec > RT_MAX_LEN || t_y > RT_MAX_LEN) return VITS_E_UNSUP;
  VITS_CHECK_SHAPE(dur_old_bstride >= t_x && dur_new_bstride >= t_x && batch <= 65535);
  RtStages st;
  st.n = n_stage;
  for (int i = 0; i < RT_MAX_STAGES; ++i)
    st.mult[i] = i < n_stage ? (stage_mult ? stage_mult[i] : 1) : 0;
  dim3 grid((t_y + RW_T - 1) / RW_T, batch);
  hipLaunchKernelGGL(retime_warp_kernel, grid, dim3(256), 0, as_stream(stream), z_p_rec, t_rec,
                     dur_old, dur_old_bstride, dur_new, dur_new_bstride, x_len, t_x, y_len_old, z,
                     channels, t_y, batch, lens, meta, st);
  return vits_launch_status();
}
