// edit.hip — the kernels of speech editing: a span of a
// recording's tokens re-spoken with new text, spliced in latent space at
// frame positions only the device knows (prefix sums of MAS' and the
// duration plan's durations, computed inside the same graph).
//
//   vits_edit_pins    old durations + span -> the pins and the target of the
//                     duration plan over the new text
//   vits_edit_splice  the prior expansion of the new span and the recording's
//                     own z_p on both sides of it, in one pass
//   vits_edit_patch   the waveform side: the recording outside the edit, the
//                     synthesis inside, a cross-fade at each seam
//
// All lengths are read on the device; the calls keep no host pointer and can
// be captured.  include/vits_amd.h states the arithmetic.
#include "common.h"

// The header states every product and sum of this file as an fp32 operation
// of its own: no contraction into fma anywhere below (the __f*_rn forms alone
// do not prevent it: they are plain operators to the compiler).
#pragma clang fp contract(off)

namespace {

constexpr int EP_MAX_TX = 4096;
constexpr int EP_MAX_DUR = 1 << 18;  // the clamp of the _int entry points (misc.hip)
constexpr int EP_MAX_STAGES = 8;
constexpr int ES_T = 64;             // frames per workgroup of the splice
constexpr int EPA_T = 1024;          // samples per workgroup of the patch

struct EpStages {
  int32_t mult[EP_MAX_STAGES];
  int n;
};

// The inclusive scan of one row's clamped durations by a whole 256-thread
// workgroup (misc.hip's ed_scan_tokens / ed_scan_given, restated: that one
// lives in misc.hip's unnamed namespace): cum[x] = sum_{x' <= x} d(x') with
// d(x) = min(max(dur[x], 0), 2^18) for x < nx and 0 for nx <= x < t_x;
// returns the total.  Every thread must call it; cum is valid on return.
__device__ __forceinline__ int ep_scan(const int32_t* __restrict__ dur, int nx, int t_x, int* cum,
                                       int* part) {
  const int tid = threadIdx.x;
  const int per = (t_x + 255) / 256;
  const int xb0 = tid * per;
  int local = 0;
  for (int i = 0; i < per; ++i) {
    const int x = xb0 + i;
    if (x < t_x) {
      local += x < nx ? min(max(dur[x], 0), EP_MAX_DUR) : 0;
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
  __syncthreads();
  return part[255];
}

// ---------------------------------------------------------------------------
// Pins: one workgroup per row.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void edit_pins_kernel(
    const int32_t* __restrict__ dur_old, int64_t dur_old_bstride,
    const int32_t* __restrict__ x_len_old, int t_x_old, const int32_t* __restrict__ x_len_new,
    int t_x_new, const int32_t* __restrict__ spans, const int32_t* __restrict__ span_given,
    const int32_t* __restrict__ span_target, const int32_t* __restrict__ y_len_old,
    int32_t* __restrict__ given, int32_t* __restrict__ target, int32_t* __restrict__ meta,
    int batch) {
  __shared__ int cum[EP_MAX_TX];
  __shared__ int part[256];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int nxo = x_len_old ? x_len_old[b] : t_x_old;
  const int nxn = x_len_new ? x_len_new[b] : t_x_new;
  const int a = spans[b * 3], bo = spans[b * 3 + 1], bn = spans[b * 3 + 2];
  const int32_t* drow = dur_old + (int64_t)b * dur_old_bstride;
  const int total = ep_scan(drow, min(max(nxo, 0), t_x_old), t_x_old, cum, part);
  const int ty = y_len_old[b];
  bool ok = nxo >= 0 && nxo <= t_x_old && nxn >= 0 && nxn <= t_x_new;
  ok = ok && a >= 0 && a <= bo && bo <= nxo && a <= bn && bn <= nxn && nxo - bo == nxn - bn;
  ok = ok && !(nxo > 0 && total == 0) && total == ty;
  const int f0 = ok && a > 0 ? cum[a - 1] : 0;
  const int f1 = ok && bo > 0 ? cum[bo - 1] : 0;
  int32_t* grow = given + (int64_t)b * t_x_new;
  const int32_t* srow = span_given ? span_given + (int64_t)b * t_x_new : nullptr;
  for (int t = tid; t < t_x_new; t += 256) {
    int g = 0;
    if (ok) {
      if (t < a) {
        g = min(max(drow[t], 0), EP_MAX_DUR);
      } else if (t < bn) {
        g = srow ? srow[t] : -1;
      } else if (t < nxn) {
        g = min(max(drow[t - bn + bo], 0), EP_MAX_DUR);
      } else {
        g = -1;  // (past the row's tokens: the plan does not read it)
      }
    }
    grow[t] = g;
  }
  if (tid == 0) {
    int tg = 0;
    const int st = span_target ? span_target[b] : 0;
    if (ok && st > 0) tg = ty - (f1 - f0) + st;
    if (ok && st < 0) tg = ty;
    target[b] = tg;
    meta[b] = f0;
    meta[batch + b] = f1;
    meta[2 * batch + b] = ok ? 0 : 1;
  }
}

// ---------------------------------------------------------------------------
// Splice: workgroup = (ES_T frames, row).  The geometry of a row comes from
// the scan of dur_new alone: the pins make the prefix and the suffix of
// dur_new those of the old durations, so
//   f0 = cum[a - 1], n_new = cum[b_new - 1] - f0, suffix = total - cum[b_new - 1],
//   f1 = y_len_old - suffix, y_new = total.
// Each group of four frames [4k, 4k + 4) is either moved as one 16-byte
// vector (wholly kept or wholly past y_new, source and destination
// co-aligned: a lane = one group of one channel, 16 channels per pass) or its
// frames go one by one (a lane = one frame of one channel, 4 channels per
// pass, consecutive lanes consecutive addresses): the new span, the groups
// across a boundary and a suffix whose shift is no multiple of four.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void edit_splice_kernel(
    const int32_t* __restrict__ dur_new, int64_t dur_bstride,
    const int32_t* __restrict__ x_len_new, int t_x, const int32_t* __restrict__ spans,
    const int32_t* __restrict__ y_len_old, const float* __restrict__ m,
    const float* __restrict__ s, int64_t ms_bstride, int ms_cstride,
    const float* __restrict__ noise, const float* __restrict__ z_rec, int t_rec,
    float* __restrict__ z, int channels, int t_y, int batch, int32_t* __restrict__ lens,
    int32_t* __restrict__ meta, const EpStages st, int z_aligned, int rec_aligned) {
  __shared__ int cum[EP_MAX_TX];
  __shared__ int part[256];
  __shared__ int src[ES_T];   // kept frame: its frame of the recording; new: its token
  __shared__ int kind[ES_T];  // 0 zero, 1 kept, 2 new
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int nx = x_len_new ? min(max(x_len_new[b], 0), t_x) : t_x;
  const int total = ep_scan(dur_new + (int64_t)b * dur_bstride, nx, t_x, cum, part);
  const int a = spans[b * 3], bo = spans[b * 3 + 1], bn = spans[b * 3 + 2];
  const int ty = y_len_old[b];
  int f0 = 0, n_new = 0, f1 = 0, status = 1;
  if (a >= 0 && a <= bn && bn <= nx && bo >= a && ty >= 0 && ty <= t_rec) {
    f0 = a > 0 ? cum[a - 1] : 0;
    const int e1 = bn > 0 ? cum[bn - 1] : 0;
    n_new = e1 - f0;
    f1 = ty - (total - e1);
    status = f1 >= f0 ? (total > t_y ? -1 : 0) : 1;
  }
  if (status == 1) f0 = n_new = f1 = 0;
  const int y_new = status == 0 ? total : 0;
  if (blockIdx.x == 0) {
    if (tid < st.n) lens[tid * batch + b] = y_new * st.mult[tid];
    if (tid == 0) {
      meta[b] = f0;
      meta[batch + b] = n_new;
      meta[2 * batch + b] = f1;
      meta[3 * batch + b] = status;
    }
  }
  const int e0 = f0 + n_new;             // first frame of the kept suffix
  const int shift = n_new - (f1 - f0);   // suffix frame t reads the recording at t - shift
  const int t0 = blockIdx.x * ES_T;
  if (tid < ES_T) {
    const int t = t0 + tid;
    int k = 0, r = 0;
    if (t < y_new) {
      if (t < f0) {
        k = 1, r = t;
      } else if (t >= e0) {
        k = 1, r = t - shift;
      } else {
        int lo = 0, hi = t_x - 1;  // first x with cum[x] > t
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (cum[mid] > t) hi = mid; else lo = mid + 1;
        }
        k = 2, r = lo;
      }
    }
    kind[tid] = k;
    src[tid] = r;
  }
  __syncthreads();
  // which groups of four go as vectors (the same for every channel)
  // (z_aligned / rec_aligned: the buffer starts on a 16-byte boundary)
  const bool dst_al = z_aligned && (t_y & 3) == 0;
  const bool pre_al = dst_al && rec_aligned && (t_rec & 3) == 0;
  const bool suf_al = pre_al && (shift & 3) == 0;
  auto group_mode = [&](int g) {  // 0: frame by frame, 1: vector copy, 2: vector zero
    const int t = t0 + g * 4;
    if (t + 4 > t_y) return 0;
    if (t >= y_new) return dst_al ? 2 : 0;
    if (t + 4 <= f0) return pre_al ? 1 : 0;
    if (t >= e0 && t + 4 <= y_new) return suf_al ? 1 : 0;
    return 0;
  };
  const float* mb = m + (int64_t)b * ms_bstride;
  const float* sb = s + (int64_t)b * ms_bstride;
  {
    const int g = tid & 15;
    const int mode = group_mode(g);
    if (mode) {
      const int t = t0 + g * 4;
      const int r = src[g * 4];
      for (int c = tid >> 4; c < channels; c += 16) {
        const int64_t row = (int64_t)b * channels + c;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (mode == 1) v = *reinterpret_cast<const f32x4*>(z_rec + row * t_rec + r);
        *reinterpret_cast<f32x4*>(z + row * t_y + t) = v;
      }
    }
  }
  {
    const int tl = tid & (ES_T - 1);
    const int t = t0 + tl;
    if (t < t_y && group_mode(tl >> 2) == 0) {
      const int k = kind[tl], r = src[tl];
      for (int c = tid / ES_T; c < channels; c += 256 / ES_T) {
        const int64_t row = (int64_t)b * channels + c;
        float v = 0.f;
        if (k == 1) {
          v = z_rec[row * t_rec + r];
        } else if (k == 2) {
          // vits_expand_durations_int's m + (noise * s) * 1.0: a rounded
          // product, then a rounded sum (no contraction into an fma)
          const float n = noise[row * t_y + t];
          const float p = n * sb[(int64_t)c * ms_cstride + r];
          v = mb[(int64_t)c * ms_cstride + r] + p;
        }
        z[row * t_y + t] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Patch: workgroup = (EPA_T samples, row), a lane = consecutive samples.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void edit_patch_kernel(
    const float* __restrict__ orig, int64_t orig_bstride, int orig_cap,
    const float* __restrict__ o, int64_t o_bstride, int o_cap,
    const int32_t* __restrict__ y_len_old, const int32_t* __restrict__ smeta, int hop, int margin,
    int fade, float* __restrict__ out, int64_t out_bstride, int out_cap,
    int32_t* __restrict__ out_len, int batch) {
  const int b = blockIdx.y;
  const int64_t ty = y_len_old[b];
  const int64_t f0 = smeta[b], n_new = smeta[batch + b], f1 = smeta[2 * batch + b];
  const int64_t y_new = f0 + n_new + ty - f1;
  int64_t L = y_new * hop;
  const bool ok = smeta[3 * batch + b] == 0 && ty >= 0 && f0 >= 0 && n_new >= 0 && f1 >= f0 &&
                  f1 <= ty && ty * hop <= orig_cap && L <= o_cap && L <= out_cap;
  if (!ok) L = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) out_len[b] = (int32_t)L;
  int64_t lo = (f0 - margin > 0 ? f0 - margin : 0) * hop;
  int64_t hi = (f0 + n_new + margin < y_new ? f0 + n_new + margin : y_new) * hop;
  const int64_t shift = (y_new - ty) * hop;
  // a fade that does not fit is dropped and the synthesis runs to that end
  const bool fade_in = fade > 0 && lo - fade >= 0;
  const bool fade_out = fade > 0 && hi + fade <= L;
  if (fade > 0 && !fade_in) lo = 0;
  if (fade > 0 && !fade_out) hi = L;
  const float* ob = o + (int64_t)b * o_bstride;
  const float* gb = orig + (int64_t)b * orig_bstride;
  float* yb = out + (int64_t)b * out_bstride;
  const float fl = (float)fade;
#pragma unroll
  for (int k = 0; k < EPA_T / 256; ++k) {
    const int64_t i = (int64_t)blockIdx.x * EPA_T + k * 256 + threadIdx.x;
    if (i >= out_cap) break;
    float v = 0.f;
    if (i < L) {
      if (i >= lo && i < hi) {
        v = ob[i];
      } else if (i < lo) {
        v = gb[i];
        if (fade_in && i >= lo - fade) {
          const float w = ((float)(i - (lo - fade)) + 0.5f) / fl;
          v = v * (1.0f - w) + ob[i] * w;
        }
      } else {
        v = gb[i - shift];
        if (fade_out && i < hi + fade) {
          const float w = ((float)(hi + fade - 1 - i) + 0.5f) / fl;
          v = v * (1.0f - w) + ob[i] * w;
        }
      }
    }
    yb[i] = v;
  }
}

}  // namespace

extern "C" int vits_edit_pins(const int32_t* dur_old, int64_t dur_old_bstride,
                              const int32_t* x_len_old, int t_x_old, const int32_t* x_len_new,
                              int t_x_new, const int32_t* spans, const int32_t* span_given,
                              const int32_t* span_target, const int32_t* y_len_old,
                              int32_t* given, int32_t* target, int32_t* meta, int batch,
                              void* stream) {
  VITS_CHECK_ARG(dur_old && x_len_old && x_len_new && spans && y_len_old && given && target &&
                 meta && batch > 0 && t_x_old > 0 && t_x_new > 0);
  if (t_x_old > EP_MAX_TX || t_x_new > EP_MAX_TX) return VITS_E_UNSUP;
  VITS_CHECK_SHAPE(dur_old_bstride >= t_x_old);
  hipLaunchKernelGGL(edit_pins_kernel, dim3(batch), dim3(256), 0, as_stream(stream), dur_old,
                     dur_old_bstride, x_len_old, t_x_old, x_len_new, t_x_new, spans, span_given,
                     span_target, y_len_old, given, target, meta, batch);
  return vits_launch_status();
}

extern "C" int vits_edit_splice(const int32_t* dur_new, int64_t dur_bstride,
                                const int32_t* x_len_new, int t_x, const int32_t* spans,
                                const int32_t* y_len_old, const float* m, const float* s,
                                int64_t ms_bstride, int32_t ms_cstride, const float* noise,
                                const float* z_p_rec, int t_rec, float* z, int batch, int channels,
                                int t_y, int32_t* lens, const int32_t* stage_mult, int n_stage,
                                int32_t* meta, void* stream) {
  VITS_CHECK_ARG(dur_new && spans && y_len_old && m && s && noise && z_p_rec && z && lens && meta &&
                 batch > 0 && channels > 0 && t_y > 0 && t_rec > 0 && t_x > 0);
  VITS_CHECK_ARG(n_stage >= 1 && n_stage <= EP_MAX_STAGES && (n_stage == 1 || stage_mult));
  if (t_x > EP_MAX_TX) return VITS_E_UNSUP;
  VITS_CHECK_SHAPE(dur_bstride >= t_x && ms_cstride >= t_x && ms_bstride >= 0 && batch <= 65535);
  VITS_CHECK_ARG(((uintptr_t)z & 3) == 0 && ((uintptr_t)z_p_rec & 3) == 0);
  EpStages st;
  st.n = n_stage;
  for (int i = 0; i < EP_MAX_STAGES; ++i)
    st.mult[i] = i < n_stage ? (stage_mult ? stage_mult[i] : 1) : 0;
  const int z_aligned = ((uintptr_t)z & 15) == 0, rec_aligned = ((uintptr_t)z_p_rec & 15) == 0;
  dim3 grid((t_y + ES_T - 1) / ES_T, batch);
  hipLaunchKernelGGL(edit_splice_kernel, grid, dim3(256), 0, as_stream(stream), dur_new,
                     dur_bstride, x_len_new, t_x, spans, y_len_old, m, s, ms_bstride, ms_cstride,
                     noise, z_p_rec, t_rec, z, channels, t_y, batch, lens, meta, st, z_aligned,
                     rec_aligned);
  return vits_launch_status();
}

extern "C" int vits_edit_patch(const float* orig, int64_t orig_bstride, int orig_cap,
                               const float* o, int64_t o_bstride, int o_cap,
                               const int32_t* y_len_old, const int32_t* splice_meta, int hop,
                               int margin, int fade, float* out, int64_t out_bstride, int out_cap,
                               int32_t* out_len, int batch, void* stream) {
  VITS_CHECK_ARG(orig && o && y_len_old && splice_meta && out && out_len && batch > 0 &&
                 orig_cap > 0 && o_cap > 0 && out_cap > 0 && hop > 0 && margin >= 0 && fade >= 0);
  VITS_CHECK_SHAPE(orig_bstride >= orig_cap && o_bstride >= o_cap && out_bstride >= out_cap &&
                   batch <= 65535);
  dim3 grid((out_cap + EPA_T - 1) / EPA_T, batch);
  hipLaunchKernelGGL(edit_patch_kernel, grid, dim3(256), 0, as_stream(stream), orig, orig_bstride,
                     orig_cap, o, o_bstride, o_cap, y_len_old, splice_meta, hop, margin, fade, out,
                     out_bstride, out_cap, out_len, batch);
  return vits_launch_status();
}
