// post.hip — device-side PCM output stage: polyphase FIR resampler and the
// volume / clip / int16 epilogue of VITSWrap.speaking (vits_wrap.py:186-197:
// librosa.resample for pitch and sampling rate, then clip(wav * volume *
// 32767) -> int16 and the tail-silence pad).
//
// The resampler is scipy.signal.resample_poly(x, up, down) with its default
// Kaiser-5.0 filter h (2 * half_len + 1 taps, designed on the host) and zero
// extension:
//   out[n] = sum_i x[i] * h[n * down - i * up + half_len],   n < ceil(n_in * up / down)
// One thread per output sample: c = n * down + half_len, phase r = c % up,
// newest input i0 = c / up, taps h[r + k * up] * x[i0 - k] for k = 0, 1, ...
// The host lays the filter out by phase, P[r][k] = h[r + k * up] (rows padded
// with zeros to K taps), so a thread walks one contiguous row.  The inputs of
// a wave are one contiguous window of at most 64 * down / up + K samples and
// P is at most a few hundred KB, so both are served from L1 / L2; there is no
// LDS stage, whose size would depend on the ratio.  Accumulation is one fp32
// FMA chain per sample in ascending k (no atomics): reruns are bit-identical.
//
// Each row has its own length: a host integer, or lens[b] * len_scale read on
// the device (no host sync behind the utterance graph).  Samples of x at or
// past the length count as zero whatever the buffer holds; output past n_out
// is written as zero up to the end of the buffer (the tail silence).  The
// grid covers the static output buffer; blocks past n_out only zero-fill.
#include "common.h"

namespace {

__device__ __forceinline__ float post_ld(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float post_ld(const _Float16* p, int64_t i) { return (float)p[i]; }
__device__ __forceinline__ float post_ld(const __bf16* p, int64_t i) { return (float)p[i]; }

__device__ __forceinline__ void post_st(float* p, int64_t i, float v, float) { p[i] = v; }
// int16(clip(float32(float32(v * volume) * 32767), -32768, 32767)), truncated
// toward zero: the two fp32 roundings of the host expression, in its order
__device__ __forceinline__ void post_st(int16_t* p, int64_t i, float v, float volume) {
  float s = __fmul_rn(__fmul_rn(v, volume), 32767.0f);
  s = fminf(fmaxf(s, -32768.0f), 32767.0f);
  p[i] = (int16_t)(int)s;
}

// The FMA chain of one output sample: taps k_lo .. k_hi of its phase row
// against the inputs xr[i0 - k], ascending k.  The whole-signal kernels and
// the span kernel both call it, so a sample is the same bits in either.
template <typename XT>
__device__ __forceinline__ float post_chain(const XT* __restrict__ xr, int64_t i0,
                                            const float* __restrict__ row, int k_lo, int k_hi) {
  float acc = 0.f;
  for (int k = k_lo; k <= k_hi; ++k) acc = fmaf(post_ld(xr, i0 - k), row[k], acc);
  return acc;
}

// Output sample blockIdx.x * 256 + threadIdx.x of row b = blockIdx.y, whose
// input length is n_in before clamping: the one place the arithmetic of the
// output stage lives (the uniform and the per-row kernel both call it).
// table == nullptr: up == down == 1, out[n] = x[n] (the copy / the epilogue alone)
template <typename XT, typename OT>
__device__ __forceinline__ void post_row_sample(
    const XT* __restrict__ x, int64_t x_bstride, int x_cap, int64_t n_in,
    const float* __restrict__ table, int K, int up, int down, int half_len,
    OT* __restrict__ out, int64_t out_bstride, int out_cap, float volume,
    int32_t* __restrict__ out_lens) {
  const int b = blockIdx.y;
  n_in = min(max(n_in, (int64_t)0), (int64_t)x_cap);
  const int64_t n_out = min((n_in * up + down - 1) / down, (int64_t)out_cap);
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n == 0 && out_lens) out_lens[b] = (int32_t)n_out;
  if (n >= out_cap) return;
  float acc = 0.f;
  if (n < n_out) {
    const XT* xr = x + (int64_t)b * x_bstride;
    if (!table) {
      acc = post_ld(xr, n);
    } else {
      const int64_t c = n * down + half_len;
      const int64_t i0 = c / up;
      const float* row = table + (c - i0 * up) * K;
      // input i0 - k must lie in [0, n_in)
      const int k_lo = (int)max((int64_t)0, i0 - (n_in - 1));
      const int k_hi = (int)min((int64_t)(K - 1), i0);
      acc = post_chain(xr, i0, row, k_lo, k_hi);
    }
  }
  post_st(out + (int64_t)b * out_bstride, n, acc, volume);
}

template <typename XT, typename OT>
__global__ __launch_bounds__(256) void post_resample_kernel(
    const XT* __restrict__ x, int64_t x_bstride, int x_cap, const int32_t* __restrict__ lens,
    int len_scale, int n_host, const float* __restrict__ table, int K, int up, int down,
    int half_len, OT* __restrict__ out, int64_t out_bstride, int out_cap, float volume,
    int32_t* __restrict__ out_lens) {
  const int64_t n_in = lens ? (int64_t)lens[blockIdx.y] * len_scale : (int64_t)n_host;
  post_row_sample(x, x_bstride, x_cap, n_in, table, K, up, down, half_len, out, out_bstride,
                  out_cap, volume, out_lens);
}

// ---------------------------------------------------------------------------
// Span form (streaming): out[j] = output sample out_lo + j of the whole
// signal of n_in samples, computed from a window x that holds its samples
// [x_lo, x_lo + x_len).  The phase and the newest input follow the GLOBAL
// index n = out_lo + j; the chain is post_chain over the same taps as the
// whole-signal kernel, minus the zero taps that pad a phase row to K (their
// inputs may lie outside the window; a zero tap leaves the sum as it is).
// Zero from n_out on.  The host has checked that every input read lies in
// the window.
// ---------------------------------------------------------------------------
template <typename XT, typename OT>
__global__ __launch_bounds__(256) void post_span_kernel(
    const XT* __restrict__ x, int64_t x_lo, int64_t n_in, const float* __restrict__ table, int K,
    int up, int down, int half_len, OT* __restrict__ out, int64_t out_lo, int64_t out_len,
    float volume) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= out_len) return;
  const int64_t n = out_lo + j;
  const int64_t n_out = (n_in * up + down - 1) / down;
  float acc = 0.f;
  if (n < n_out) {
    if (!table) {
      acc = post_ld(x, n - x_lo);
    } else {
      const int64_t c = n * down + half_len;
      const int64_t i0 = c / up;
      const int r = (int)(c - i0 * up);
      const float* row = table + (int64_t)r * K;
      // input i0 - k must lie in [0, n_in), tap r + k * up in [0, 2 * half_len]
      const int k_lo = (int)max((int64_t)0, i0 - (n_in - 1));
      const int k_hi = (int)min((int64_t)((2 * half_len - r) / up), i0);
      acc = post_chain(x, i0 - x_lo, row, k_lo, k_hi);
    }
  }
  post_st(out, j, acc, volume);
}

template <typename XT>
int post_span_launch(const void* x, int64_t x_lo, int64_t n_in, const float* table, int K, int up,
                     int down, int half_len, float* out, int16_t* pcm, int64_t out_lo,
                     int64_t out_len, float volume, hipStream_t s) {
  const dim3 grid((unsigned)((out_len + 255) / 256));
  const XT* xp = reinterpret_cast<const XT*>(x);
  if (pcm)
    hipLaunchKernelGGL((post_span_kernel<XT, int16_t>), grid, dim3(256), 0, s, xp, x_lo, n_in,
                       table, K, up, down, half_len, pcm, out_lo, out_len, volume);
  else
    hipLaunchKernelGGL((post_span_kernel<XT, float>), grid, dim3(256), 0, s, xp, x_lo, n_in, table,
                       K, up, down, half_len, out, out_lo, out_len, volume);
  return vits_launch_status();
}

// ---------------------------------------------------------------------------
// Per-row form: one launch over [batch][x_cap] in which every row has its own
// ratio, filter and volume (a group of requests with different pitch, output
// rate and volume behind one graph replay).  The descriptors travel by value
// in the kernel arguments; row b = blockIdx.y is uniform per workgroup, so
// its descriptor is read with scalar loads and the sample loop is the uniform
// kernel's.  The grid covers the shared out_cap: a row is zero from its own
// n_out on.
// ---------------------------------------------------------------------------
constexpr int PR_MAX_BATCH = 64;
struct PostRows {
  vits_post_row r[PR_MAX_BATCH];
};

template <typename XT, typename OT>
__global__ __launch_bounds__(256) void post_resample_rows_kernel(
    const XT* __restrict__ x, int64_t x_bstride, int x_cap, const int32_t* __restrict__ lens,
    int len_scale, const PostRows rows, OT* __restrict__ out, int64_t out_bstride, int out_cap,
    int32_t* __restrict__ out_lens) {
  const vits_post_row& d = rows.r[blockIdx.y];
  post_row_sample(x, x_bstride, x_cap, (int64_t)lens[blockIdx.y] * len_scale, d.table, d.table_k,
                  d.up, d.down, d.half_len, out, out_bstride, out_cap, d.volume, out_lens);
}

template <typename XT>
int post_rows_launch(const void* x, int64_t x_bstride, int x_cap, const int32_t* lens,
                     int len_scale, const PostRows& rows, float* out, int16_t* pcm,
                     int64_t out_bstride, int out_cap, int32_t* out_lens, int batch,
                     hipStream_t s) {
  const dim3 grid((out_cap + 255) / 256, batch);
  const XT* xp = reinterpret_cast<const XT*>(x);
  if (pcm)
    hipLaunchKernelGGL((post_resample_rows_kernel<XT, int16_t>), grid, dim3(256), 0, s, xp,
                       x_bstride, x_cap, lens, len_scale, rows, pcm, out_bstride, out_cap,
                       out_lens);
  else
    hipLaunchKernelGGL((post_resample_rows_kernel<XT, float>), grid, dim3(256), 0, s, xp,
                       x_bstride, x_cap, lens, len_scale, rows, out, out_bstride, out_cap,
                       out_lens);
  return vits_launch_status();
}

template <typename XT>
int post_launch(const void* x, int64_t x_bstride, int x_cap, const int32_t* lens, int len_scale,
                int n_host, const float* table, int K, int up, int down, int half_len, float* out,
                int16_t* pcm, int64_t out_bstride, int out_cap, float volume, int32_t* out_lens,
                int batch, hipStream_t s) {
  const dim3 grid((out_cap + 255) / 256, batch);
  const XT* xp = reinterpret_cast<const XT*>(x);
  if (pcm)
    hipLaunchKernelGGL((post_resample_kernel<XT, int16_t>), grid, dim3(256), 0, s, xp, x_bstride,
                       x_cap, lens, len_scale, n_host, table, K, up, down, half_len, pcm,
                       out_bstride, out_cap, volume, out_lens);
  else
    hipLaunchKernelGGL((post_resample_kernel<XT, float>), grid, dim3(256), 0, s, xp, x_bstride,
                       x_cap, lens, len_scale, n_host, table, K, up, down, half_len, out,
                       out_bstride, out_cap, volume, out_lens);
  return vits_launch_status();
}

int post_dispatch(const void* x, int x_dtype, int64_t x_bstride, int x_cap, const int32_t* lens,
                  int len_scale, int n_host, const float* table, int K, int up, int down,
                  int half_len, float* out, int16_t* pcm, int64_t out_bstride, int out_cap,
                  float volume, int32_t* out_lens, int batch, void* stream) {
  VITS_CHECK_ARG(x && batch > 0 && x_cap > 0 && out_cap > 0 && up >= 1 && down >= 1);
  VITS_CHECK_ARG((out != nullptr) != (pcm != nullptr));
  VITS_CHECK_ARG(x_dtype == VITS_DT_F32 || x_dtype == VITS_DT_F16 || x_dtype == VITS_DT_BF16);
  VITS_CHECK_SHAPE(batch <= 65535 && x_bstride >= x_cap && out_bstride >= out_cap);
  if (lens) {
    VITS_CHECK_ARG(len_scale >= 1);
  } else {
    // host length: the input and the whole output must fit their buffers
    VITS_CHECK_SHAPE(n_host >= 0 && n_host <= x_cap);
    VITS_CHECK_SHAPE(((int64_t)n_host * up + down - 1) / down <= out_cap);
  }
  if (table) {
    // the phase table must be the one of this ratio: up rows of
    // K = ceil((2 * half_len + 1) / up) taps, half_len = 10 * max(up, down)
    VITS_CHECK_SHAPE(half_len == 10 * (up > down ? up : down));
    VITS_CHECK_SHAPE(K == (2 * half_len + up) / up);
  } else {
    VITS_CHECK_ARG(up == 1 && down == 1);
  }
  const hipStream_t s = as_stream(stream);
  switch (x_dtype) {
    case VITS_DT_F16:
      return post_launch<_Float16>(x, x_bstride, x_cap, lens, len_scale, n_host, table, K, up,
                                   down, half_len, out, pcm, out_bstride, out_cap, volume,
                                   out_lens, batch, s);
    case VITS_DT_BF16:
      return post_launch<__bf16>(x, x_bstride, x_cap, lens, len_scale, n_host, table, K, up, down,
                                 half_len, out, pcm, out_bstride, out_cap, volume, out_lens,
                                 batch, s);
    default:
      return post_launch<float>(x, x_bstride, x_cap, lens, len_scale, n_host, table, K, up, down,
                                half_len, out, pcm, out_bstride, out_cap, volume, out_lens, batch,
                                s);
  }
}

// ---------------------------------------------------------------------------
// Ragged pack behind the last pass: the rows of a batch, each cut at its own
// length and followed by `tail` zeros, back to back in one int16 stream, with
// the int32 row offsets beside it (one device-to-host copy returns a whole
// request).  n_out[b] = y_len[b] * hop through ceil(n * up / down) per pass
// (ops.resample_out_len on reduced ratios); offset[b + 1] = offset[b] +
// n_out[b] + tail for b < *n_rows, offset[b + 1] = offset[b] for the padding
// rows of a batch bucket.  Workgroup = (2048 samples of row b, b): every
// workgroup recomputes the prefix over the rows before its own (batch <= 64
// integer steps, no atomics, no second launch).  Samples past the row's
// buffer (a y_len beyond the bucket: the caller re-runs) read as zero and
// nothing is written at or past stream_cap.
// ---------------------------------------------------------------------------
constexpr int PK_MAX_PASSES = 2;
constexpr int PK_MAX_BATCH = 64;
constexpr int PK_T = 2048;
struct PackPasses {
  int32_t up[PK_MAX_PASSES];
  int32_t down[PK_MAX_PASSES];
  int n;
};

__device__ __forceinline__ int64_t pack_row_len(int32_t frames, int hop, const PackPasses& pp) {
  int64_t n = (int64_t)max(frames, 0) * hop;
  for (int i = 0; i < pp.n; ++i) n = (n * pp.up[i] + pp.down[i] - 1) / pp.down[i];
  return n;
}

__global__ __launch_bounds__(256) void pack_pcm_kernel(
    const int16_t* __restrict__ rows, int64_t bstride, int cap, const int32_t* __restrict__ y_len,
    int hop, const PackPasses pp, int tail, const int32_t* __restrict__ n_rows_p, int batch,
    int32_t* __restrict__ offsets, int16_t* __restrict__ stream, int64_t stream_cap) {
  const int b = blockIdx.y;
  const int n_rows = n_rows_p ? min(max(*n_rows_p, 0), batch) : batch;
  if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) {
    int64_t off = 0;
    offsets[0] = 0;
    for (int r = 0; r < batch; ++r) {
      if (r < n_rows) off += pack_row_len(y_len[r], hop, pp) + tail;
      offsets[r + 1] = (int32_t)min(off, (int64_t)INT32_MAX);
    }
  }
  if (b >= n_rows) return;
  int64_t off = 0;
  for (int r = 0; r < b; ++r) off += pack_row_len(y_len[r], hop, pp) + tail;
  const int64_t n_out = pack_row_len(y_len[b], hop, pp);
  const int16_t* src = rows + (int64_t)b * bstride;
  for (int k = 0; k < PK_T / 256; ++k) {
    const int64_t i = (int64_t)blockIdx.x * PK_T + k * 256 + threadIdx.x;
    if (i >= n_out + tail || off + i >= stream_cap) break;
    stream[off + i] = (i < n_out && i < cap) ? src[i] : (int16_t)0;
  }
}

// Per-row form of the pack: row b has its own pass ratios (always
// PK_MAX_PASSES of them, 1 / 1 where it has fewer) and its own tail.
struct PackRows {
  int32_t up[PK_MAX_BATCH][PK_MAX_PASSES];
  int32_t down[PK_MAX_BATCH][PK_MAX_PASSES];
  int32_t tail[PK_MAX_BATCH];
};

__device__ __forceinline__ int64_t pack_rows_len(int32_t frames, int hop, const PackRows& pr,
                                                 int r) {
  int64_t n = (int64_t)max(frames, 0) * hop;
  for (int i = 0; i < PK_MAX_PASSES; ++i) n = (n * pr.up[r][i] + pr.down[r][i] - 1) / pr.down[r][i];
  return n;
}

__global__ __launch_bounds__(256) void pack_pcm_rows_kernel(
    const int16_t* __restrict__ rows, int64_t bstride, int cap, const int32_t* __restrict__ y_len,
    int hop, const PackRows pr, const int32_t* __restrict__ n_rows_p, int batch,
    int32_t* __restrict__ offsets, int16_t* __restrict__ stream, int64_t stream_cap) {
  const int b = blockIdx.y;
  const int n_rows = n_rows_p ? min(max(*n_rows_p, 0), batch) : batch;
  if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) {
    int64_t off = 0;
    offsets[0] = 0;
    for (int r = 0; r < batch; ++r) {
      if (r < n_rows) off += pack_rows_len(y_len[r], hop, pr, r) + pr.tail[r];
      offsets[r + 1] = (int32_t)min(off, (int64_t)INT32_MAX);
    }
  }
  if (b >= n_rows) return;
  int64_t off = 0;
  for (int r = 0; r < b; ++r) off += pack_rows_len(y_len[r], hop, pr, r) + pr.tail[r];
  const int64_t n_out = pack_rows_len(y_len[b], hop, pr, b);
  const int tail = pr.tail[b];
  const int16_t* src = rows + (int64_t)b * bstride;
  for (int k = 0; k < PK_T / 256; ++k) {
    const int64_t i = (int64_t)blockIdx.x * PK_T + k * 256 + threadIdx.x;
    if (i >= n_out + tail || off + i >= stream_cap) break;
    stream[off + i] = (i < n_out && i < cap) ? src[i] : (int16_t)0;
  }
}

}  // namespace

extern "C" int vits_resample_poly_rows(const void* x, int x_dtype, int64_t x_bstride, int x_cap,
                                       const int32_t* lens, int len_scale,
                                       const vits_post_row* rows, float* out, int16_t* pcm,
                                       int64_t out_bstride, int out_cap, int32_t* out_lens,
                                       int batch, void* stream) {
  VITS_CHECK_ARG(x && lens && rows && batch > 0 && x_cap > 0 && out_cap > 0 && len_scale >= 1);
  VITS_CHECK_ARG((out != nullptr) != (pcm != nullptr));
  VITS_CHECK_ARG(x_dtype == VITS_DT_F32 || x_dtype == VITS_DT_F16 || x_dtype == VITS_DT_BF16);
  VITS_CHECK_SHAPE(batch <= PR_MAX_BATCH && x_bstride >= x_cap && out_bstride >= out_cap);
  PostRows pr;
  for (int b = 0; b < PR_MAX_BATCH; ++b) {
    vits_post_row& d = pr.r[b];
    if (b >= batch) {
      d = vits_post_row{nullptr, 1, 1, 0, 0, 1.0f, 0};
      continue;
    }
    d = rows[b];
    d.reserved = 0;
    VITS_CHECK_ARG(d.up >= 1 && d.down >= 1);
    if (d.up == 1 && d.down == 1) {
      d.table = nullptr;  // scipy returns a copy: no filter
      d.half_len = d.table_k = 0;
    } else {
      // the phase table must be the one of this row's ratio (see post_dispatch)
      VITS_CHECK_ARG(d.table);
      VITS_CHECK_SHAPE(d.half_len == 10 * (d.up > d.down ? d.up : d.down));
      VITS_CHECK_SHAPE(d.table_k == (2 * d.half_len + d.up) / d.up);
    }
  }
  const hipStream_t s = as_stream(stream);
  switch (x_dtype) {
    case VITS_DT_F16:
      return post_rows_launch<_Float16>(x, x_bstride, x_cap, lens, len_scale, pr, out, pcm,
                                        out_bstride, out_cap, out_lens, batch, s);
    case VITS_DT_BF16:
      return post_rows_launch<__bf16>(x, x_bstride, x_cap, lens, len_scale, pr, out, pcm,
                                      out_bstride, out_cap, out_lens, batch, s);
    default:
      return post_rows_launch<float>(x, x_bstride, x_cap, lens, len_scale, pr, out, pcm,
                                     out_bstride, out_cap, out_lens, batch, s);
  }
}

extern "C" int vits_pack_pcm_rows(const int16_t* rows, int64_t bstride, int cap,
                                  const int32_t* y_len, int hop, const int32_t* up,
                                  const int32_t* down, const int32_t* tail, const int32_t* n_rows,
                                  int batch, int32_t* offsets, int16_t* out, int64_t out_cap,
                                  void* stream) {
  VITS_CHECK_ARG(rows && y_len && offsets && out && up && down && tail && batch > 0 && cap > 0 &&
                 hop >= 1 && out_cap > 0);
  VITS_CHECK_SHAPE(batch <= PK_MAX_BATCH && bstride >= cap);
  PackRows pr;
  int tail_max = 0;
  for (int b = 0; b < PK_MAX_BATCH; ++b) {
    for (int i = 0; i < PK_MAX_PASSES; ++i) {
      pr.up[b][i] = b < batch ? up[b * PK_MAX_PASSES + i] : 1;
      pr.down[b][i] = b < batch ? down[b * PK_MAX_PASSES + i] : 1;
      VITS_CHECK_ARG(pr.up[b][i] >= 1 && pr.down[b][i] >= 1);
    }
    pr.tail[b] = b < batch ? tail[b] : 0;
    VITS_CHECK_ARG(pr.tail[b] >= 0);
    tail_max = pr.tail[b] > tail_max ? pr.tail[b] : tail_max;
  }
  const int64_t n_max = (int64_t)cap + tail_max;  // the longest row a buffer row can hold
  VITS_CHECK_SHAPE(n_max <= INT32_MAX);
  const dim3 grid((unsigned)((n_max + PK_T - 1) / PK_T), batch);
  hipLaunchKernelGGL(pack_pcm_rows_kernel, grid, dim3(256), 0, as_stream(stream), rows, bstride,
                     cap, y_len, hop, pr, n_rows, batch, offsets, out, out_cap);
  return vits_launch_status();
}

extern "C" int vits_pack_pcm(const int16_t* rows, int64_t bstride, int cap, const int32_t* y_len,
                             int hop, const int32_t* up, const int32_t* down, int n_passes,
                             int tail, const int32_t* n_rows, int batch, int32_t* offsets,
                             int16_t* out, int64_t out_cap, void* stream) {
  VITS_CHECK_ARG(rows && y_len && offsets && out && batch > 0 && cap > 0 && hop >= 1 &&
                 tail >= 0 && out_cap > 0);
  VITS_CHECK_ARG(n_passes >= 0 && n_passes <= PK_MAX_PASSES && (n_passes == 0 || (up && down)));
  VITS_CHECK_SHAPE(batch <= PK_MAX_BATCH && bstride >= cap);
  PackPasses pp;
  pp.n = n_passes;
  for (int i = 0; i < PK_MAX_PASSES; ++i) {
    pp.up[i] = i < n_passes ? up[i] : 1;
    pp.down[i] = i < n_passes ? down[i] : 1;
    VITS_CHECK_ARG(pp.up[i] >= 1 && pp.down[i] >= 1);
  }
  const int64_t n_max = (int64_t)cap + tail;  // the longest row a buffer row can hold
  VITS_CHECK_SHAPE(n_max <= INT32_MAX);
  const dim3 grid((unsigned)((n_max + PK_T - 1) / PK_T), batch);
  hipLaunchKernelGGL(pack_pcm_kernel, grid, dim3(256), 0, as_stream(stream), rows, bstride, cap,
                     y_len, hop, pp, tail, n_rows, batch, offsets, out, out_cap);
  return vits_launch_status();
}

extern "C" int vits_resample_poly(const void* x, int x_dtype, int64_t x_bstride, int x_cap,
                                  const int32_t* lens, int len_scale, int n_host,
                                  const float* table, int table_rows, int table_k, int up,
                                  int down, int half_len, float* out, int16_t* pcm,
                                  int64_t out_bstride, int out_cap, float volume,
                                  int32_t* out_lens, int batch, void* stream) {
  VITS_CHECK_ARG(up >= 1 && down >= 1);
  if (up == 1 && down == 1) {
    table = nullptr;  // scipy returns a copy: no filter
  } else {
    VITS_CHECK_ARG(table);
    VITS_CHECK_SHAPE(table_rows == up);
  }
  return post_dispatch(x, x_dtype, x_bstride, x_cap, lens, len_scale, n_host, table, table_k, up,
                       down, half_len, out, pcm, out_bstride, out_cap, volume, out_lens, batch,
                       stream);
}

extern "C" int vits_resample_poly_span(const void* x, int x_dtype, int64_t x_lo, int64_t x_len,
                                       int64_t n_in, const float* table, int table_rows,
                                       int table_k, int up, int down, int half_len, float* out,
                                       int16_t* pcm, int64_t out_lo, int64_t out_len, float volume,
                                       void* stream) {
  VITS_CHECK_ARG(up >= 1 && down >= 1);
  VITS_CHECK_ARG(x_lo >= 0 && x_len >= 0 && n_in >= 0 && out_lo >= 0 && out_len >= 0);
  VITS_CHECK_ARG(x || x_len == 0);
  VITS_CHECK_ARG((out != nullptr) != (pcm != nullptr));
  VITS_CHECK_ARG(x_dtype == VITS_DT_F32 || x_dtype == VITS_DT_F16 || x_dtype == VITS_DT_BF16);
  if (up == 1 && down == 1) {
    table = nullptr;  // scipy returns a copy: no filter
    half_len = table_k = 0;
  } else {
    // the phase table must be the one of this ratio (see post_dispatch)
    VITS_CHECK_ARG(table);
    VITS_CHECK_SHAPE(table_rows == up);
    VITS_CHECK_SHAPE(half_len == 10 * (up > down ? up : down));
    VITS_CHECK_SHAPE(table_k == (2 * half_len + up) / up);
  }
  // every index the kernel forms fits int64, and the grid its 32-bit x extent
  VITS_CHECK_SHAPE(x_lo <= INT64_MAX - x_len && out_lo <= INT64_MAX - out_len);
  VITS_CHECK_SHAPE(n_in <= (INT64_MAX - down) / up);
  VITS_CHECK_SHAPE(out_lo + out_len <= (INT64_MAX - half_len) / down);
  VITS_CHECK_SHAPE((out_len + 255) / 256 <= INT32_MAX);
  // the inputs in [0, n_in) under a tap of any requested output below n_out
  // (both ends grow with n: the first output gives the lowest input, the
  // last one the highest); ops.resample_span_input is this arithmetic
  const int64_t n_out = (n_in * up + down - 1) / down;
  const int64_t n_end = out_lo + out_len < n_out ? out_lo + out_len : n_out;
  if (out_lo < n_end) {
    int64_t need_lo = out_lo, need_hi = n_end;
    if (table) {
      const int64_t first = out_lo * down - half_len;
      need_lo = first <= 0 ? 0 : (first + up - 1) / up;
      need_hi = ((n_end - 1) * down + half_len) / up + 1;
      need_hi = need_hi < n_in ? need_hi : n_in;
    }
    if (need_lo < need_hi) VITS_CHECK_SHAPE(x_lo <= need_lo && need_hi <= x_lo + x_len);
  }
  if (out_len == 0) return VITS_OK;
  const hipStream_t s = as_stream(stream);
  switch (x_dtype) {
    case VITS_DT_F16:
      return post_span_launch<_Float16>(x, x_lo, n_in, table, table_k, up, down, half_len, out,
                                        pcm, out_lo, out_len, volume, s);
    case VITS_DT_BF16:
      return post_span_launch<__bf16>(x, x_lo, n_in, table, table_k, up, down, half_len, out, pcm,
                                      out_lo, out_len, volume, s);
    default:
      return post_span_launch<float>(x, x_lo, n_in, table, table_k, up, down, half_len, out, pcm,
                                     out_lo, out_len, volume, s);
  }
}

extern "C" int vits_pcm16(const void* x, int x_dtype, int64_t x_bstride, int x_cap,
                          const int32_t* lens, int len_scale, int n_host, float volume,
                          int16_t* pcm, int64_t out_bstride, int out_cap, int batch,
                          void* stream) {
  VITS_CHECK_ARG(pcm);
  return post_dispatch(x, x_dtype, x_bstride, x_cap, lens, len_scale, n_host, nullptr, 0, 1, 1, 0,
                       nullptr, pcm, out_bstride, out_cap, volume, nullptr, batch, stream);
}
