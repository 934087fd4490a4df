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

// table == nullptr: up == down == 1, out[n] = x[n] (the copy / the epilogue alone)
template <typename XT, typename OT>
__global__ __launch_bounds__(256) void post_resample_kernel(
    const XT* __restrict__ x, int64_t x_bstride, int x_cap, const int32_t* __restrict__ lens,
    int len_scale, int n_host, const float* __restrict__ table, int K, int up, int down,
    int half_len, OT* __restrict__ out, int64_t out_bstride, int out_cap, float volume,
    int32_t* __restrict__ out_lens) {
  const int b = blockIdx.y;
  int64_t n_in = lens ? (int64_t)lens[b] * len_scale : (int64_t)n_host;
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
      for (int k = k_lo; k <= k_hi; ++k) acc = fmaf(post_ld(xr, i0 - k), row[k], acc);
    }
  }
  post_st(out + (int64_t)b * out_bstride, n, acc, volume);
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

}  // namespace

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

extern "C" int vits_pcm16(const void* x, int x_dtype, int64_t x_bstride, int x_cap,
                          const int32_t* lens, int len_scale, int n_host, float volume,
                          int16_t* pcm, int64_t out_bstride, int out_cap, int batch,
                          void* stream) {
  VITS_CHECK_ARG(pcm);
  return post_dispatch(x, x_dtype, x_bstride, x_cap, lens, len_scale, n_host, nullptr, 0, 1, 1, 0,
                       nullptr, pcm, out_bstride, out_cap, volume, nullptr, batch, stream);
}
