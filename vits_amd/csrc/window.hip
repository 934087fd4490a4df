// window.hip — the copy of long-recording voice conversion:
// up to 64 ranges of fp32 elements moved in ONE launch, in either direction
// between a whole recording and the overlapping rows of a conversion graph.
//
// Job j, channel r:
//   dst[dst_off_j + r * dst_rstride + i] = src[src_off_j + r * src_rstride + i]   i < len_j
//   dst[dst_off_j + r * dst_rstride + i] = 0                          len_j <= i < fill_len_j
// and nothing else is written.  The three uses: the waveform gather (R = 1:
// the recording into the graph's static wav rows, zero past each row's
// length), the noise gather (R = inter_channels: one [C, F] draw into each
// row's [C, window] slice) and the core scatter (R = 1: each row's core of
// the graph's output into the stitched waveform).
//
// The jobs travel by value in the kernel arguments (2 KB), as the rows of
// vits_resample_poly_rows do: the call keeps no host pointer and can be
// captured.  Workgroup = (tile of 1024 elements, channel, job); job and
// channel are uniform per workgroup, so the descriptor is read with scalar
// loads and the path choice below does not diverge.  Where source and
// destination of a (job, channel) are co-aligned modulo 16 bytes a lane moves
// one aligned float4 (the lanes of the first and the last vector of a range,
// and those across len, go element by element); otherwise every lane moves
// single elements, consecutive lanes consecutive addresses.
#include "common.h"

namespace {

constexpr int CW_MAX_JOBS = 64;
constexpr int CW_TILE = 1024;  // elements per workgroup: 256 lanes x 4
struct CopyJobs {
  vits_window_job j[CW_MAX_JOBS];
};

__global__ __launch_bounds__(256) void copy_windows_kernel(
    const float* __restrict__ src, int64_t src_rstride, float* __restrict__ dst,
    int64_t dst_rstride, const CopyJobs jobs) {
  const vits_window_job& jb = jobs.j[blockIdx.z];
  const int64_t len = jb.len, fill = jb.fill_len;
  const int64_t t0 = (int64_t)blockIdx.x * CW_TILE;
  // (a tile starts up to 3 elements before the range on the aligned path)
  if (t0 >= fill + 3) return;
  const float* s = src + jb.src_off + (int64_t)blockIdx.y * src_rstride;
  float* d = dst + jb.dst_off + (int64_t)blockIdx.y * dst_rstride;
  const int a = (int)(((uintptr_t)d >> 2) & 3);  // elements past a 16-byte boundary
  if (a == (int)(((uintptr_t)s >> 2) & 3)) {
    // element i0 of both sides lies on a 16-byte boundary
    const int64_t i0 = t0 + (int64_t)threadIdx.x * 4 - a;
    if (i0 >= 0 && i0 + 4 <= len) {
      *reinterpret_cast<f32x4*>(d + i0) = *reinterpret_cast<const f32x4*>(s + i0);
    } else if (i0 >= len && i0 + 4 <= fill) {
      *reinterpret_cast<f32x4*>(d + i0) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t i = i0 + k;
        if (i >= 0 && i < fill) d[i] = i < len ? s[i] : 0.f;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i = t0 + k * 256 + threadIdx.x;
      if (i < fill) d[i] = i < len ? s[i] : 0.f;
    }
  }
}

}  // namespace

extern "C" int vits_copy_windows(const float* src, int64_t src_numel, int64_t src_rstride,
                                 float* dst, int64_t dst_numel, int64_t dst_rstride,
                                 const vits_window_job* jobs, int n_jobs, int channels,
                                 void* stream) {
  VITS_CHECK_ARG(src && dst && jobs && n_jobs >= 1 && channels >= 1);
  VITS_CHECK_ARG(src_numel >= 0 && dst_numel >= 0 && src_rstride >= 0 && dst_rstride >= 0);
  VITS_CHECK_ARG(((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0);
  VITS_CHECK_SHAPE(n_jobs <= CW_MAX_JOBS && channels <= 65535);
  // every element a job reads or writes lies inside its buffer (no overflow:
  // the products are bounded before they are formed)
  const int64_t last = channels - 1;
  auto fits = [last](int64_t off, int64_t n, int64_t rstride, int64_t numel) {
    if (n > numel || (last && rstride > (numel - n) / last)) return false;
    return off <= numel - n - last * rstride;
  };
  CopyJobs cj;
  int64_t fill_max = 0;
  for (int j = 0; j < CW_MAX_JOBS; ++j) {
    if (j >= n_jobs) {
      cj.j[j] = vits_window_job{0, 0, 0, 0};
      continue;
    }
    const vits_window_job& jb = jobs[j];
    VITS_CHECK_ARG(jb.len >= 0 && jb.fill_len >= jb.len && jb.src_off >= 0 && jb.dst_off >= 0);
    VITS_CHECK_SHAPE(fits(jb.src_off, jb.len, src_rstride, src_numel));
    VITS_CHECK_SHAPE(fits(jb.dst_off, jb.fill_len, dst_rstride, dst_numel));
    // the channels of a job do not write over each other
    VITS_CHECK_SHAPE(channels == 1 || dst_rstride >= jb.fill_len);
    cj.j[j] = jb;
    fill_max = jb.fill_len > fill_max ? jb.fill_len : fill_max;
  }
  if (fill_max == 0) return VITS_OK;  // nothing to write
  const int64_t tiles = (fill_max + 3 + CW_TILE - 1) / CW_TILE;
  VITS_CHECK_SHAPE(tiles <= INT32_MAX);
  hipLaunchKernelGGL(copy_windows_kernel, dim3((unsigned)tiles, channels, n_jobs), dim3(256), 0,
                     as_stream(stream), src, src_rstride, dst, dst_rstride, cj);
  return vits_launch_status();
}
