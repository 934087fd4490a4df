// attention.hip — scaled-dot-product attention of attentions.MultiHeadAttention
// (attentions.py:85-100) on gfx950 fp32 MFMA, flash-style (online softmax).
//
// q/k/v arrive channel-major [B][H*D][T] straight from the 1x1 projection
// convs (attentions.py:79-81), so no transpose is ever materialised:
//   S^T[key][query] = K[key][:] . Q[query][:]       (v_mfma_f32_32x32x2_f32)
// with the key on the accumulator ROW and the query on the lane: the softmax
// over keys is then an in-register reduction plus one xor-32 shuffle per
// query, and the accumulator registers are directly the B operand of
//   O^T[d][query] += V^T[d][key] . P^T[key][query]
// (k-step r of that product takes key (r&3)+8(r>>2)+4*(lane>>5), which is
// exactly the row register r holds in each half-wave).
//
// One wave = one (utterance, head, 32-query tile).  Mask semantics follow
// attentions.py:94-95: scores.masked_fill(mask == 0, -1e4) with
// mask = x_mask[q] * x_mask[k]; keys beyond T (tile padding) are excluded
// (-inf), so a fully-masked query row averages all T keys exactly like the
// reference softmax over the padded row.
#include "common.h"

namespace {

constexpr int AT_Q = 32;
constexpr int AT_K = 32;

template <int D>
__global__ __launch_bounds__(64) void attn_fwd_kernel(const float* __restrict__ q,
                                                      const float* __restrict__ k,
                                                      const float* __restrict__ v,
                                                      float* __restrict__ out, int H, int T,
                                                      int64_t bstride, int64_t out_bstride,
                                                      const int32_t* __restrict__ lengths) {
  static_assert(D % 16 == 0, "head dim multiple of 16");
  constexpr int KS = D / 2;          // k-steps of the QK product
  constexpr int DT = (D + 31) / 32;  // d tiles of the PV product (last one partial for D%32)
  const int lane = threadIdx.x;
  const int l32 = lane & 31;
  const int lhi = lane >> 5;
  const int q0 = blockIdx.x * AT_Q;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int len = lengths ? lengths[b] : T;
  const int64_t hoff = (int64_t)b * bstride + (int64_t)h * D * T;
  const float* qb = q + hoff;
  const float* kb = k + hoff;
  const float* vb = v + hoff;
  const float scale_div = sqrtf((float)D);

  // Q^T fragment (B operand): lane holds Q[query q0+l32][d = 2s + lhi] / sqrt(D)
  const int qi = q0 + l32;
  const bool qvalid = qi < T;
  float qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = qvalid ? qb[(int64_t)(2 * s + lhi) * T + qi] / scale_div : 0.f;
  const bool qmasked = qi >= len;

  f32x16 o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float m_run = -INFINITY;
  float l_run = 0.f;

  for (int k0 = 0; k0 < T; k0 += AT_K) {
    // S^T tile: rows = keys k0 + row, cols = queries
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    const int kr = k0 + l32;  // A operand row (key) of this lane
    const bool kvalid = kr < T;
#pragma unroll
    for (int st = 0; st < KS; ++st) {
      const float a = kvalid ? kb[(int64_t)(2 * st + lhi) * T + kr] : 0.f;
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(a, qf[st], s, 0, 0, 0);
    }
    // mask + online softmax over the key rows of this lane's query column
    float mloc = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      float sv = s[r];
      if (key >= T)
        sv = -INFINITY;
      else if (qmasked || key >= len)
        sv = -1e4f;
      s[r] = sv;
      mloc = fmaxf(mloc, sv);
    }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    const float m_new = fmaxf(m_run, mloc);
    const float alpha = (m_run == -INFINITY) ? 0.f : expf(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = (s[r] == -INFINITY) ? 0.f : expf(s[r] - m_new);
      s[r] = p;
      psum += p;
    }
    psum += __shfl_xor(psum, 32, 64);
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
    // O^T[d][query] += V^T[d][key] P^T[key][query]
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const bool dvalid = (D % 32 == 0) || (t * 32 + l32 < D);
      const float* vr = vb + (int64_t)(t * 32 + l32) * T + k0 + 4 * lhi;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = (r & 3) + 8 * (r >> 2);
        const float a = (dvalid && k0 + kk + 4 * lhi < T) ? vr[kk] : 0.f;
        o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, s[r], o[t], 0, 0, 0);
      }
    }
  }
  // epilogue: O^T rows = d, cols = query (this lane)
  if (!qvalid) return;
  const float inv = 1.0f / l_run;
  float* ob = out + (int64_t)b * out_bstride + (int64_t)h * D * T;
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      if (D % 32 == 0 || d < D) ob[(int64_t)d * T + qi] = o[t][r] * inv;
    }
}

}  // namespace

extern "C" int vits_attention_forward(const float* q, const float* k, const float* v, float* out,
                                      int batch, int heads, int head_dim, int t_len,
                                      int64_t bstride, int64_t out_bstride,
                                      const int32_t* lengths, void* stream) {
  VITS_CHECK_ARG(q && k && v && out && batch > 0 && heads > 0 && t_len > 0);
  VITS_CHECK_SHAPE(bstride >= (int64_t)heads * head_dim * t_len);
  VITS_CHECK_SHAPE(out_bstride >= (int64_t)heads * head_dim * t_len);
  dim3 grid((t_len + AT_Q - 1) / AT_Q, heads, batch);
  hipStream_t s = as_stream(stream);
  switch (head_dim) {
#define VITS_ATTN_CASE(D)                                                                      \
    case D:                                                                                    \
      hipLaunchKernelGGL(attn_fwd_kernel<D>, grid, dim3(64), 0, s, q, k, v, out, heads, t_len, \
                         bstride, out_bstride, lengths);                                       \
      break;
    VITS_ATTN_CASE(16)
    VITS_ATTN_CASE(32)
    VITS_ATTN_CASE(48)
#undef VITS_ATTN_CASE
    case 64:
      hipLaunchKernelGGL(attn_fwd_kernel<64>, grid, dim3(64), 0, s, q, k, v, out, heads, t_len,
                         bstride, out_bstride, lengths);
      break;
    case 128:
      hipLaunchKernelGGL(attn_fwd_kernel<128>, grid, dim3(64), 0, s, q, k, v, out, heads, t_len,
                         bstride, out_bstride, lengths);
      break;
    case 96:
      hipLaunchKernelGGL(attn_fwd_kernel<96>, grid, dim3(64), 0, s, q, k, v, out, heads, t_len,
                         bstride, out_bstride, lengths);
      break;
    default:
      return VITS_E_UNSUP;
  }
  return vits_launch_status();
}

// ===========================================================================
// Training: the same attention with a saved log-sum-exp, dropout of the
// normalised probabilities (attentions.py:97) and its backward.
//
// I/O type: fp32 (v_mfma_f32_32x32x2_f32, the arithmetic of the kernel above)
// or fp16 / bf16 (v_mfma_f32_32x32x16_{f16,bf16}; fp32 accumulation, fp32
// softmax; operands rounded where torch's autocast rounds them: q/sqrt(D), P
// after dropout, dS).  All products go through at_mma: a lane supplies its A
// row's / B column's value for "slot" n of its lane half, and the caller
// decides which k index a (slot, half) pair is - any bijection works as long
// as both operands use the same one, which is what lets an accumulator tile
// (row (r&3)+8(r>>2)+4*half in register r) be the next product's operand in
// either instruction with no lane movement.
//
// Backward (no atomics, fixed reduction order -> bit-reproducible):
//   dq kernel     one wave per (b, h, 32-query tile), loops over key tiles,
//                 S^T / dP^T with the key on the accumulator row exactly like
//                 the forward, dQ^T[d][q] += K^T[d][key] dS^T[key][q]; also
//                 writes delta[q] = sum_d dO O.
//   dk/dv kernel  one wave per (b, h, 32-key tile, 32-wide d tile), loops over
//                 query tiles
//                 with the QUERY on the accumulator row (S = Q K^T), so that
//                 dV^T[d][key] += dO^T[d][q] Pd[q][key] and
//                 dK^T[d][key] += Q^T[d][q] dS[q][key] sum over the row index.
//   P = exp(S - lse), Pd = P keep/(1-p), dS = P (keep/(1-p) (dO.V) - delta),
//   dS = 0 where the score was filled with -1e4 (masked_fill passes no
//   gradient) - those entries still carry P into dV.
// ===========================================================================
namespace {

template <int DT> struct at_io;
template <> struct at_io<VITS_DT_F32> { typedef float T; };
template <> struct at_io<VITS_DT_F16> { typedef _Float16 T; };
template <> struct at_io<VITS_DT_BF16> { typedef __bf16 T; };

struct at_args {
  const void* q;
  const void* k;
  const void* v;
  const void* o;     // forward output (read by the backward)
  const void* dout;
  void* out;         // forward: output
  void* dq;
  void* dk;
  void* dv;
  float* lse;        // written by the forward, read by the backward
  float* delta;      // written by the dq kernel, read by the dk/dv kernel
  int H, T;
  int64_t bs_qkv, bs_out, bs_dout, bs_dqkv;
  const int32_t* lengths;
  const int64_t* seed;  // device scalar; read only when thr != 0
  uint32_t thr;         // drop when hash < thr (p * 2^32); 0 = no dropout
  float inv_keep;       // 1 / (1 - p)
};

__device__ __forceinline__ uint64_t at_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the dropout draw of (seed, b, h, query, key): splitmix64 finaliser over the
// element's linear index keyed with the mixed seed (sm = at_mix64(seed));
// shared by the forward, both backward kernels and the mask kernel
__device__ __forceinline__ bool at_keep(uint64_t sm, int bh, int T, int qi, int key,
                                        uint32_t thr) {
  const uint64_t idx = ((uint64_t)bh * (uint64_t)T + (uint64_t)qi) * (uint64_t)T + (uint64_t)key;
  const uint64_t z = at_mix64(sm ^ ((idx + 1) * 0x9E3779B97F4A7C15ull));
  return (uint32_t)(z >> 32) >= thr;
}

// accumulator register r of lane half h holds tile row at_row(r, h)
__device__ __forceinline__ int at_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// acc[32][32] += A[32][2 NS] B[2 NS][32]; fa(n) / fb(n): this lane's A row /
// B column at the k index the caller assigns to slot n of this lane half
template <int DT, int NS, class FA, class FB>
__device__ __forceinline__ void at_mma(f32x16& acc, FA fa, FB fb) {
  // every operand is fetched before the first MFMA: one memory latency per
  // product instead of one per k-step
  if constexpr (DT == VITS_DT_F32) {
    float a[NS], b[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      a[n] = fa(n);
      b[n] = fb(n);
    }
#pragma unroll
    for (int n = 0; n < NS; ++n) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[n], b[n], acc, 0, 0, 0);
  } else {
    static_assert(NS % 8 == 0, "16 k per 16-bit MFMA");
    typedef typename at_io<DT>::T T;
    typedef T T8 __attribute__((ext_vector_type(8)));
    T8 a[NS / 8], b[NS / 8];
#pragma unroll
    for (int s = 0; s < NS / 8; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a[s][j] = (T)fa(8 * s + j);
        b[s][j] = (T)fb(8 * s + j);
      }
#pragma unroll
    for (int s = 0; s < NS / 8; ++s) {
      if constexpr (DT == VITS_DT_F16)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], b[s], acc, 0, 0, 0);
      else
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], b[s], acc, 0, 0, 0);
    }
  }
}

template <int D, int DT>
__global__ __launch_bounds__(64) void attn_train_fwd_kernel(const at_args a) {
  typedef typename at_io<DT>::T T_;
  static_assert(D % 16 == 0, "head dim multiple of 16");
  constexpr int KS = D / 2;
  constexpr int DTL = (D + 31) / 32;
  const int T = a.T;
  const int lane = threadIdx.x;
  const int l32 = lane & 31;
  const int lhi = lane >> 5;
  const int q0 = blockIdx.x * AT_Q;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int bh = b * a.H + h;
  const int len = a.lengths ? a.lengths[b] : T;
  const int64_t hoff = (int64_t)b * a.bs_qkv + (int64_t)h * D * T;
  const T_* qb = static_cast<const T_*>(a.q) + hoff;
  const T_* kb = static_cast<const T_*>(a.k) + hoff;
  const T_* vb = static_cast<const T_*>(a.v) + hoff;
  const float scale_div = sqrtf((float)D);
  const bool drop = a.thr != 0;
  const uint64_t sm = drop ? at_mix64((uint64_t)*a.seed) : 0;

  const int qi = q0 + l32;
  const bool qvalid = qi < T;
  float qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s)
    qf[s] = qvalid ? (float)qb[(int64_t)(2 * s + lhi) * T + qi] / scale_div : 0.f;
  const bool qmasked = qi >= len;

  f32x16 o[DTL];
#pragma unroll
  for (int t = 0; t < DTL; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float m_run = -INFINITY;
  float l_run = 0.f;

  for (int k0 = 0; k0 < T; k0 += AT_K) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    const int kr = k0 + l32;
    const bool kvalid = kr < T;
    at_mma<DT, KS>(
        s, [&](int n) { return kvalid ? (float)kb[(uint32_t)((2 * n + lhi) * T + kr)] : 0.f; },
        [&](int n) { return qf[n]; });
    float mloc = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + at_row(r, lhi);
      float sv = s[r];
      if (key >= T)
        sv = -INFINITY;
      else if (qmasked || key >= len)
        sv = -1e4f;
      s[r] = sv;
      mloc = fmaxf(mloc, sv);
    }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    const float m_new = fmaxf(m_run, mloc);
    const float alpha = (m_run == -INFINITY) ? 0.f : expf(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = (s[r] == -INFINITY) ? 0.f : expf(s[r] - m_new);
      s[r] = p;
      psum += p;
    }
    psum += __shfl_xor(psum, 32, 64);
    l_run = l_run * alpha + psum;
    m_run = m_new;
    if (drop) {  // the normaliser keeps the undropped sum
#pragma unroll
      for (int r = 0; r < 16; ++r)
        s[r] = at_keep(sm, bh, T, qi, k0 + at_row(r, lhi), a.thr) ? s[r] * a.inv_keep : 0.f;
    }
#pragma unroll
    for (int t = 0; t < DTL; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
#pragma unroll
    for (int t = 0; t < DTL; ++t) {
      const bool dvalid = (D % 32 == 0) || (t * 32 + l32 < D);
      const T_* vr = vb + (int64_t)(t * 32 + l32) * T + k0 + 4 * lhi;
      at_mma<DT, 16>(
          o[t],
          [&](int r) {
            const int kk = (r & 3) + 8 * (r >> 2);
            return (dvalid && k0 + kk + 4 * lhi < T) ? (float)vr[kk] : 0.f;
          },
          [&](int r) { return s[r]; });
    }
  }
  if (!qvalid) return;
  const float inv = 1.0f / l_run;
  T_* ob = static_cast<T_*>(a.out) + (int64_t)b * a.bs_out + (int64_t)h * D * T;
#pragma unroll
  for (int t = 0; t < DTL; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = t * 32 + at_row(r, lhi);
      if (D % 32 == 0 || d < D) ob[(int64_t)d * T + qi] = (T_)(o[t][r] * inv);
    }
  if (lhi == 0) a.lse[(int64_t)bh * T + qi] = m_run + logf(l_run);
}

template <int D, int DT>
__global__ __launch_bounds__(64) void attn_bwd_dq_kernel(const at_args a) {
  typedef typename at_io<DT>::T T_;
  constexpr int KS = D / 2;
  constexpr int DTL = (D + 31) / 32;
  const int T = a.T;
  const int lane = threadIdx.x;
  const int l32 = lane & 31;
  const int lhi = lane >> 5;
  const int q0 = blockIdx.x * AT_Q;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int bh = b * a.H + h;
  const int len = a.lengths ? a.lengths[b] : T;
  const int64_t hoff = (int64_t)b * a.bs_qkv + (int64_t)h * D * T;
  const T_* qb = static_cast<const T_*>(a.q) + hoff;
  const T_* kb = static_cast<const T_*>(a.k) + hoff;
  const T_* vb = static_cast<const T_*>(a.v) + hoff;
  const T_* ob = static_cast<const T_*>(a.o) + (int64_t)b * a.bs_out + (int64_t)h * D * T;
  const T_* dob = static_cast<const T_*>(a.dout) + (int64_t)b * a.bs_dout + (int64_t)h * D * T;
  const float scale_div = sqrtf((float)D);
  const bool drop = a.thr != 0;
  const uint64_t sm = drop ? at_mix64((uint64_t)*a.seed) : 0;

  const int qi = q0 + l32;
  const bool qvalid = qi < T;
  const bool qmasked = qi >= len;
  // B-operand fragments of this lane's query: Q / sqrt(D) and dO at d = 2n + lhi
  float qf[KS], dof[KS];
  float delta = 0.f;
#pragma unroll
  for (int n = 0; n < KS; ++n) {
    const int64_t at = (int64_t)(2 * n + lhi) * T + qi;
    qf[n] = qvalid ? (float)qb[at] / scale_div : 0.f;
    dof[n] = qvalid ? (float)dob[at] : 0.f;
    delta += qvalid ? dof[n] * (float)ob[at] : 0.f;
  }
  delta += __shfl_xor(delta, 32, 64);
  const float lse = qvalid ? a.lse[(int64_t)bh * T + qi] : 0.f;
  if (qvalid && lhi == 0) a.delta[(int64_t)bh * T + qi] = delta;

  f32x16 dq[DTL];
#pragma unroll
  for (int t = 0; t < DTL; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[t][r] = 0.f;

  for (int k0 = 0; k0 < T; k0 += AT_K) {
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
    const int kr = k0 + l32;
    const bool kvalid = kr < T;
    // S^T[key][q] = K Q^T / sqrt(D), dP^T[key][q] = V dO^T
    at_mma<DT, KS>(
        s, [&](int n) { return kvalid ? (float)kb[(uint32_t)((2 * n + lhi) * T + kr)] : 0.f; },
        [&](int n) { return qf[n]; });
    at_mma<DT, KS>(
        dp, [&](int n) { return kvalid ? (float)vb[(uint32_t)((2 * n + lhi) * T + kr)] : 0.f; },
        [&](int n) { return dof[n]; });
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + at_row(r, lhi);
      const bool filled = qmasked || key >= len;
      const float sv = filled ? -1e4f : s[r];
      const float p = (qvalid && key < T) ? expf(sv - lse) : 0.f;
      float g = dp[r];
      if (drop) g = at_keep(sm, bh, T, qi, key, a.thr) ? g * a.inv_keep : 0.f;
      s[r] = filled ? 0.f : p * (g - delta);
    }
    // dQ^T[d][q] += K^T[d][key] dS^T[key][q]
#pragma unroll
    for (int t = 0; t < DTL; ++t) {
      const bool dvalid = (D % 32 == 0) || (t * 32 + l32 < D);
      const T_* kr_ = kb + (int64_t)(t * 32 + l32) * T;
      at_mma<DT, 16>(
          dq[t],
          [&](int r) {
            const int key = k0 + at_row(r, lhi);
            return (dvalid && key < T) ? (float)kr_[key] : 0.f;
          },
          [&](int r) { return s[r]; });
    }
  }
  if (!qvalid) return;
  T_* dqb = static_cast<T_*>(a.dq) + (int64_t)b * a.bs_dqkv + (int64_t)h * D * T;
#pragma unroll
  for (int t = 0; t < DTL; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = t * 32 + at_row(r, lhi);
      if (D % 32 == 0 || d < D) dqb[(int64_t)d * T + qi] = (T_)(dq[t][r] / scale_div);
    }
}

template <int D, int DT>
__global__ __launch_bounds__(64) void attn_bwd_dkv_kernel(const at_args a) {
  typedef typename at_io<DT>::T T_;
  constexpr int KS = D / 2;
  constexpr int DTL = (D + 31) / 32;
  const int T = a.T;
  const int lane = threadIdx.x;
  const int l32 = lane & 31;
  const int lhi = lane >> 5;
  // grid.x = key tile x d tile: one 32-wide d tile of dK / dV per wave (S and
  // dP are recomputed per d tile: the grids are far smaller than the chip,
  // and 2 accumulator tiles instead of 2 DTL keep the wave out of scratch)
  const int t = blockIdx.x % DTL;
  const int k0 = (blockIdx.x / DTL) * AT_K;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int bh = b * a.H + h;
  const int len = a.lengths ? a.lengths[b] : T;
  const int64_t hoff = (int64_t)b * a.bs_qkv + (int64_t)h * D * T;
  const T_* qb = static_cast<const T_*>(a.q) + hoff;
  const T_* kb = static_cast<const T_*>(a.k) + hoff;
  const T_* vb = static_cast<const T_*>(a.v) + hoff;
  const T_* dob = static_cast<const T_*>(a.dout) + (int64_t)b * a.bs_dout + (int64_t)h * D * T;
  const float* lseb = a.lse + (int64_t)bh * T;
  const float* deltab = a.delta + (int64_t)bh * T;
  const float scale_div = sqrtf((float)D);
  const bool drop = a.thr != 0;
  const uint64_t sm = drop ? at_mix64((uint64_t)*a.seed) : 0;

  const int kj = k0 + l32;  // this lane's key (B column / output column)
  const bool kvalid = kj < T;
  const bool kmasked = kj >= len;
  const float inv_t = 1.0f / (float)T;

  const bool dvalid = (D % 32 == 0) || (t * 32 + l32 < D);
  const T_* dor = dob + (int64_t)(t * 32 + l32) * T;
  const T_* qrow = qb + (int64_t)(t * 32 + l32) * T;
  f32x16 dk, dv;
#pragma unroll
  for (int r = 0; r < 16; ++r) dk[r] = dv[r] = 0.f;

  for (int q0 = 0; q0 < T; q0 += AT_Q) {
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
    const int qr = q0 + l32;  // A row (query) of this lane
    const bool qrv = qr < T;
    // S[q][key] = (Q / sqrt(D)) K^T, dP[q][key] = dO V^T
    at_mma<DT, KS>(
        s,
        [&](int n) { return qrv ? (float)qb[(uint32_t)((2 * n + lhi) * T + qr)] / scale_div : 0.f; },
        [&](int n) { return kvalid ? (float)kb[(uint32_t)((2 * n + lhi) * T + kj)] : 0.f; });
    at_mma<DT, KS>(
        dp, [&](int n) { return qrv ? (float)dob[(uint32_t)((2 * n + lhi) * T + qr)] : 0.f; },
        [&](int n) { return kvalid ? (float)vb[(uint32_t)((2 * n + lhi) * T + kj)] : 0.f; });
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = q0 + at_row(r, lhi);
      const bool qv = qi < T;
      const float lse = qv ? lseb[qi] : 0.f;
      const float delta = qv ? deltab[qi] : 0.f;
      const bool filled = qi >= len || kmasked;
      const float sv = filled ? -1e4f : s[r];
      // (a fully masked query row is T scores of -1e4: P = 1/T exactly, where
      // its lse = -1e4 + log T has an fp32 ulp of 1e-3)
      const float p = !(qv && kvalid) ? 0.f : (qi >= len ? inv_t : expf(sv - lse));
      float pd = p, g = dp[r];
      if (drop) {
        const bool keep = at_keep(sm, bh, T, qi, kj, a.thr);
        pd = keep ? p * a.inv_keep : 0.f;
        g = keep ? g * a.inv_keep : 0.f;
      }
      s[r] = pd;
      dp[r] = filled ? 0.f : p * (g - delta);
    }
    // dV^T[d][key] += dO^T[d][q] Pd[q][key];  dK^T[d][key] += (Q/sqrt(D))^T[d][q] dS[q][key]
    at_mma<DT, 16>(
        dv,
        [&](int r) {
          const int qi = q0 + at_row(r, lhi);
          return (dvalid && qi < T) ? (float)dor[qi] : 0.f;
        },
        [&](int r) { return s[r]; });
    at_mma<DT, 16>(
        dk,
        [&](int r) {
          const int qi = q0 + at_row(r, lhi);
          return (dvalid && qi < T) ? (float)qrow[qi] / scale_div : 0.f;
        },
        [&](int r) { return dp[r]; });
  }
  if (!kvalid) return;
  const int64_t goff = (int64_t)b * a.bs_dqkv + (int64_t)h * D * T;
  T_* dkb = static_cast<T_*>(a.dk) + goff;
  T_* dvb = static_cast<T_*>(a.dv) + goff;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int d = t * 32 + at_row(r, lhi);
    if (D % 32 == 0 || d < D) {
      dkb[(int64_t)d * T + kj] = (T_)dk[r];
      dvb[(int64_t)d * T + kj] = (T_)dv[r];
    }
  }
}

__global__ __launch_bounds__(256) void attn_dropout_mask_kernel(const int64_t* __restrict__ seed,
                                                                uint8_t* __restrict__ mask,
                                                                int T, int64_t total,
                                                                uint32_t thr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int key = (int)(i % T);
  const int qi = (int)((i / T) % T);
  const int bh = (int)(i / ((int64_t)T * T));
  mask[i] = thr == 0 ? 1 : (at_keep(at_mix64((uint64_t)*seed), bh, T, qi, key, thr) ? 1 : 0);
}

enum { AT_FWD, AT_DQ, AT_DKV };

template <int WHICH, int D, int DT>
void at_launch_one(dim3 grid, hipStream_t s, const at_args& a) {
  if constexpr (WHICH == AT_FWD)
    hipLaunchKernelGGL((attn_train_fwd_kernel<D, DT>), grid, dim3(64), 0, s, a);
  else if constexpr (WHICH == AT_DQ)
    hipLaunchKernelGGL((attn_bwd_dq_kernel<D, DT>), grid, dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<D, DT>), grid, dim3(64), 0, s, a);
}

template <int WHICH, int DT>
int at_launch_d(int head_dim, dim3 grid, hipStream_t s, const at_args& a) {
  switch (head_dim) {
    case 16: at_launch_one<WHICH, 16, DT>(grid, s, a); break;
    case 32: at_launch_one<WHICH, 32, DT>(grid, s, a); break;
    case 48: at_launch_one<WHICH, 48, DT>(grid, s, a); break;
    case 64: at_launch_one<WHICH, 64, DT>(grid, s, a); break;
    case 96: at_launch_one<WHICH, 96, DT>(grid, s, a); break;
    case 128: at_launch_one<WHICH, 128, DT>(grid, s, a); break;
    default: return VITS_E_UNSUP;
  }
  return vits_launch_status();
}

template <int WHICH>
int at_launch(int dtype, int head_dim, dim3 grid, hipStream_t s, const at_args& a) {
  switch (dtype) {
    case VITS_DT_F32: return at_launch_d<WHICH, VITS_DT_F32>(head_dim, grid, s, a);
    case VITS_DT_F16: return at_launch_d<WHICH, VITS_DT_F16>(head_dim, grid, s, a);
    case VITS_DT_BF16: return at_launch_d<WHICH, VITS_DT_BF16>(head_dim, grid, s, a);
    default: return VITS_E_UNSUP;
  }
}

bool at_head_dim_ok(int d) { return d == 16 || d == 32 || d == 48 || d == 64 || d == 96 || d == 128; }

// p -> drop threshold on the 32-bit draw
uint32_t at_threshold(float p) {
  const double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
}

}  // namespace

extern "C" int vits_attention_train_forward(const void* q, const void* k, const void* v, void* out,
                                            float* lse, int batch, int heads, int head_dim,
                                            int t_len, int64_t qkv_bstride, int64_t out_bstride,
                                            const int32_t* lengths, int dtype, float p_drop,
                                            const int64_t* seed, void* stream) {
  VITS_CHECK_ARG(q && k && v && out && lse && batch > 0 && heads > 0 && t_len > 0);
  VITS_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f && (p_drop == 0.f || seed));
  if (!at_head_dim_ok(head_dim)) return VITS_E_UNSUP;
  VITS_CHECK_SHAPE((int64_t)(head_dim + 1) * t_len <= INT32_MAX);  // 32-bit in-head offsets
  VITS_CHECK_SHAPE(qkv_bstride >= (int64_t)heads * head_dim * t_len);
  VITS_CHECK_SHAPE(out_bstride >= (int64_t)heads * head_dim * t_len);
  at_args a = {};
  a.q = q, a.k = k, a.v = v, a.out = out, a.lse = lse;
  a.H = heads, a.T = t_len, a.bs_qkv = qkv_bstride, a.bs_out = out_bstride;
  a.lengths = lengths, a.seed = seed;
  a.thr = at_threshold(p_drop), a.inv_keep = 1.0f / (1.0f - p_drop);
  dim3 grid((t_len + AT_Q - 1) / AT_Q, heads, batch);
  return count_ok(at_launch<AT_FWD>(dtype, head_dim, grid, as_stream(stream), a), VITS_CNT_ATTN);
}

extern "C" int vits_attention_backward(const void* q, const void* k, const void* v,
                                       const void* out, const void* dout, const float* lse,
                                       void* dq, void* dk, void* dv, float* delta, int batch,
                                       int heads, int head_dim, int t_len, int64_t qkv_bstride,
                                       int64_t out_bstride, int64_t dout_bstride,
                                       int64_t dqkv_bstride, const int32_t* lengths, int dtype,
                                       float p_drop, const int64_t* seed, void* stream) {
  VITS_CHECK_ARG(q && k && v && out && dout && lse && dq && dk && dv && delta);
  VITS_CHECK_ARG(batch > 0 && heads > 0 && t_len > 0);
  VITS_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f && (p_drop == 0.f || seed));
  if (!at_head_dim_ok(head_dim)) return VITS_E_UNSUP;
  VITS_CHECK_SHAPE((int64_t)(head_dim + 1) * t_len <= INT32_MAX);  // 32-bit in-head offsets
  const int64_t ct = (int64_t)heads * head_dim * t_len;
  VITS_CHECK_SHAPE(qkv_bstride >= ct && out_bstride >= ct && dout_bstride >= ct &&
                   dqkv_bstride >= ct);
  at_args a = {};
  a.q = q, a.k = k, a.v = v, a.o = out, a.dout = dout, a.dq = dq, a.dk = dk, a.dv = dv;
  a.lse = const_cast<float*>(lse), a.delta = delta;
  a.H = heads, a.T = t_len;
  a.bs_qkv = qkv_bstride, a.bs_out = out_bstride, a.bs_dout = dout_bstride;
  a.bs_dqkv = dqkv_bstride;
  a.lengths = lengths, a.seed = seed;
  a.thr = at_threshold(p_drop), a.inv_keep = 1.0f / (1.0f - p_drop);
  dim3 grid((t_len + AT_Q - 1) / AT_Q, heads, batch);
  hipStream_t s = as_stream(stream);
  int rc = count_ok(at_launch<AT_DQ>(dtype, head_dim, grid, s, a), VITS_CNT_ATTN);
  if (rc != VITS_OK) return rc;
  grid.x *= (head_dim + 31) / 32;  // one wave per (key tile, 32-wide d tile)
  return count_ok(at_launch<AT_DKV>(dtype, head_dim, grid, s, a), VITS_CNT_ATTN);
}

extern "C" int vits_attention_dropout_mask(const int64_t* seed, uint8_t* mask, int batch,
                                           int heads, int t_len, float p_drop, void* stream) {
  VITS_CHECK_ARG(mask && batch > 0 && heads > 0 && t_len > 0);
  VITS_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f && (p_drop == 0.f || seed));
  const int64_t total = (int64_t)batch * heads * t_len * t_len;
  hipLaunchKernelGGL(attn_dropout_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     as_stream(stream), seed, mask, t_len, total, at_threshold(p_drop));
  return vits_launch_status();
}
