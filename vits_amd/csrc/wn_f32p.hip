// wn_f32p.hip — one WN layer (modules.py:130-182) of the fp32 model's flow and
// posterior encoder as ONE kernel, in the split-fp32 arithmetic of the
// pre-split-weight conv (VITS_WDT_F32P, conv1d_impl.h):
//
//   (a | b) = in_layer(h) + bias + cond        Conv1d(H, 2H, k, dil), rows
//                                              gate-interleaved
//   g       = tanh(a) * sigmoid(b)             rounded to fp32 once
//   rs      = res_skip(g) + bias               1x1, 2H rows (last layer: H)
//   h_out   = h + rs[:H]                       (not on the last layer)
//   skip    = skip (+)= rs[H:]                 (last layer: all H rows)
//
// The two-conv path writes g to HBM and reads it back as three split planes
// for a 16-k-step GEMM whose staging, barriers and read-modify-write
// epilogue dominate it; its in_layer runs 64 x 128 tiles at two waves per
// SIMD.  Here one workgroup owns all 2H gate rows (res_skip mixes every gated
// channel) and a time tile of NG columns; 2H / 32 waves, each a 32 x NG wave
// tile in both phases (four waves per SIMD at H = 256):
//   phase 1: the in_layer GEMM, resblock_f32p.hip's / the conv kernel's
//            global-A loop: A fragments (hi / mid / lo planes) from the
//            host-split image in L2, three k-steps ahead (64-column tile:
//            one); the h window staged 64
//            channels at a time (zero padding, exact three-way bf16 split)
//            into double-buffered [t][64 + 4] planes - wave w stages channel
//            quad w, one 8-byte block of two time steps per lane;
//   gate:    tanh * sigmoid of the fp32 accumulators, split exactly into
//            three bf16 planes G[t][H + 8] in LDS, over the dead X buffers;
//            every column is computed unmasked, as the gate conv does;
//   phase 2: the 1x1 GEMM from G (no halo: NG stored columns, no barriers),
//            then the conv kernel's EPI_STORE2 expressions in its order:
//            acc + bias, res + v, y_old + v, the length mask.
// The arithmetic is the two-conv path's to the bit: the same split planes,
// the same k-step order (slab-major, then tap), the same six products per
// fragment pair in the same order, the same gate and epilogue expressions
// (tests/test_wn_fused_gpu.py checks equality); NG = 32 and 64 run the same
// k-steps per output element, so the tile choice changes no bit either.
// h_out must not be h: neighbouring workgroups still read h's halo columns.
#include <type_traits>

#include "conv1d_impl.h"

namespace {

using vits_conv::fast_sigmoid;
using vits_conv::fast_tanh;
using vits_conv::split3_bf16x4;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

struct WnArgs {
  vits_wn_layer_desc d;
  int batch;
};

constexpr int WN_KC = 64;  // in_layer channels per staged h chunk (one barrier each)

__host__ __device__ inline int wn_xcols(int NG, int k, int dil) {
  // NG + (k-1) dil window columns + up to 3 of alignment shift, 4-blocks
  return ((NG + (k - 1) * dil + 3 + 3) >> 2) << 2;
}
// LDS: the row constants [4H] floats (in_layer bias + cond, res_skip bias),
// then max(two X chunk buffers, the G planes)
__host__ __device__ inline int wn_lds_bytes(int H, int NG, int k, int dil) {
  const int xs = 2 * 3 * wn_xcols(NG, k, dil) * (WN_KC + 4);
  const int gsz = 3 * NG * (H + 8);
  return 4 * 4 * H + 2 * (xs > gsz ? xs : gsz) + 64;
}

// The gated value, rounded to fp32 once as the two-conv path stores it (the
// product must not contract into the split's first subtraction;
// resblock_f32p.hip rp_gate)
__device__ __forceinline__ float wn_gate(float a, float b) {
#pragma clang fp contract(off)
  return fast_tanh(a) * fast_sigmoid(b);
}

// A copy of a lane index the compiler cannot see through: what a phase
// derives from it is recomputed there instead of being held across the
// k-loop (the kernel runs at the 128-register limit; resblock_f32p.hip)
template <typename T>
__device__ __forceinline__ T wn_fresh(T v) {
  asm volatile("" : "+v"(v));
  return v;
}

// A wave-uniform global address held in scalar registers, for loads of the
// form scalar base + 32-bit lane offset
template <typename T>
__device__ __forceinline__ const T* wn_sbase(const T* p) {
  uint64_t u = reinterpret_cast<uint64_t>(p);
  asm("" : "+s"(u));
  return (const T*)reinterpret_cast<const __attribute__((address_space(1))) T*>(u);
}

template <int H, int NG>
__global__ __launch_bounds__(H * 4, 4) void wn_layer_f32p_kernel(const WnArgs A) {
  typedef std::integral_constant<bool, true> edge_t;       // a tile that touches the end
  typedef std::integral_constant<bool, false> interior_t;  // all columns inside [0, L)
  constexpr int M1 = 2 * H;           // gate rows
  constexpr int NT = (M1 / 32) * 64;  // one wave per 32 rows
  constexpr int TN = NG / 32;
  constexpr int KC = WN_KC;
  constexpr int KCP = KC + 4;   // X chunk row pitch (bf16)
  constexpr int GP = H + 8;     // G row pitch (bf16): 16-byte rows
  constexpr int GPL = NG * GP;  // G plane (elements)
  constexpr int S1 = H / 16, S2 = H / 16;
  static_assert(NT == H * 4 && NT <= 1024, "threads");
  static_assert(KC / 4 == NT / 64, "staging: one channel quad per wave");
  static_assert(NG == 32 || NG == 64, "tile columns");
  typedef bf16x8 av_t;

  const vits_wn_layer_desc& p = A.d;
  const int b = blockIdx.z;
  const int Tn = p.t_len;
  const int L = p.lengths ? min(Tn, (int)p.lengths[b]) : Tn;
  const int n0 = blockIdx.x * NG;
  if (n0 >= Tn) return;
  if (p.lengths && p.len_skip > 0 && n0 >= L + p.len_skip) return;
  const int M2 = p.last ? H : 2 * H;  // res_skip rows

  extern __shared__ float smem[];
  float* const erow = smem;  // [2H] in_layer bias + cond (gate-interleaved), [2H] res_skip bias
  __bf16* const reg = reinterpret_cast<__bf16*>(smem + 4 * H);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: wave-uniform rows)
  const int wm = wid * 32;
  const int l32 = lane & 31;
  const int lhi = lane >> 5;

  const int k = p.k;
  const int dil = p.dil;
  const int p1 = (k - 1) * dil / 2;
  const int tw0 = n0 - p1;      // time of window column 0
  const int xstart = tw0 & ~1;  // 8-byte aligned block start
  const int xcols = wn_xcols(NG, k, dil);
  // interior tile (block-uniform): every stored column inside [0, L)
  const bool interior = n0 + NG <= L;

  {
    const float* cond = p.cond ? p.cond + (int64_t)b * p.cond_bstride : nullptr;
    for (int r = tid; r < 4 * H; r += NT) {
      float e = 0.f;
      if (r < M1) {
        const int idx = (r & 1) ? H + (r >> 1) : (r >> 1);
        if (p.b1) e = p.b1[idx];
        if (cond) e += cond[idx];
      } else if (p.b2 && r - M1 < M2) {
        e = p.b2[r - M1];
      }
      erow[r] = e;
    }
  }

  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  // six products per fragment pair, small terms first (conv1d_impl.h's F32P
  // order: bitwise the conv's sums)
  auto mma = [&](const av_t* a, const av_t* bh, const av_t* bm, const av_t* bl) {
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
      f32x16 c = acc[ni];
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], bl[ni], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], bh[ni], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], bm[ni], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], bm[ni], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], bh[ni], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], bh[ni], c, 0, 0, 0);
      acc[ni] = c;
    }
  };
  // A fragments of flat step s (image [cin_pad/16][k][2][3][m_pad][8]): plane
  // q, half lhi, rows wm + l32.  Step, plane and row base are wave-uniform (a
  // scalar address); the lane adds one 32-bit byte offset `al`.
  auto loadA = [&](const __bf16* w, uint32_t al, int64_t wstep, int m_pad, int s, int total,
                   av_t* a) {
    const __bf16* wp = w + (int64_t)(s < total ? s : total - 1) * wstep + (int64_t)wm * 8;
    const uint32_t av = wn_fresh(al);
#pragma unroll
    for (int q = 0; q < 3; ++q)
      a[q] = *reinterpret_cast<const av_t*>(
          reinterpret_cast<const char*>(wn_sbase(wp + (int64_t)q * m_pad * 8)) + av);
  };

  // A fragments run PF - 1 k-steps ahead in a register ring (slot = step %
  // PF; a chunk is 4 k steps and res_skip 16: multiples of PF, so the ring
  // never rotates).  Every workgroup streams both whole images alone; with
  // few workgroups (B = 1) or weights not yet in L2 one step ahead leaves the
  // loop waiting on each fetch.  The 64-column tile has no registers for more.
  constexpr int PF = TN == 1 ? 4 : 2;
  static_assert((KC / 16) % PF == 0 && S2 % PF == 0, "ring alignment");
  av_t ar[PF][3];
  av_t bh[2][TN], bm[2][TN], bl[2][TN];

  // ---------------- phase 1: in_layer over NG columns from n0 ----------------
  const float* xb = p.h + (int64_t)b * p.h_bstride;
  {
    const int xsh = tw0 - xstart;  // window column c sits at LDS row c + xsh
    const int nblk = xcols >> 1;   // 2-step blocks per row (<= 64: one per lane)
    const int xpl = xcols * KCP;   // plane (elements)
    __bf16* const xbuf0 = reg;
    __bf16* const xbuf1 = reg + 3 * xpl;
    // wave w stages channel quad w of the chunk, lane l the 2-step block l
    // (8-byte loads: 8 staging registers held under a chunk's MFMAs, not 16)
    const int tt = xstart + 2 * lane;
    const bool xact = lane < nblk;
    const bool xok = xact && tt >= 0 && tt < Tn;  // T % 2 == 0: a block is all in or out
    // (byte offset < 2^31: the host checks H * cstride < 2^31 elements / 4 rows)
    const uint32_t xoff = xok ? (uint32_t)tt * 4u : 0u;
    f32x2v xr[4];
    // loads issued unconditionally (a block outside reads the row's first
    // columns - always inside the tensor - and is zeroed in lstore)
    auto gload = [&](int ch) __attribute__((always_inline)) {
      const float* base = xb + (int64_t)(ch * KC + 4 * wid) * p.h_cstride;
      const uint32_t xo = wn_fresh(xoff);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float* row = wn_sbase(base + (int64_t)i * p.h_cstride);
        xr[i] = *reinterpret_cast<const f32x2v*>(reinterpret_cast<const char*>(row) + xo);
      }
    };
    auto lstore = [&](__bf16* xs) __attribute__((always_inline)) {
      const int fl = wn_fresh(lane);
      if (fl < nblk) {
        __bf16* xh = xs + 2 * fl * KCP + 4 * wid;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          f32x4v w;
#pragma unroll
          for (int i = 0; i < 4; ++i) w[i] = xok ? xr[i][e] : 0.f;
          bf16x4 h4, m4, l4;
          split3_bf16x4(w, h4, m4, l4);
          *reinterpret_cast<bf16x4*>(xh + e * KCP) = h4;
          *reinterpret_cast<bf16x4*>(xh + xpl + e * KCP) = m4;
          *reinterpret_cast<bf16x4*>(xh + 2 * xpl + e * KCP) = l4;
        }
      }
    };
    // B fragments of tap j, slab g of the chunk: rows ni * 32 + l32 + j * dil
    // (+ xsh), channels 16 g + 8 lhi .. + 8 (two 8-byte reads per plane)
    auto loadB = [&](const __bf16* xs, int j, int g, av_t* bh, av_t* bm, av_t* bl) {
      const int P4 = xpl / 4;
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) {
        const bf16x4* xp = reinterpret_cast<const bf16x4*>(
            xs + (ni * 32 + l32 + j * dil + xsh) * KCP + 16 * g + 8 * lhi);
        bh[ni] = __builtin_shufflevector(xp[0], xp[1], 0, 1, 2, 3, 4, 5, 6, 7);
        bm[ni] = __builtin_shufflevector(xp[P4], xp[P4 + 1], 0, 1, 2, 3, 4, 5, 6, 7);
        bl[ni] = __builtin_shufflevector(xp[2 * P4], xp[2 * P4 + 1], 0, 1, 2, 3, 4, 5, 6, 7);
      }
    };
    const __bf16* wl = reinterpret_cast<const __bf16*>(p.w1);
    const uint32_t al = (uint32_t)((lhi * 3) * p.m_pad1 + l32) * 16u;
    const int64_t wstep = (int64_t)16 * 3 * p.m_pad1;
    const int total = S1 * k;
    const int nst = (KC / 16) * k;  // k-steps per chunk: slab-major, then tap
#pragma unroll
    for (int i = 0; i < PF - 1; ++i) loadA(wl, al, wstep, p.m_pad1, i, total, ar[i]);
    gload(0);
    lstore(xbuf0);
    __syncthreads();
    for (int ch = 0; ch < H / KC; ++ch) {
      const bool more = ch + 1 < H / KC;
      if (more) gload(ch + 1);  // in flight under this chunk's MFMAs
      const __bf16* xs = (ch & 1) ? xbuf1 : xbuf0;
      const int s0 = ch * nst;
      int j = 0, g = 0;  // (tap, slab) of the next B load
      auto next = [&]() {
        if (++j == k) {
          j = 0;
          ++g;
        }
      };
      loadB(xs, 0, 0, bh[0], bm[0], bl[0]);
      // the loads of the steps ahead pinned before step st + u's MFMAs (past
      // the chunk's end: the next chunk's first steps)
      for (int st = 0; st < nst; st += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
          loadA(wl, al, wstep, p.m_pad1, s0 + st + u + PF - 1, total, ar[(u + PF - 1) % PF]);
          next();
          if (st + u + 1 < nst) loadB(xs, j, g, bh[(u + 1) & 1], bm[(u + 1) & 1], bl[(u + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
          mma(ar[u], bh[u & 1], bm[u & 1], bl[u & 1]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (more) lstore((ch & 1) ? xbuf0 : xbuf1);
      __syncthreads();
    }
  }

  // ---------------- gate -> G planes (over the dead X buffers) ---------------
  // rows 4 lhi + 8 g .. + 3 of the wave's 32: a_q, b_q, a_q+1, b_q+1
  __bf16* const gs = reg;
  {
    const int fl = wn_fresh(lane);
    const int l32 = fl & 31, lhi = fl >> 5;
    f32x4v er[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      er[g] = *reinterpret_cast<const f32x4v*>(erow + wm + 4 * lhi + 8 * g);
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
      const int col = ni * 32 + l32;
#pragma unroll
      for (int r = 0; r < 16; r += 4) {
        const int row = wm + 4 * lhi + 8 * (r >> 2);
        const f32x4v e = er[r >> 2];
        const float g0 = wn_gate(acc[ni][r] + e[0], acc[ni][r + 1] + e[1]);
        const float g1 = wn_gate(acc[ni][r + 2] + e[2], acc[ni][r + 3] + e[3]);
        __bf16* gp = gs + col * GP + (row >> 1);
        const f32x4v w = {g0, g1, 0.f, 0.f};
        bf16x4 h4, m4, l4;
        split3_bf16x4(w, h4, m4, l4);
        *reinterpret_cast<bf16x2*>(gp) = __builtin_shufflevector(h4, h4, 0, 1);
        *reinterpret_cast<bf16x2*>(gp + GPL) = __builtin_shufflevector(m4, m4, 0, 1);
        *reinterpret_cast<bf16x2*>(gp + 2 * GPL) = __builtin_shufflevector(l4, l4, 0, 1);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;
    }
  }
  __syncthreads();
  if (wm >= M2) return;  // (last layer: res_skip has H rows)

  // ---------------- phase 2: res_skip (1x1) from G ---------------------------
  {
    const int fl = wn_fresh(lane);
    const int l32 = fl & 31, lhi = fl >> 5;
    const __bf16* wl = reinterpret_cast<const __bf16*>(p.w2);
    const uint32_t al = (uint32_t)((lhi * 3) * p.m_pad2 + l32) * 16u;
    const int64_t wstep = (int64_t)16 * 3 * p.m_pad2;
    const int total = S2;
    const __bf16* gl = gs + l32 * GP + 8 * lhi;
    int g = 0;  // slab of the next B load
    auto loadB = [&](av_t* bh, av_t* bm, av_t* bl) {
      const __bf16* x = gl + 16 * g;
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) {
        bh[ni] = *reinterpret_cast<const av_t*>(x + ni * 32 * GP);
        bm[ni] = *reinterpret_cast<const av_t*>(x + ni * 32 * GP + GPL);
        bl[ni] = *reinterpret_cast<const av_t*>(x + ni * 32 * GP + 2 * GPL);
      }
      ++g;
    };
#pragma unroll
    for (int i = 0; i < PF - 1; ++i) loadA(wl, al, wstep, p.m_pad2, i, total, ar[i]);
    loadB(bh[0], bm[0], bl[0]);
    for (int s = 0; s < total; s += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        loadA(wl, al, wstep, p.m_pad2, s + u + PF - 1, total, ar[(u + PF - 1) % PF]);
        if (s + u + 1 < total) loadB(bh[(u + 1) & 1], bm[(u + 1) & 1], bl[(u + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        mma(ar[u], bh[u & 1], bm[u & 1], bl[u & 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // epilogue, the conv kernel's EPI_STORE2 / STORE expressions in their order:
  // v = acc + bias; h rows: h + v; skip rows: skip_old + v when accumulating;
  // 0 at t >= L.  A wave's 32 rows lie on one side of the split (H % 32 == 0).
  // Every load of a 32 x 32 sub-tile is issued before its first store; rows
  // are a scalar row base + one 32-bit lane offset (4 lhi rows + the column).
  const bool to_h = !p.last && wm < H;
  const int yr = (p.last || wm < H) ? wm : wm - H;  // first output row
  const float* const rrow = xb + (int64_t)wm * p.h_cstride;  // (to_h only)
  float* const yb = to_h ? p.h_out + (int64_t)b * p.ho_bstride + (int64_t)yr * p.ho_cstride
                         : p.skip + (int64_t)b * p.skip_bstride + (int64_t)yr * p.skip_cstride;
  const int ycs = to_h ? p.ho_cstride : p.skip_cstride;
  const bool accum = !to_h && p.accumulate;
  auto epilogue = [&](auto edge) __attribute__((always_inline)) {
    const int fl = wn_fresh(lane);
    const int l32 = fl & 31, lhi = fl >> 5;
    f32x4v e2[4];  // res_skip bias rows 4 lhi + 8 g .. + 3
#pragma unroll
    for (int g = 0; g < 4; ++g)
      e2[g] = *reinterpret_cast<const f32x4v*>(erow + M1 + wm + 4 * lhi + 8 * g);
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
      const int t = n0 + ni * 32 + l32;
      const bool st = decltype(edge)::value ? t < Tn : true;
      const int tc = st ? t : 0;
      const uint32_t xv = (uint32_t)(4 * lhi * p.h_cstride + tc) * 4u;
      const uint32_t yv = (uint32_t)(4 * lhi * ycs + tc) * 4u;
      // element r: row (r & 3) + 8 (r >> 2) of the lane's four-row groups
      auto xat = [&](int r) __attribute__((always_inline)) -> const float& {
        const float* row = rrow + (int64_t)((r & 3) + 8 * (r >> 2)) * p.h_cstride;
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(row) + xv);
      };
      auto yat = [&](int r) __attribute__((always_inline)) -> float& {
        float* row = yb + (int64_t)((r & 3) + 8 * (r >> 2)) * ycs;
        return *reinterpret_cast<float*>(reinterpret_cast<char*>(row) + yv);
      };
      float o[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] = acc[ni][r] + e2[r >> 2][r & 3];
      if (to_h) {
        float rv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) rv[r] = xat(r);
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = rv[r] + o[r];  // (the conv's rv + res_scale * v, scale 1)
      }
      if (accum) {
        float yo[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) yo[r] = yat(r);
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = yo[r] + o[r];
      }
      if (st) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if constexpr (decltype(edge)::value) o[r] = t < L ? o[r] : 0.f;
          yat(r) = o[r];
        }
      }
    }
  };
  if (interior)
    epilogue(interior_t());
  else
    epilogue(edge_t());
}

// Tile columns by grid size, as conv1d_dispatch chooses its tile: 64 columns
// halve the weight traffic per output column (every workgroup streams both
// images from L2) but need 256 workgroups to cover the chip.
int wn_pick_ng(const vits_wn_layer_desc& d, int batch) {
  if (d.ng == 32 || d.ng == 64) return d.ng;
  const long tiles64 = (long)((d.t_len + 63) / 64) * batch;
  return tiles64 >= 256 ? 64 : 32;
}

template <int H, int NG>
int wn_launch(const vits_wn_layer_desc& d, int batch, hipStream_t s) {
  const int lds = wn_lds_bytes(H, NG, d.k, d.dil);
  if (lds > 160 * 1024) return VITS_E_UNSUP;
  WnArgs a;
  a.d = d;
  a.batch = batch;
  hipLaunchKernelGGL((wn_layer_f32p_kernel<H, NG>), dim3((d.t_len + NG - 1) / NG, 1, batch),
                     dim3(H * 4), lds, s, a);
  return vits_launch_status();
}

}  // namespace

// argument checks of one fused WN layer (no GPU call)
int vits_wn_layer_check(const vits_wn_layer_desc& d, int batch) {
  VITS_CHECK_ARG(batch >= 1 && batch <= 65535);
  VITS_CHECK_ARG(d.h && d.w1 && d.w2 && d.skip);
  VITS_CHECK_ARG(d.last ? d.h_out == nullptr : d.h_out != nullptr);
  // other workgroups still read h (halos, residual): never write in place
  VITS_CHECK_ARG(reinterpret_cast<const void*>(d.h_out) != reinterpret_cast<const void*>(d.h) &&
                 reinterpret_cast<const void*>(d.skip) != reinterpret_cast<const void*>(d.h) &&
                 reinterpret_cast<const void*>(d.skip) != reinterpret_cast<const void*>(d.h_out));
  VITS_CHECK_ARG(d.ng == 0 || d.ng == 32 || d.ng == 64);
  VITS_CHECK_SHAPE(d.hidden == 256);
  VITS_CHECK_SHAPE(d.k >= 1 && d.k <= 15 && (d.k & 1) == 1 && d.dil >= 1 && d.t_len > 0);
  // the window's 2-step blocks: one per lane (64-column tile: 64 + 56 + 6)
  VITS_CHECK_SHAPE((d.k - 1) * d.dil <= 56);
  const int m2 = d.last ? d.hidden : 2 * d.hidden;
  // images [cin_pad/16][k][2][3][m_pad][8] bf16
  VITS_CHECK_SHAPE(d.m_pad1 >= 2 * d.hidden && d.m_pad2 >= m2 && (d.m_pad1 & 3) == 0 &&
                   (d.m_pad2 & 3) == 0);
  VITS_CHECK_SHAPE(d.cin_pad1 == d.hidden && d.cin_pad2 == d.hidden);
  // h staging in aligned blocks: time-contiguous 16-byte aligned rows, T % 4 == 0
  VITS_CHECK_SHAPE((d.t_len & 3) == 0 && (d.h_cstride & 3) == 0 && (d.h_bstride & 3) == 0 &&
                   d.h_cstride >= d.t_len && d.skip_cstride >= d.t_len &&
                   (d.last || d.ho_cstride >= d.t_len) &&
                   (reinterpret_cast<uintptr_t>(d.h) & 15) == 0);
  VITS_CHECK_SHAPE((reinterpret_cast<uintptr_t>(d.skip) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(d.h_out) & 3) == 0);
  // 32-bit lane offsets within one utterance (staging, epilogue)
  VITS_CHECK_SHAPE((int64_t)d.hidden * d.h_cstride < (1LL << 31) &&
                   (int64_t)d.hidden * d.skip_cstride < (1LL << 31) &&
                   (d.last || (int64_t)d.hidden * d.ho_cstride < (1LL << 31)));
  VITS_CHECK_SHAPE((reinterpret_cast<uintptr_t>(d.w1) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(d.w2) & 15) == 0);
  return VITS_OK;
}

// one checked layer on the stream (conv1d.hip's mixed sequence entry too)
int vits_wn_layer_launch(const vits_wn_layer_desc& d, int batch, hipStream_t s) {
  const int rc = wn_pick_ng(d, batch) == 64 ? wn_launch<256, 64>(d, batch, s)
                                            : wn_launch<256, 32>(d, batch, s);
  return count_ok(rc, VITS_CNT_CONV_SPLIT);
}

extern "C" int vits_wn_layers_f32p_forward(const vits_wn_layer_desc* d, int n, int batch,
                                           void* stream) {
  if (!d || n < 1) return VITS_E_ARG;
  for (int i = 0; i < n; ++i) {  // every layer is checked before the first launch
    const int rc = vits_wn_layer_check(d[i], batch);
    if (rc) return rc;
  }
  for (int i = 0; i < n; ++i) {
    const int rc = vits_wn_layer_launch(d[i], batch, as_stream(stream));
    if (rc) return rc;
  }
  return VITS_OK;
}
