// resblock_f32p.hip — one ResBlock2 dilation pair of the fp32 Generator's
// 32-, 64-, 128- and 256-channel stages as ONE kernel, in the split-fp32
// arithmetic of the pre-split-weight conv (VITS_WDT_F32P, conv1d_impl.h):
//
//   y = x + c2( tanh(a + sa) * sigmoid(b + sb) ) ,   (a | b) = c1(lrelu(x, 0.1))
//
// (modules.py:250-260; c1 = Conv1d(C, C, k, dil d), c2 = Conv1d(C/2, C, k),
// sa / sb the utterance's cond Linear; models.py:306-318 averages the
// branches: the last pair of each branch accumulates into the stage output).
//
// The two-conv path writes the gated tensor (fp32) to HBM, reads it back
// with c2's halo, and re-reads x as the residual; c2 is a short-K GEMM
// (K = C/2 * k) whose own window staging, barriers and epilogue dominate
// it (0.2-0.4 of the split-fp32 ceiling on the headline step).  Here one
// workgroup owns a time tile of BN = NG - (k - 1) outputs and all C
// channels; every wave computes a 32 x 64 sub-tile (the 16-bit modes: 64 x
// 64) in both phases:
//   phase 1: the c1 GEMM over NG columns (the tile plus c2's (k-1)/2 halo
//            each side; rows gate-interleaved), exactly the conv kernel's
//            global-A loop: A fragments (hi / mid / lo planes) from the
//            host-split image in L2, one k-step ahead; the x window staged
//            16 channels (C = 256: 64) at a time (lrelu, zero padding, exact
//            three-way bf16 split) into double-buffered [t][16 + 4] planes;
//   gate:    tanh * sigmoid of the fp32 accumulators, split exactly into
//            three bf16 planes G[t][C/2 + 8] in LDS (zero outside [0, L):
//            c2's own zero padding, and the utterance end) - over the X
//            buffers, which are dead by then;
//   phase 2: the c2 GEMM from G (tap j = row shift j), no barriers, then
//            residual (x: L2-resident from phase 1) + bias (+ accumulate /
//            branch-mean division) to HBM.
// Halo columns are recomputed by the neighbouring tile, never exchanged.
// The arithmetic is the two-conv path's to the bit: the same split planes,
// the same k-step order (slab-major, then tap), the same six products per
// fragment pair in the same order, the same gate and epilogue expressions
// (tests/test_resblock_f32p_gpu.py checks equality).  Workgroup tiles: C =
// 64 -> 64 x 256 (C = 32: 32 x 256), C = 128 -> 128 x 128, two workgroups per
// CU; C = 256 -> 256 x 128, one per CU.  Split-fp32 at C >= 64: 32 x 64 wave
// tiles (2 x 4, 4 x 2 and 8 x 2 waves: 512 / 512 / 1024 threads) at 128
// VGPRs, four waves per SIMD - twice the waves of the 64 x 64 wave tile on
// the same workgroup tile, LDS and grid, to cover the phases that issue no
// MFMA (staging, gate, epilogue, barriers); DESIGN.md 4m, and rp_tm below
// for the build switches that bring the 64 x 64 form back.  Every launch
// holds up to 3 independent pairs (the branches of a stage).
//
// MODE 1 / 2: the same tile for a bf16 / fp16 model's 256-channel pairs
// (vits_resblock_pair16_forward routes them here - resblock16.hip stages a
// whole window, which 256 channels do not fit): 16-bit x / y in HBM, one
// operand plane, one MFMA per fragment pair, the gated tensor rounded to the
// 16-bit type in LDS as the two-conv path rounds it in HBM.  C5 (B=4,
// Ty=2500): 9.84 -> 9.07 ms/step (tools/r05_p256.sh).  The 128-channel
// pairs measured the same here as in resblock16 (r05_p128.sh) and stay there.
//
// Per-element work (DESIGN.md "Fused split pair: per-element work"): a tile
// whose staged window and gate columns all lie inside [0, L) - block-uniform,
// the large majority - takes paths without the validity selects (staging),
// the `in` select (gate) and the length select (epilogue); the epilogue
// addresses rows as a scalar row base + one 32-bit lane offset per sub-tile.
// MEAN: the last pairs of a stage's branches as one launch - the workgroup
// runs the members in order on one common tile (NG - (kmax - 1) columns) and
// keeps (o0 + o1) + o2 in registers, then / n: the accumulating launches'
// arithmetic in their order, without their reads and writes of the output.
#include <type_traits>

#include "conv1d_impl.h"

namespace {

using vits_conv::fast_sigmoid;
using vits_conv::fast_tanh;
using vits_conv::split3_bf16x4;

constexpr int RP_GROUP = 3;
struct RpGroup {
  vits_resblock_pair_desc d[RP_GROUP];
  int n;
  int batch;
  int bn;  // MEAN: the common tile's stored columns (NG - (kmax - 1))
};

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

// operand mode: 0 = split fp32 (fp32 x / y, three exact bf16 planes per
// operand, six products), 1 = bf16 / 2 = fp16 models (16-bit x / y as the
// 16-bit decoder holds them, one plane, one product; the gated tensor rounded
// to the 16-bit type as the two-conv path stores it)
template <int MODE>
struct RpT {
  typedef float xt;   // activation element in HBM
  typedef __bf16 lt;  // LDS / MFMA operand element
  static constexpr int NPL = 3;
};
template <>
struct RpT<1> {
  typedef __bf16 xt;
  typedef __bf16 lt;
  static constexpr int NPL = 1;
};
template <>
struct RpT<2> {
  typedef _Float16 xt;
  typedef _Float16 lt;
  static constexpr int NPL = 1;
};
__host__ __device__ constexpr int rp_npl(int mode) { return mode == 0 ? 3 : 1; }

__host__ __device__ constexpr int rp_ng(int C) { return C <= 64 ? 256 : 128; }
// Wave-tile rows / 32 (TM): 2 = a 64 x 64 wave tile (64 accumulators + 96
// double-buffered operand registers: ~200 VGPRs, two waves per SIMD), 1 =
// 32 x 64, twice the waves on the same workgroup tile at <= 128 VGPRs (four
// per SIMD).  Split-fp32 at C = 64 / 128 / 256: chosen per C by measurement
// (DESIGN.md "Fused split pair: four waves per SIMD"; -DVITS_RP_TM64=2 etc.
// rebuild the other side).  C = 32 is one 32-row wave tile; the 16-bit modes
// keep 64 x 64 (two 8-wave workgroups measured equal there).
#ifndef VITS_RP_TM64
#define VITS_RP_TM64 1
#endif
#ifndef VITS_RP_TM128
#define VITS_RP_TM128 1
#endif
#ifndef VITS_RP_TM256
#define VITS_RP_TM256 1
#endif
// -DVITS_RP_OTHER_SIDE: every per-C choice flipped - the Makefile's second,
// one-file library, through which the tests run the side that is not shipped
#ifdef VITS_RP_OTHER_SIDE
#define VITS_RP_SIDE(tm) (3 - (tm))
#else
#define VITS_RP_SIDE(tm) (tm)
#endif
__host__ __device__ constexpr int rp_tm(int C, int mode = 0) {
  return C == 32     ? 1
         : mode != 0 ? 2
         : C == 64   ? VITS_RP_SIDE(VITS_RP_TM64)
         : C == 128  ? VITS_RP_SIDE(VITS_RP_TM128)
                     : VITS_RP_SIDE(VITS_RP_TM256);
}
// threads: (C / 32 TM) row-waves x (NG / 64) column-waves
__host__ __device__ constexpr int rp_threads(int C, int tm) {
  return (C / (32 * tm)) * (rp_ng(C) / 64) * 64;
}
// c1 channels per staged X chunk (one barrier each): 16 where two workgroups
// share a CU (the double-buffered chunk must fit beside nothing but the G
// planes it aliases), 64 for the one-workgroup 256-channel tile (its X
// buffers still fit the LDS: four slabs per barrier).  C = 32: the whole C
// as one chunk - one staging pass, no mid-loop barrier, no second buffer,
// less LDS; measured against 16 on the headline step's three 32-channel
// launches: 0.747 / 0.721 / 0.699 -> 0.702 / 0.687 / 0.692 ms
// (profiles/pairs_kc32_ab.txt; -DVITS_RP_KC32=16 rebuilds the other side)
#ifndef VITS_RP_KC32
#define VITS_RP_KC32 32
#endif
__host__ __device__ constexpr int rp_kc(int C, int mode = 0) {
  // (the 16-bit mode measured the same at 32 / 64)
  return C == 256 ? 64 : C == 32 ? VITS_RP_KC32 : 16;
}
__host__ __device__ inline int rp_xcols(int NG, int k, int dil) {
  // NG + (k-1) dil window columns + up to 3 of alignment shift, 4-blocks
  return ((NG + (k - 1) * dil + 3 + 3) >> 2) << 2;
}
// LDS: erow [2C] floats, then max(two X slab buffers, the G planes)
__host__ __device__ inline int rp_lds_bytes(int C, int k, int dil, int mode = 0) {
  const int NG = rp_ng(C), npl = rp_npl(mode);
  // (a whole-C chunk needs no second buffer)
  const int nbuf = rp_kc(C, mode) < C ? 2 : 1;
  const int xs = nbuf * npl * rp_xcols(NG, k, dil) * (rp_kc(C, mode) + 4);
  const int gsz = npl * (NG + 16) * (C / 2 + 8);
  return 4 * 2 * C + 2 * (xs > gsz ? xs : gsz) + 64;
}
// minimum waves per SIMD the kernel is compiled for (launch_bounds' second
// argument): two 4-wave workgroups per CU below 256 channels, one 8-wave one
// at 256.  (16-bit 256: two 8-wave workgroups per CU need <= 128 VGPRs and
// spill 24; measured the same on C5, tools/r05_p256b.sh)
// The 32 x 64 wave tile: four waves per SIMD (two 8-wave workgroups, or one
// 16-wave one at 256 channels).
__host__ __device__ constexpr int rp_occ(int C, int, int tm) {
  return tm == 1 && C >= 64 ? 4 : C == 256 ? 1 : 2;
}

// The gated value, rounded to fp32 once as the two-conv path stores it: the
// product must not contract into the split's first subtraction (g - hi as
// fma(tanh, sigmoid, -hi) keeps the product's low bits; with no select
// between them on interior tiles the compiler would)
__device__ __forceinline__ float rp_gate(float a, float b) {
#pragma clang fp contract(off)
  return fast_tanh(a) * fast_sigmoid(b);
}

// max of two floats as one v_max_f32 (fmaxf costs a canonicalising
// instruction per loaded operand first; the hardware max needs none)
__device__ __forceinline__ float rp_max(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// A copy of a lane / thread index the compiler cannot see through.  The 32 x
// 64 wave tile runs at the 128-register limit; what a phase derives from its
// own copy (LDS addresses, columns, row offsets: a few integer instructions)
// is recomputed in that phase instead of being held - or spilled - across
// the k-loop.
template <typename T>
__device__ __forceinline__ T rp_fresh(T v) {
  asm volatile("" : "+v"(v));
  return v;
}

// A wave-uniform global address held in scalar registers, for loads of the
// form scalar base + 32-bit lane offset (left to itself the compiler folds
// the uniform part into a 64-bit vector address per load).
template <typename T>
__device__ __forceinline__ const T* rp_sbase(const T* p) {
  uint64_t u = reinterpret_cast<uint64_t>(p);
  asm("" : "+s"(u));
  return (const T*)reinterpret_cast<const __attribute__((address_space(1))) T*>(u);
}

template <int C, int MODE = 0, bool MEAN = false, int TM = rp_tm(C, MODE)>
__global__ __launch_bounds__(rp_threads(C, TM), rp_occ(C, MODE, TM)) void resblock_f32p_kernel(
    const RpGroup G) {
  typedef std::integral_constant<bool, true> edge_t;       // a tile that touches an end
  typedef std::integral_constant<bool, false> interior_t;  // all columns inside [0, L)
  typedef typename RpT<MODE>::xt xt;
  typedef typename RpT<MODE>::lt lt;
  constexpr int NPL = RpT<MODE>::NPL;
  typedef lt lt8 __attribute__((ext_vector_type(8)));
  typedef lt lt4 __attribute__((ext_vector_type(4)));
  typedef lt lt2 __attribute__((ext_vector_type(2)));
  typedef xt xt4 __attribute__((ext_vector_type(4)));
  constexpr int H = C / 2;
  static_assert(TM == 1 || (TM == 2 && C >= 64), "wave tile rows");
  constexpr int NT = rp_threads(C, TM);
  constexpr int WAVES_M = C / (32 * TM);
  constexpr int WAVES_N = NT / 64 / WAVES_M;
  constexpr int NG = 64 * WAVES_N;
  static_assert(NG == rp_ng(C), "tile columns");
  constexpr int TN = 2;  // (32 TM) x 64 per wave
  constexpr int KC = rp_kc(C, MODE);          // c1 channels per staged chunk
  constexpr int KCP = KC + 4;           // X chunk row pitch (bf16)
  constexpr int GP = H + 8;              // G row pitch (bf16): 16-byte rows
  constexpr int GPL = (NG + 16) * GP;    // G plane (elements)
  constexpr int S1 = C / 16, S2 = H / 16;
  constexpr int NU = ((KC / 4) * ((NG + 102) / 4) + NT - 1) / NT;  // staging units per thread
  typedef lt8 av_t;
  constexpr int NB = NPL == 3 ? TN : 1;  // (mid / lo B planes: split only)
  constexpr bool REMAT = TM == 1 && C >= 64;  // (rp_fresh: the 128-register forms)

  // MEAN: every member on this workgroup's tile (blockIdx.z = utterance; the
  // members share t_len and lengths); else blockIdx.z = member * batch + b
  const int gi = MEAN ? 0 : (int)blockIdx.z / G.batch;
  const int b = (int)blockIdx.z - gi * G.batch;
  const int Tn = G.d[gi].t_len;
  const int L = G.d[gi].lengths ? min(Tn, (int)G.d[gi].lengths[b]) : Tn;
  const int BN = MEAN ? G.bn : NG - (G.d[gi].k - 1);  // columns this tile stores
  const int n0 = blockIdx.x * BN;
  if (n0 >= Tn) return;
  if (G.d[gi].lengths && G.d[gi].len_skip > 0 && n0 >= L + G.d[gi].len_skip) return;

  extern __shared__ float smem[];
  float* const erow = smem;  // [2C]: c1 bias + cond (gate-interleaved), c2 bias
  lt* const reg = reinterpret_cast<lt*>(smem + 2 * C);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: wave-uniform rows)
  const int wn = (wid % WAVES_N) * 64;
  const int wm = (wid / WAVES_N) * (32 * TM);
  const int l32 = lane & 31;
  const int lhi = lane >> 5;

  // MEAN: the members' outputs summed in member order, (o0 + o1) + o2
  float msum[TM][TN][MEAN ? 16 : 1];

#pragma unroll 1
  for (int br = 0; br < (MEAN ? G.n : 1); ++br) {
    const vits_resblock_pair_desc& p = G.d[MEAN ? br : gi];
    const int k = p.k;
    const int dil = p.dil;
    const int p1 = (k - 1) * dil / 2;
    const int p2 = (k - 1) / 2;
    // interior tile (block-uniform): the staged window inside [0, Tn) and
    // every gate column - hence every stored one - inside [0, L)
    const int tw0 = n0 - p2 - p1;  // time of window column 0
    const int xstart = tw0 & ~3;   // 16-byte aligned block start
    const int xcols = rp_xcols(NG, k, dil);
    const bool interior = xstart >= 0 && xstart + xcols <= Tn && n0 - p2 + NG <= L;
    if (MEAN && br > 0) __syncthreads();  // the previous member's erow / G reads are done

    {
      const float* cond = p.cond ? p.cond + (int64_t)b * p.cond_bstride : nullptr;
      for (int r = tid; r < 2 * C; r += NT) {
        float e = 0.f;
        if (r < C) {
          const int idx = (r & 1) ? H + (r >> 1) : (r >> 1);
          if (p.b1) e = p.b1[idx];
          if (cond) e += cond[idx];
        } else if (p.b2) {
          e = p.b2[r - C];
        }
        erow[r] = e;
      }
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // six products per fragment pair, small terms first (conv1d_impl.h's
    // F32P order: bitwise the conv's sums)
    auto mma = [&](av_t (*a)[TM], const av_t* bh, const av_t* bm, const av_t* bl) {
#pragma unroll
      for (int mi = 0; mi < TM; ++mi)
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          f32x16 c = acc[mi][ni];
          if constexpr (MODE == 0) {
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][mi], bl[ni], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2][mi], bh[ni], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][mi], bm[ni], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][mi], bm[ni], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][mi], bh[ni], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][mi], bh[ni], c, 0, 0, 0);
          } else if constexpr (MODE == 1) {
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][mi], bh[ni], c, 0, 0, 0);
          } else {
            c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0][mi], bh[ni], c, 0, 0, 0);
          }
          acc[mi][ni] = c;
        }
    };
    // A fragments of flat step s (image [cin_pad/16][k][2][NPL][m_pad][8]):
    // plane q, half lhi, rows wm + mi * 32 + l32.  The step, plane and row
    // base are wave-uniform (a scalar address); the lane adds one 32-bit byte
    // offset `al` (half and row: far below 2^32), so no 64-bit per-plane
    // address lives in vector registers across the k-loop.
    auto loadA = [&](const lt* w, uint32_t al, int64_t wstep, int m_pad, int s, int total,
                     av_t (*a)[TM]) {
      const lt* wp = w + (int64_t)(s < total ? s : total - 1) * wstep + (int64_t)wm * 8;
      // (the copy keeps the offset's zero-extension beside the loads, where
      // it folds into their scalar-base addressing)
      const uint32_t av = REMAT ? rp_fresh(al) : al;
#pragma unroll
      for (int q = 0; q < NPL; ++q)
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
          if constexpr (REMAT)
            a[q][mi] = *reinterpret_cast<const av_t*>(
                reinterpret_cast<const char*>(rp_sbase(wp + ((int64_t)q * m_pad + mi * 32) * 8)) +
                av);
          else
            a[q][mi] = *reinterpret_cast<const av_t*>(
                reinterpret_cast<const char*>(wp + ((int64_t)q * m_pad + mi * 32) * 8) + av);
    };

    av_t a0[NPL][TM], a1[NPL][TM];
    av_t bh0[TN], bm0[NB], bl0[NB], bh1[TN], bm1[NB], bl1[NB];

    // ---------------- phase 1: c1 over NG columns from n0 - p2 ---------------
    const xt* xb = reinterpret_cast<const xt*>(p.x) + (int64_t)b * p.x_bstride;
    {
      const int xsh = tw0 - xstart;  // window column c sits at LDS row c + xsh
      const int nunits = (KC / 4) * (xcols >> 2);  // channel quads x 4-step blocks
      const int xpl = xcols * KCP;   // plane (elements)
      lt* const xbuf0 = reg;
      lt* const xbuf1 = reg + NPL * xpl;
      const float slope = p.in_slope;
      // unit u: channel quad u % (KC/4), 4-step block u / (KC/4) (a 16-lane
      // group's 8-byte LDS pieces fall on distinct banks)
      // (xoff: bytes where KC rows of bytes stay below 2^32 given the host's
      // C * cstride < 2^31 - one 32-bit lane offset on a scalar row address;
      // else elements)
      constexpr bool XB = KC * sizeof(xt) <= 2 * C;
      constexpr uint32_t XU = XB ? (uint32_t)sizeof(xt) : 1u;
      xt4 xr[NU][4];
      uint32_t xoff[NU];
      bool xok[NU];
#pragma unroll
      for (int q = 0; q < NU; ++q) {
        const int u = tid + NT * q;
        const int tt = xstart + 4 * (u / (KC / 4));
        xok[q] = u < nunits && tt >= 0 && tt < Tn;  // T % 4 == 0: a block is all in or out
        xoff[q] = xok[q] ? (uint32_t)(4 * (u % (KC / 4)) * p.x_cstride + tt) * XU : 0;
      }
      // loads issued unconditionally (a block outside reads the chunk's first
      // columns - offset 0, always inside the tensor - and is zeroed in lstore)
      auto gload = [&](int ch) __attribute__((always_inline)) {
        const xt* base = xb + (int64_t)ch * KC * p.x_cstride;
#pragma unroll
        for (int q = 0; q < NU; ++q) {
          if (q * NT < nunits) {
            const uint32_t xo = REMAT ? rp_fresh(xoff[q]) : xoff[q];  // (as loadA's)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const xt* row = base + (int64_t)i * p.x_cstride;
              if constexpr (REMAT) row = rp_sbase(row);
              xr[q][i] = *reinterpret_cast<const xt4*>(reinterpret_cast<const char*>(row) +
                                                       (size_t)xo * (sizeof(xt) / XU));
            }
          }
        }
      };
      // interior tiles with 0 < slope < 1: no validity select, and lrelu as
      // max(t, t * slope) - exact there (t >= 0: t * slope <= t; t < 0: t * slope
      // >= t, equal only where both are the same -0).  Any other tile or slope:
      // the compare form.
      const bool xfast = interior && slope > 0.f && slope < 1.f;
      auto lstore_as = [&](lt* xs, auto edge) __attribute__((always_inline)) {
        const int ftid = REMAT ? rp_fresh(tid) : tid;
#pragma unroll
        for (int q = 0; q < NU; ++q) {
          const int u = ftid + NT * q;
          if (q * NT < nunits && u < nunits) {
            f32x4v v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                float t = (float)xr[q][i][e];
                if constexpr (decltype(edge)::value) {
                  t = t < 0.f ? t * slope : t;
                  v[i][e] = xok[q] ? t : 0.f;
                } else {
                  v[i][e] = rp_max(t, t * slope);
                }
              }
            lt* xh = xs + 4 * (u / (KC / 4)) * KCP + 4 * (u % (KC / 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const f32x4v w = {v[0][e], v[1][e], v[2][e], v[3][e]};
              if constexpr (NPL == 3) {
                bf16x4 h4, m4, l4;
                split3_bf16x4(w, h4, m4, l4);
                *reinterpret_cast<bf16x4*>(xh + e * KCP) = h4;
                *reinterpret_cast<bf16x4*>(xh + xpl + e * KCP) = m4;
                *reinterpret_cast<bf16x4*>(xh + 2 * xpl + e * KCP) = l4;
              } else {
                lt4 w4;
#pragma unroll
                for (int i = 0; i < 4; ++i) w4[i] = (lt)w[i];
                *reinterpret_cast<lt4*>(xh + e * KCP) = w4;
              }
            }
          }
        }
      };
      auto lstore = [&](lt* xs) __attribute__((always_inline)) {
        if (xfast)
          lstore_as(xs, interior_t());
        else
          lstore_as(xs, edge_t());
      };
      // B fragments of tap j, slab g of the chunk: rows wn + ni * 32 + l32 +
      // j * dil (+ xsh), channels 16 g + 8 lhi .. + 8 (two 8-byte reads per plane)
      auto loadB = [&](const lt* xs, int j, int g, av_t* bh, av_t* bm, av_t* bl) {
        const int P4 = xpl / 4;
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          const lt4* xp = reinterpret_cast<const lt4*>(
              xs + (wn + ni * 32 + l32 + j * dil + xsh) * KCP + 16 * g + 8 * lhi);
          bh[ni] = __builtin_shufflevector(xp[0], xp[1], 0, 1, 2, 3, 4, 5, 6, 7);
          if constexpr (NPL == 3) {
            bm[ni] = __builtin_shufflevector(xp[P4], xp[P4 + 1], 0, 1, 2, 3, 4, 5, 6, 7);
            bl[ni] = __builtin_shufflevector(xp[2 * P4], xp[2 * P4 + 1], 0, 1, 2, 3, 4, 5, 6, 7);
          }
        }
      };
      const lt* wl = reinterpret_cast<const lt*>(p.w1);
      const uint32_t al = (uint32_t)((lhi * NPL) * p.m_pad1 + l32) * (uint32_t)(8 * sizeof(lt));
      const int64_t wstep = (int64_t)16 * NPL * p.m_pad1;
      const int total = S1 * k;
      const int nst = (KC / 16) * k;  // k-steps per chunk: slab-major, then tap
      loadA(wl, al, wstep, p.m_pad1, 0, total, a0);
      gload(0);
      lstore(xbuf0);
      __syncthreads();
      for (int ch = 0; ch < C / KC; ++ch) {
        const bool more = ch + 1 < C / KC;
        if (more) gload(ch + 1);  // in flight under this chunk's MFMAs
        const lt* xs = (ch & 1) ? xbuf1 : xbuf0;
        const int s0 = ch * nst;
        int j = 0, g = 0;  // (tap, slab) of the next B load
        auto next = [&]() {
          if (++j == k) {
            j = 0;
            ++g;
          }
        };
        loadB(xs, 0, 0, bh0, bm0, bl0);
        int st = 0;
        // the loads of step st + 1 pinned ahead of step st's MFMAs
        for (; st + 2 <= nst; st += 2) {
          next();
          loadA(wl, al, wstep, p.m_pad1, s0 + st + 1, total, a1);
          loadB(xs, j, g, bh1, bm1, bl1);
          __builtin_amdgcn_sched_barrier(0);
          mma(a0, bh0, bm0, bl0);
          __builtin_amdgcn_sched_barrier(0);
          next();
          loadA(wl, al, wstep, p.m_pad1, s0 + st + 2, total, a0);
          if (st + 2 < nst) loadB(xs, j, g, bh0, bm0, bl0);
          __builtin_amdgcn_sched_barrier(0);
          mma(a1, bh1, bm1, bl1);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (st < nst) {  // odd step count: the last step, and the next chunk's A
          loadA(wl, al, wstep, p.m_pad1, s0 + nst, total, a1);
          __builtin_amdgcn_sched_barrier(0);
          mma(a0, bh0, bm0, bl0);
#pragma unroll
          for (int q = 0; q < NPL; ++q)
#pragma unroll
            for (int mi = 0; mi < TM; ++mi) a0[q][mi] = a1[q][mi];
        }
        if (more) lstore((ch & 1) ? xbuf0 : xbuf1);
        __syncthreads();
      }
    }

    // ---------------- gate -> G planes (over the dead X buffers) -------------
    lt* const gs = reg;
    // (edge tiles only: the `in` select that zeroes columns outside [0, L))
    auto gate = [&](auto edge) __attribute__((always_inline)) {
      const int flane = REMAT ? rp_fresh(lane) : lane;
      const int l32 = flane & 31, lhi = flane >> 5;
#pragma unroll
      for (int mi = 0; mi < TM; ++mi) {
        // the sub-tile's c1 bias + cond rows, read once for both column halves
        // (rows 4 lhi + 8 g .. + 3 of the 32: a_q, b_q, a_q+1, b_q+1)
        f32x4v er[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
          er[g] = *reinterpret_cast<const f32x4v*>(erow + wm + mi * 32 + 4 * lhi + 8 * g);
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          const int col = wn + ni * 32 + l32;
          const int t = n0 - p2 + col;
          const bool in = t >= 0 && t < L;
#pragma unroll
          for (int r = 0; r < 16; r += 4) {
            const int row = wm + mi * 32 + 4 * lhi + 8 * (r >> 2);
            const f32x4v e = er[r >> 2];
            float g0 = rp_gate(acc[mi][ni][r] + e[0], acc[mi][ni][r + 1] + e[1]);
            float g1 = rp_gate(acc[mi][ni][r + 2] + e[2], acc[mi][ni][r + 3] + e[3]);
            if constexpr (decltype(edge)::value) {
              g0 = in ? g0 : 0.f;
              g1 = in ? g1 : 0.f;
            }
            lt* gp = gs + col * GP + (row >> 1);
            if constexpr (NPL == 3) {
              const f32x4v w = {g0, g1, 0.f, 0.f};
              bf16x4 h4, m4, l4;
              split3_bf16x4(w, h4, m4, l4);
              *reinterpret_cast<bf16x2*>(gp) = __builtin_shufflevector(h4, h4, 0, 1);
              *reinterpret_cast<bf16x2*>(gp + GPL) = __builtin_shufflevector(m4, m4, 0, 1);
              *reinterpret_cast<bf16x2*>(gp + 2 * GPL) = __builtin_shufflevector(l4, l4, 0, 1);
            } else {
              lt2 v2;
              v2[0] = (lt)g0;
              v2[1] = (lt)g1;
              *reinterpret_cast<lt2*>(gp) = v2;
            }
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
        }
      }
    };
    if (interior)
      gate(interior_t());
    else
      gate(edge_t());
    // the 16 rows past NG that phase 2's discarded columns read: zero
    for (int i = tid; i < NPL * 16 * H; i += NT) {
      const int pl = i / (16 * H);
      const int e = i - pl * 16 * H;
      gs[pl * GPL + (NG + e / H) * GP + e % H] = (lt)0.f;
    }
    __syncthreads();

    // ---------------- phase 2: c2 from G --------------------------------------
    {
      const int flane = REMAT ? rp_fresh(lane) : lane;
      const int l32 = flane & 31, lhi = flane >> 5;
      const lt* wl = reinterpret_cast<const lt*>(p.w2);
      const uint32_t al = (uint32_t)((lhi * NPL) * p.m_pad2 + l32) * (uint32_t)(8 * sizeof(lt));
      const int64_t wstep = (int64_t)16 * NPL * p.m_pad2;
      const int total = S2 * k;
      const lt* gl = gs + (wn + l32) * GP + 8 * lhi;
      int j = 0, g = 0;  // tap / slab of the next B load
      auto loadB = [&](av_t* bh, av_t* bm, av_t* bl) {
        const lt* x = gl + j * GP + 16 * g;
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          bh[ni] = *reinterpret_cast<const av_t*>(x + ni * 32 * GP);
          if constexpr (NPL == 3) {
            bm[ni] = *reinterpret_cast<const av_t*>(x + ni * 32 * GP + GPL);
            bl[ni] = *reinterpret_cast<const av_t*>(x + ni * 32 * GP + 2 * GPL);
          }
        }
        if (++j == k) {
          j = 0;
          ++g;
        }
      };
      loadA(wl, al, wstep, p.m_pad2, 0, total, a0);
      loadB(bh0, bm0, bl0);
      int s = 0;
      for (; s + 2 <= total; s += 2) {
        loadA(wl, al, wstep, p.m_pad2, s + 1, total, a1);
        loadB(bh1, bm1, bl1);
        __builtin_amdgcn_sched_barrier(0);
        mma(a0, bh0, bm0, bl0);
        __builtin_amdgcn_sched_barrier(0);
        loadA(wl, al, wstep, p.m_pad2, s + 2, total, a0);
        if (s + 2 < total) loadB(bh0, bm0, bl0);
        __builtin_amdgcn_sched_barrier(0);
        mma(a1, bh1, bm1, bl1);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (s < total) mma(a0, bh0, bm0, bl0);
    }

    // residual (+ accumulate / branch-mean division) epilogue, as the conv's
    // single-output STORE: every load of a 32 x 32 sub-tile issued first
    // Row r of a sub-tile is wave-uniform but for 4 lhi: a scalar row base
    // plus one 32-bit lane offset (4 lhi rows + the column; the host checks
    // C * cstride < 2^31), no 64-bit multiply-add per element.  accumulate and
    // the division are branched on once per sub-tile; the length select runs
    // on edge tiles only.
    xt* const yb = reinterpret_cast<xt*>(p.y) + (int64_t)b * p.y_bstride;
    const bool accum = !MEAN && p.accumulate;
    const float div = MEAN ? (float)G.n : p.post_div;
    const bool last = !MEAN || br == G.n - 1;  // (MEAN: the member that stores)
    auto epilogue = [&](auto edge) __attribute__((always_inline)) {
      const int flane = REMAT ? rp_fresh(lane) : lane;
      const int l32 = flane & 31, lhi = flane >> 5;
#pragma unroll
      for (int mi = 0; mi < TM; ++mi) {
        const xt* const xrow = xb + (int64_t)(wm + mi * 32) * p.x_cstride;
        xt* const yrow = yb + (int64_t)(wm + mi * 32) * p.y_cstride;
        f32x4v e2[4];  // c2 bias rows 4 lhi + 8 g .. + 3
#pragma unroll
        for (int g = 0; g < 4; ++g)
          e2[g] = *reinterpret_cast<const f32x4v*>(erow + C + wm + mi * 32 + 4 * lhi + 8 * g);
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          const int col = wn + ni * 32 + l32;
          const int t = n0 + col;
          const bool st = decltype(edge)::value ? col < BN && t < Tn : col < BN;
          const int tc = st ? t : 0;
          // byte offsets (at most 5 rows: < 2^31 with C * cstride < 2^31, C >= 32)
          const uint32_t xv = (uint32_t)(4 * lhi * p.x_cstride + tc) * (uint32_t)sizeof(xt);
          const uint32_t yv = (uint32_t)(4 * lhi * p.y_cstride + tc) * (uint32_t)sizeof(xt);
          // element r: row (r & 3) + 8 (r >> 2) of the lane's four-row groups
          auto xat = [&](int r) __attribute__((always_inline)) -> const xt& {
            const xt* row = xrow + (int64_t)((r & 3) + 8 * (r >> 2)) * p.x_cstride;
            return *reinterpret_cast<const xt*>(reinterpret_cast<const char*>(row) + xv);
          };
          auto yat = [&](int r) __attribute__((always_inline)) -> xt& {
            xt* row = yrow + (int64_t)((r & 3) + 8 * (r >> 2)) * p.y_cstride;
            return *reinterpret_cast<xt*>(reinterpret_cast<char*>(row) + yv);
          };
          float o[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float rv = (float)xat(r);
            const float v = acc[mi][ni][r] + e2[r >> 2][r & 3];
            o[r] = rv + v;  // (the conv's rv + res_scale * v, res_scale 1)
          }
          if constexpr (MEAN) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              o[r] = br == 0 ? o[r] : msum[mi][ni][r] + o[r];
              msum[mi][ni][r] = o[r];
            }
          }
          if (accum) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
              o[r] = (float)yat(r) + o[r];
          }
          if (last) {
            if (div != 1.0f) {
#pragma unroll
              for (int r = 0; r < 16; ++r) o[r] = o[r] / div;
            }
            if (st) {
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                if constexpr (decltype(edge)::value) o[r] = t < L ? o[r] : 0.f;
                yat(r) = (xt)o[r];
              }
            }
          }
        }
      }
    };
    if (interior)
      epilogue(interior_t());
    else
      epilogue(edge_t());
  }  // br
}

template <int C, int MODE = 0, bool MEAN = false, int TM = rp_tm(C, MODE)>
int rp_launch(const RpGroup& g, hipStream_t s) {
  int lds = 0, gx = 0;
  for (int i = 0; i < g.n; ++i) {
    const vits_resblock_pair_desc& d = g.d[i];
    const int l = rp_lds_bytes(C, d.k, d.dil, MODE);
    if (l > lds) lds = l;
    const int BN = MEAN ? g.bn : rp_ng(C) - (d.k - 1);
    const int x = (d.t_len + BN - 1) / BN;
    if (x > gx) gx = x;
  }
  if (lds > 160 * 1024) return VITS_E_UNSUP;
  hipLaunchKernelGGL((resblock_f32p_kernel<C, MODE, MEAN, TM>),
                     dim3(gx, 1, MEAN ? g.batch : g.n * g.batch), dim3(rp_threads(C, TM)), lds, s,
                     g);
  return vits_launch_status();
}

int rp_check(const vits_resblock_pair_desc& d, int mode = 0) {
  VITS_CHECK_ARG(d.x && d.w1 && d.w2 && d.y);
  // other workgroups still read x (halos, residual): never write in place
  VITS_CHECK_ARG(reinterpret_cast<const void*>(d.y) != reinterpret_cast<const void*>(d.x));
  VITS_CHECK_SHAPE(d.channels == 32 || d.channels == 64 || d.channels == 128 ||
                   d.channels == 256);
  VITS_CHECK_SHAPE(d.k >= 1 && d.k <= 15 && (d.k & 1) == 1 && d.dil >= 1 && d.t_len > 0);
  VITS_CHECK_SHAPE((d.k - 1) * d.dil <= 96);  // window within the staging units
  // images [cin_pad/16][k][2][3][m_pad][8] bf16, rows = C (c1 gate-interleaved / c2)
  VITS_CHECK_SHAPE(d.m_pad1 >= d.channels && d.m_pad2 >= d.channels && (d.m_pad1 & 3) == 0 &&
                   (d.m_pad2 & 3) == 0);
  VITS_CHECK_SHAPE(d.cin_pad1 >= d.channels && d.cin_pad2 >= d.channels / 2);
  // 4-step x staging (16 bytes fp32 / 8 bytes 16-bit): time-contiguous rows,
  // T % 4 == 0, aligned
  VITS_CHECK_SHAPE((d.t_len & 3) == 0 && (d.x_cstride & 3) == 0 && (d.x_bstride & 3) == 0 &&
                   d.x_cstride >= d.t_len && d.y_cstride >= d.t_len &&
                   (reinterpret_cast<uintptr_t>(d.x) & (mode ? 7 : 15)) == 0);
  // 32-bit staging offsets within one utterance
  VITS_CHECK_SHAPE((int64_t)d.channels * d.x_cstride < (1LL << 31));
  // (and the epilogue's 32-bit lane offsets into y)
  VITS_CHECK_SHAPE((int64_t)d.channels * d.y_cstride < (1LL << 31));
  VITS_CHECK_SHAPE((reinterpret_cast<uintptr_t>(d.w1) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(d.w2) & 15) == 0);
  return VITS_OK;
}

}  // namespace

// the 16-bit models' 256-channel pairs (vits_resblock_pair16_forward routes
// them here: resblock16.hip stages whole windows, which a 256-channel window
// does not fit)
int vits_rp16_256(const vits_resblock_pair_desc* d, int n, int batch, int wdtype,
                  hipStream_t s) {
  if (!d || n < 1 || n > RP_GROUP || batch < 1) return VITS_E_ARG;
  if (wdtype != VITS_WDT_BF16 && wdtype != VITS_WDT_F16) return VITS_E_ARG;
  const int mode = wdtype == VITS_WDT_BF16 ? 1 : 2;
  RpGroup g;
  g.n = n;
  g.batch = batch;
  g.bn = 0;
  for (int i = 0; i < n; ++i) {
    const int rc = rp_check(d[i], mode);
    if (rc) return rc;
    if (d[i].channels != d[0].channels) return VITS_E_SHAPE;
    g.d[i] = d[i];
  }
  if (d[0].channels != 256) return VITS_E_SHAPE;
  return mode == 1 ? rp_launch<256, 1>(g, s) : rp_launch<256, 2>(g, s);
}

extern "C" int vits_resblock_pair_f32p_forward(const vits_resblock_pair_desc* d, int n, int batch,
                                               void* stream) {
  if (!d || n < 1 || n > RP_GROUP || batch < 1) return VITS_E_ARG;
  RpGroup g;
  g.n = n;
  g.batch = batch;
  g.bn = 0;
  for (int i = 0; i < n; ++i) {
    const int rc = rp_check(d[i]);
    if (rc) return rc;
    if (d[i].channels != d[0].channels) return VITS_E_SHAPE;
    g.d[i] = d[i];
  }
  hipStream_t s = as_stream(stream);
  int rc;
  if (d[0].channels == 32)
    rc = rp_launch<32>(g, s);
  else if (d[0].channels == 64)
    rc = rp_launch<64>(g, s);
  else if (d[0].channels == 128)
    rc = rp_launch<128>(g, s);
  else
    rc = rp_launch<256>(g, s);
  return count_ok(rc, VITS_CNT_RESBLOCK);
}

// the branch mean of the 32-channel stage as one launch (the kernel's MEAN
// form; wider stages keep the accumulating launches: the 16-bit kernel's
// 64-channel mean reached 256 VGPRs and lost, and this one is not measured)
extern "C" int vits_resblock_pair_f32p_mean_forward(const vits_resblock_pair_desc* d, int n,
                                                    int batch, void* stream) {
  if (!d || n < 1 || n > RP_GROUP || batch < 1) return VITS_E_ARG;
  RpGroup g;
  g.n = n;
  g.batch = batch;
  int kmax = 1;
  for (int i = 0; i < n; ++i) {
    const int rc = rp_check(d[i]);
    if (rc) return rc;
    VITS_CHECK_SHAPE(d[i].channels == 32);
    // one output tile per workgroup over every member: the same time axis,
    // utterance lengths and output, and no member's input is the output
    VITS_CHECK_SHAPE(d[i].t_len == d[0].t_len && d[i].lengths == d[0].lengths &&
                     d[i].len_skip == d[0].len_skip && d[i].y == d[0].y &&
                     d[i].y_bstride == d[0].y_bstride && d[i].y_cstride == d[0].y_cstride);
    VITS_CHECK_ARG(reinterpret_cast<const void*>(d[0].y) != reinterpret_cast<const void*>(d[i].x));
    if (d[i].k > kmax) kmax = d[i].k;
    g.d[i] = d[i];
  }
  g.bn = rp_ng(32) - (kmax - 1);
  return count_ok(rp_launch<32, 0, true>(g, as_stream(stream)), VITS_CNT_RESBLOCK);
}
