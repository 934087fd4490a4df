// mas_long.hip — monotonic alignment search of long recordings on gfx950:
// the DP and backtrack of mas.hip (see its header: the same -1e9 boundaries,
// the same Cython max, the same decision V[y-1][x] < V[y-1][x-1]) over a
// score matrix that never exists as a whole.  The matrix arrives in panels of
// `panel` frames (a multiple of 32) by all t_s tokens, in increasing y0, and
// a panel's row is cut into strips of `strip` = 64 * XPL tokens.
//
//   vits_mas_long_panel      forward step of one panel: one workgroup per
//                            recording runs the strips left to right.  Wave 0
//                            runs a strip's rows exactly like mas_kernel
//                            (registers, one DPP shift, a decision word per
//                            column stored once per 32 rows), waves 1-3 stream
//                            the rows into the LDS ring.  Lane 0's left
//                            neighbour V[y-1][x0-1] comes from the strip to
//                            the left through an LDS column buffer (two of
//                            them, alternating).  Between panels the carry
//                            row V[y0-1][.] lives in the workspace twice: a
//                            panel reads the half of its parity and writes the
//                            other, so strip s still reads the old
//                            V[y0-1][x0-1] after strip s-1 wrote its carry.
//   vits_mas_long_backtrack  the backtrack over the global decision words
//                            (mas_kernel's block scheme; the next block's 64
//                            candidate words are loaded while this block is
//                            walked: the index drops by at most 32 a block).
//                            frame_token and the token starts go to the
//                            workspace, durations are differences of starts.
//   vits_mas_long_gather     second sweep: val[y] = panel[y][frame_token[y]].
//   vits_mas_long_scores     per token the fp32 sum of val over its frames in
//                            increasing y (__fadd_rn from 0), val staged
//                            through LDS in windows: the DUR epilogue's sums.
//
// The calls depend on each other through stream order only: no workgroup
// waits on another, no flags, no atomics; every store is a vector store.
#include "common.h"

namespace {

constexpr int ML_RING_BYTES = 64 * 1024;
__host__ __device__ inline int ml_rows(int xpl) {
  int r = ML_RING_BYTES / (2 * 64 * xpl * (int)sizeof(float));
  return r > 64 ? 64 : (r < 4 ? 4 : r);
}
constexpr float ML_NEG = -1e9f;
constexpr int ML_COL_SLACK = 4;     // the DP reads the column buffer 2 rows ahead
constexpr int ML_VAL_WINDOW = 8192; // frames per LDS window of the score sums
constexpr int ML_LDS_MAX = 160 * 1024;

// workspace sections (each rounded up to 256 bytes), in this order
struct MlLayout {
  int Ws;        // padded width: ceil(t_s / strip) * strip
  int nblk;      // ceil(t_t / 32)
  int64_t carry; // float    [2][B][Ws]
  int64_t words; // uint32_t [B][nblk][Ws]
  int64_t ftok;  // int32_t  [B][t_t]
  int64_t start; // int32_t  [B][Ws + 1]
  int64_t val;   // float    [B][t_t]
  int64_t total;
};

inline int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }

inline bool ml_strip_ok(int strip) {
  if (strip < 64 || strip > 2048 || (strip & 63)) return false;
  const int xpl = strip / 64;
  return (xpl & (xpl - 1)) == 0;
}

inline size_t ml_panel_lds(int strip, int panel) {
  const int xpl = strip / 64;
  return sizeof(float) * ((size_t)2 * ml_rows(xpl) * strip + 3 * (size_t)strip +
                          2 * ((size_t)panel + ML_COL_SLACK));
}

// 0 = fine, else the error code
inline int ml_layout(int batch, int t_t, int t_s, int strip, int panel, MlLayout* L) {
  if (batch <= 0 || t_t <= 0 || t_s <= 0 || strip <= 0 || panel <= 0) return VITS_E_ARG;
  if (panel & 31) return VITS_E_ARG;
  if (!ml_strip_ok(strip)) return VITS_E_ARG;
  if (ml_panel_lds(strip, panel) > (size_t)ML_LDS_MAX) return VITS_E_UNSUP;
  const int64_t nstr = ((int64_t)t_s + strip - 1) / strip;
  if (nstr * strip > (int64_t)1 << 30) return VITS_E_UNSUP;
  L->Ws = (int)(nstr * strip);
  L->nblk = (t_t + 31) / 32;
  int64_t off = 0;
  L->carry = off;
  off += up256((int64_t)sizeof(float) * 2 * batch * L->Ws);
  L->words = off;
  off += up256((int64_t)sizeof(uint32_t) * batch * L->nblk * L->Ws);
  L->ftok = off;
  off += up256((int64_t)sizeof(int32_t) * batch * t_t);
  L->start = off;
  off += up256((int64_t)sizeof(int32_t) * batch * (L->Ws + 1));
  L->val = off;
  off += up256((int64_t)sizeof(float) * batch * t_t);
  L->total = off;
  return VITS_OK;
}

// the row's lengths, clamped; false = no alignment
__device__ __forceinline__ bool ml_lengths(const int32_t* tt_len, const int32_t* ts_len, int b,
                                           int T_t, int T_s, int& t_t, int& t_s) {
  t_t = tt_len[b];
  t_s = ts_len[b];
  t_t = t_t < 0 ? 0 : (t_t > T_t ? T_t : t_t);
  t_s = t_s < 0 ? 0 : (t_s > T_s ? T_s : t_s);
  return t_t > 0 && t_s > 0 && t_t >= t_s;
}

// nc: rows y0 .. y0 + rows of the score matrix, [B][rows][T_s] at nc_bstride
// elements per recording.  carry_in / carry_out [B][Ws], words [B][nblk][Ws].
template <int XPL>
__global__ __launch_bounds__(256) void mas_long_panel_kernel(
    const float* __restrict__ nc_all, int64_t nc_bstride, const int32_t* __restrict__ tt_len,
    const int32_t* __restrict__ ts_len, int T_t, int T_s, int Ws, int nblk, int panel, int y0,
    int rows, const float* __restrict__ carry_in, float* __restrict__ carry_out,
    uint32_t* __restrict__ words) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  constexpr int W = 64 * XPL;  // strip width
  const int R = ml_rows(XPL);
  float* ring = reinterpret_cast<float*>(smem_raw);  // [2][R][W] + 3 rows of slack
  float* colbuf = ring + 2 * R * W + 3 * W;          // [2][panel + ML_COL_SLACK]
  const int colw = panel + ML_COL_SLACK;

  int t_t, t_s;
  if (!ml_lengths(tt_len, ts_len, b, T_t, T_s, t_t, t_s)) return;
  const int yend = min(t_t, y0 + rows);
  if (yend <= y0) return;  // the row's frames ended before this panel
  const int nrows = yend - y0;
  const int nstr = (t_s + W - 1) / W;  // strips past t_s do nothing
  const int nch = (nrows + R - 1) / R;
  const int total = nstr * nch;

  const float* nc = nc_all + (int64_t)b * nc_bstride;
  carry_in += (int64_t)b * Ws;
  carry_out += (int64_t)b * Ws;
  words += (int64_t)b * nblk * Ws;

  // (strip, chunk) pairs form one sequence q; chunk q lives in ring buffer
  // q & 1, so the next strip's first chunk streams in behind this strip's
  // last.  Columns >= T_s and rows >= rows read clamped in-bounds addresses:
  // the DP never uses them.
  auto load_chunk = [&](int q, int w0, int nw) {
    const int s = q / nch;
    const int r0 = (q - s * nch) * R;
    const int x0 = s * W;
    float* dst = ring + (q & 1) * R * W;
    const int pieces = R * XPL;  // 64 floats each
    for (int p = (tid >> 6) - w0; p < pieces; p += nw) {
      const int r = p / XPL;
      const int x = x0 + (p - r * XPL) * 64 + (tid & 63);
      const int yl = min(r0 + r, rows - 1);
      const int xc = min(x, T_s - 1);
      __builtin_amdgcn_global_load_lds(nc + (int64_t)yl * T_s + xc,
                                       (__attribute__((address_space(3))) void*)(dst + p * 64), 4,
                                       0, 0);
    }
  };

  load_chunk(0, 0, 4);
  __syncthreads();

  float vp[XPL];
  uint32_t dw[XPL];
  int xs[XPL];
  const int D = t_t - t_s;  // >= 0 here
  const uint32_t Du = (uint32_t)D;
  const int xbase = lane * XPL;
  int x0 = 0;
  const float* cin = colbuf;
  float* cout = colbuf;
#pragma unroll
  for (int i = 0; i < XPL; ++i) {
    vp[i] = 0.f;
    dw[i] = 0u;
    xs[i] = 0x40000000;
  }

  for (int q = 0; q < total; ++q) {
    if (wid != 0) {
      if (q + 1 < total) load_chunk(q + 1, 1, 3);
    } else {
      const int s = q / nch;
      const int ch = q - s * nch;
      if (ch == 0) {
        // a new strip: V[y0-1][.] of its columns from the carry, the column
        // buffers swap roles
        x0 = s * W;
        cin = colbuf + ((s + 1) & 1) * colw;
        cout = colbuf + (s & 1) * colw;
#pragma unroll
        for (int i = 0; i < XPL; ++i) {
          const int x = x0 + xbase + i;
          vp[i] = y0 > 0 ? carry_in[x] : 0.f;
          dw[i] = 0u;
          xs[i] = x < t_s ? x : 0x40000000;
        }
        if (lane == 63) cout[0] = vp[XPL - 1];  // V[y0-1][x0 + W - 1]
      }
      const float* rowsp = ring + (q & 1) * R * W;
      const int yc0 = y0 + ch * R;
      const int ycend = min(yend, yc0 + R);
      float ra[XPL], rb[XPL];
      float ba, bb;  // the left boundary of lane 0 at rows y, y + 1
      auto rd = [&](float* r, float& bnd, int y) {
        const float* src = rowsp + (y - yc0) * W + xbase;
#pragma unroll
        for (int i = 0; i < XPL; ++i) r[i] = src[i];
        // V[y-1][x0-1]: the DP's own boundary left of column 0, else what the
        // strip to the left stored for row y - 1 (entry y - y0 of its buffer)
        bnd = s == 0 ? (y == 0 ? 0.f : ML_NEG) : cin[y - y0];
      };
      auto row = [&](int y, const float* cur, float bnd) {
        const float left = __int_as_float(__builtin_amdgcn_update_dpp(
            __float_as_int(bnd), __float_as_int(vp[XPL - 1]), 0x138, 0xf, 0xf, false));
        const uint32_t bit = 1u << (y & 31);
        float vn[XPL];
#pragma unroll
        for (int i = 0; i < XPL; ++i) {
          const float vcur_raw = vp[i];
          const float vprev_raw = (i == 0) ? left : vp[i - 1];
          dw[i] |= (vcur_raw < vprev_raw) ? bit : 0u;
          const uint32_t dy = (uint32_t)(y - xs[i]);
          const float v_cur = dy == 0u ? ML_NEG : vcur_raw;          // x == y
          const float mx = (v_cur > vprev_raw) ? v_cur : vprev_raw;  // Cython max(v_prev, v_cur)
          const float upd = cur[i] + mx;
          vn[i] = dy <= Du ? upd : cur[i];
        }
#pragma unroll
        for (int i = 0; i < XPL; ++i) vp[i] = vn[i];
        if (lane == 63) cout[y - y0 + 1] = vn[XPL - 1];  // V[y][x0 + W - 1]
        if ((y & 31) == 31 || y == yend - 1) {  // block of 32 rows complete
#pragma unroll
          for (int i = 0; i < XPL; ++i) {
            words[(int64_t)(y >> 5) * Ws + x0 + xbase + i] = dw[i];
            dw[i] = 0u;
          }
        }
      };
      rd(ra, ba, yc0);
      rd(rb, bb, yc0 + 1);
      for (int y = yc0; y < ycend; y += 2) {
        row(y, ra, ba);
        rd(ra, ba, y + 2);
        if (y + 1 < ycend) {
          row(y + 1, rb, bb);
          rd(rb, bb, y + 3);
        }
      }
      if (ch == nch - 1) {
#pragma unroll
        for (int i = 0; i < XPL; ++i) carry_out[x0 + xbase + i] = vp[i];
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void mas_long_backtrack_kernel(
    const int32_t* __restrict__ tt_len, const int32_t* __restrict__ ts_len, int T_t, int T_s,
    int Ws, int nblk, const uint32_t* __restrict__ words, int32_t* ftok, int32_t* start,
    int32_t* __restrict__ durations, int32_t* __restrict__ frame_token) {
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  int t_t, t_s;
  const bool aligned = ml_lengths(tt_len, ts_len, b, T_t, T_s, t_t, t_s);
  if (!aligned) t_t = 0;
  words += (int64_t)b * nblk * Ws;
  ftok += (int64_t)b * T_t;
  start += (int64_t)b * (Ws + 1);
  if (frame_token) frame_token += (int64_t)b * T_t;

  if (wid == 0 && aligned) {
    int index = t_s - 1;
    const int blk_top = (t_t - 1) >> 5;
    // lane l holds the decision word of column base - l.  The words of block
    // blk - 1 are loaded at the top of block blk with base = the index there:
    // the index drops by at most 32 in a block, so the 32 columns block
    // blk - 1 can consult lie within 64 of it.
    int base_next = index;
    uint32_t w_next = (index - lane >= 0) ? words[(int64_t)blk_top * Ws + index - lane] : 0u;
    for (int blk = blk_top; blk >= 0; --blk) {
      const int base = base_next;
      const uint32_t wv = w_next;
      if (blk > 0) {
        base_next = index;
        w_next = (index - lane >= 0) ? words[(int64_t)(blk - 1) * Ws + index - lane] : 0u;
      }
      const int yhi = min(t_t - 1, blk * 32 + 31);
      int my_idx = 0;       // lane l: the path column of row 32 * blk + l
      bool my_st = false;   // ... and whether that row is the column's first
      for (int y = yhi; y >= blk * 32; --y) {
        const bool sel = lane == (y & 31);
        my_idx = sel ? index : my_idx;
        bool dec = false;
        if (index != 0) {
          dec = (index == y);
          if (!dec && y >= 1) {
            const uint32_t w = __builtin_amdgcn_readlane(wv, base - index);
            dec = (w >> (y & 31)) & 1u;
          }
        }
        my_st = sel ? dec : my_st;
        if (dec) index = index - 1;
      }
      const int y = blk * 32 + lane;
      if (lane < 32 && y <= yhi) {
        ftok[y] = my_idx;
        if (frame_token) frame_token[y] = my_idx;
        if (my_st) start[my_idx] = y;  // the one frame where the column becomes my_idx
      }
    }
    if (lane == 0) {
      start[0] = 0;
      start[t_s] = t_t;
    }
  }
  __syncthreads();
  const int64_t obase = (int64_t)b * T_s;
  for (int x = tid; x < T_s; x += 256)
    durations[obase + x] = (aligned && x < t_s) ? start[x + 1] - start[x] : 0;
  if (frame_token)
    for (int y = t_t + tid; y < T_t; y += 256) frame_token[y] = -1;
}

__global__ __launch_bounds__(256) void mas_long_gather_kernel(
    const float* __restrict__ nc_all, int64_t nc_bstride, const int32_t* __restrict__ tt_len,
    const int32_t* __restrict__ ts_len, int T_t, int T_s, int y0, int rows,
    const int32_t* __restrict__ ftok, float* __restrict__ val) {
  const int b = blockIdx.y;
  int t_t, t_s;
  if (!ml_lengths(tt_len, ts_len, b, T_t, T_s, t_t, t_s)) return;
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int y = y0 + r;
  if (r >= rows || y >= t_t) return;
  const int x = ftok[(int64_t)b * T_t + y];
  val[(int64_t)b * T_t + y] = nc_all[(int64_t)b * nc_bstride + (int64_t)r * T_s + x];
}

__global__ __launch_bounds__(256) void mas_long_scores_kernel(
    const int32_t* __restrict__ tt_len, const int32_t* __restrict__ ts_len, int T_t, int T_s,
    int Ws, const int32_t* __restrict__ ftok, const int32_t* __restrict__ start,
    const float* __restrict__ val, float* scores) {
  __shared__ float win[ML_VAL_WINDOW];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  int t_t, t_s;
  const bool aligned = ml_lengths(tt_len, ts_len, b, T_t, T_s, t_t, t_s);
  scores += (int64_t)b * T_s;
  if (!aligned) {
    for (int x = tid; x < T_s; x += 256) scores[x] = 0.f;
    return;
  }
  for (int x = t_s + tid; x < T_s; x += 256) scores[x] = 0.f;
  ftok += (int64_t)b * T_t;
  start += (int64_t)b * (Ws + 1);
  val += (int64_t)b * T_t;
  for (int c0 = 0; c0 < t_t; c0 += ML_VAL_WINDOW) {
    const int c1 = min(t_t, c0 + ML_VAL_WINDOW);
    for (int y = c0 + tid; y < c1; y += 256) win[y - c0] = val[y];
    __syncthreads();
    // the window's tokens are ftok[c0] .. ftok[c1 - 1]; token x is always
    // thread x mod 256's, so a token that crosses windows re-reads its own
    // partial sum
    const int x_lo = ftok[c0], x_hi = ftok[c1 - 1];
    for (int x = x_lo + ((tid - x_lo) & 255); x <= x_hi; x += 256) {
      const int s0 = start[x], s1 = start[x + 1];
      float acc = s0 >= c0 ? 0.f : scores[x];
      const int ya = max(s0, c0), yb = min(s1, c1);
      for (int y = ya; y < yb; ++y) acc = __fadd_rn(acc, win[y - c0]);
      scores[x] = acc;
    }
    __syncthreads();
  }
}

struct MlCall {
  MlLayout L;
  char* ws;
};

int ml_check(const int32_t* tt, const int32_t* ts, int batch, int t_t, int t_s, int strip,
             int panel, void* workspace, int64_t ws_bytes, MlCall* c) {
  VITS_CHECK_ARG(tt && ts && workspace);
  const int rc = ml_layout(batch, t_t, t_s, strip, panel, &c->L);
  if (rc) return rc;
  VITS_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ws_bytes >= c->L.total);
  c->ws = reinterpret_cast<char*>(workspace);
  return VITS_OK;
}

int ml_check_panel(int t_t, int panel, int y0, int rows) {
  VITS_CHECK_ARG(y0 >= 0 && y0 % panel == 0 && y0 < t_t);
  VITS_CHECK_ARG(rows >= 1 && rows <= panel && rows <= t_t - y0);
  // a short panel is the last one: a decision word belongs to one panel
  VITS_CHECK_ARG(rows == panel || y0 + rows == t_t);
  return VITS_OK;
}

}  // namespace

extern "C" int64_t vits_mas_long_workspace(int batch, int t_t, int t_s, int strip, int panel) {
  MlLayout L;
  if (ml_layout(batch, t_t, t_s, strip, panel, &L)) return 0;
  return L.total;
}

extern "C" int vits_mas_long_panel(const float* scores, int64_t batch_stride,
                                   const int32_t* t_t_len, const int32_t* t_s_len, int batch,
                                   int t_t, int t_s, int strip, int panel, int y0, int rows,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
  VITS_CHECK_ARG(scores != nullptr);
  MlCall c;
  int rc = ml_check(t_t_len, t_s_len, batch, t_t, t_s, strip, panel, workspace, workspace_bytes,
                    &c);
  if (rc) return rc;
  rc = ml_check_panel(t_t, panel, y0, rows);
  if (rc) return rc;
  VITS_CHECK_ARG(batch_stride >= (int64_t)rows * t_s);
  const int par = (y0 / panel) & 1;
  float* carry = reinterpret_cast<float*>(c.ws + c.L.carry);
  const float* cin = carry + (int64_t)par * batch * c.L.Ws;
  float* cout = carry + (int64_t)(par ^ 1) * batch * c.L.Ws;
  uint32_t* words = reinterpret_cast<uint32_t*>(c.ws + c.L.words);
  const size_t lds = ml_panel_lds(strip, panel);
  hipStream_t s = as_stream(stream);
#define ML_CASE(X)                                                                              \
  case X:                                                                                       \
    hipLaunchKernelGGL((mas_long_panel_kernel<X>), dim3(batch), dim3(256), lds, s, scores,      \
                       batch_stride, t_t_len, t_s_len, t_t, t_s, c.L.Ws, c.L.nblk, panel, y0,   \
                       rows, cin, cout, words);                                                 \
    break;
  switch (strip / 64) {
    ML_CASE(1)
    ML_CASE(2)
    ML_CASE(4)
    ML_CASE(8)
    ML_CASE(16)
    ML_CASE(32)
    default:
      return VITS_E_UNSUP;
  }
#undef ML_CASE
  return vits_launch_status();
}

extern "C" int vits_mas_long_backtrack(const int32_t* t_t_len, const int32_t* t_s_len,
                                       int32_t* durations, int32_t* frame_token, int batch,
                                       int t_t, int t_s, int strip, int panel, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  VITS_CHECK_ARG(durations != nullptr);
  MlCall c;
  const int rc = ml_check(t_t_len, t_s_len, batch, t_t, t_s, strip, panel, workspace,
                          workspace_bytes, &c);
  if (rc) return rc;
  hipLaunchKernelGGL(mas_long_backtrack_kernel, dim3(batch), dim3(256), 0, as_stream(stream),
                     t_t_len, t_s_len, t_t, t_s, c.L.Ws, c.L.nblk,
                     reinterpret_cast<const uint32_t*>(c.ws + c.L.words),
                     reinterpret_cast<int32_t*>(c.ws + c.L.ftok),
                     reinterpret_cast<int32_t*>(c.ws + c.L.start), durations, frame_token);
  return vits_launch_status();
}

extern "C" int vits_mas_long_gather(const float* scores, int64_t batch_stride,
                                    const int32_t* t_t_len, const int32_t* t_s_len, int batch,
                                    int t_t, int t_s, int strip, int panel, int y0, int rows,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  VITS_CHECK_ARG(scores != nullptr);
  MlCall c;
  int rc = ml_check(t_t_len, t_s_len, batch, t_t, t_s, strip, panel, workspace, workspace_bytes,
                    &c);
  if (rc) return rc;
  rc = ml_check_panel(t_t, panel, y0, rows);
  if (rc) return rc;
  VITS_CHECK_ARG(batch_stride >= (int64_t)rows * t_s);
  hipLaunchKernelGGL(mas_long_gather_kernel, dim3((rows + 255) / 256, batch), dim3(256), 0,
                     as_stream(stream), scores, batch_stride, t_t_len, t_s_len, t_t, t_s, y0,
                     rows, reinterpret_cast<const int32_t*>(c.ws + c.L.ftok),
                     reinterpret_cast<float*>(c.ws + c.L.val));
  return vits_launch_status();
}

extern "C" int vits_mas_long_scores(const int32_t* t_t_len, const int32_t* t_s_len,
                                    float* token_scores, int batch, int t_t, int t_s, int strip,
                                    int panel, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  VITS_CHECK_ARG(token_scores != nullptr);
  MlCall c;
  const int rc = ml_check(t_t_len, t_s_len, batch, t_t, t_s, strip, panel, workspace,
                          workspace_bytes, &c);
  if (rc) return rc;
  hipLaunchKernelGGL(mas_long_scores_kernel, dim3(batch), dim3(256), 0, as_stream(stream),
                     t_t_len, t_s_len, t_t, t_s, c.L.Ws,
                     reinterpret_cast<const int32_t*>(c.ws + c.L.ftok),
                     reinterpret_cast<const int32_t*>(c.ws + c.L.start),
                     reinterpret_cast<const float*>(c.ws + c.L.val), token_scores);
  return vits_launch_status();
}
