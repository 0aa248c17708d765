// The frame transforms with an antialias filter (xp_frames_transform_aa; the arithmetic is stated in include/xpretrain_hip.h and, in
// fp64, in tests/frame_antialias_ref.py): F.interpolate(..., antialias=True) on the source box, then xp_frames_transform's window,
// flip, colour stage and Normalize.  The filter's support widens with the scale -- 2 ceil(support) + 1 = 15 / 25 table columns per
// axis for 720 x 1280 -> 224 bicubic -- and every source byte of the box is read, so this is a separable resample through LDS, not
// frames.hip's four-taps-per-axis gather.  Two launches on the caller's stream:
//
// (a) aa_table_kernel: one thread per (video, axis, output coordinate, table column).  x0 and n come from integer arithmetic on the
//     exact rational coordinate; the weights are formed in fp64 (each thread re-forms its row's normaliser, a few dozen filter
//     evaluations), rounded once to fp32, zero beyond n.  The x table is indexed by OUTPUT column, the flip already applied.  For the
//     two-stage bilinear filter the row is the composite W2[r, :] W1[crop0 + ., :]: no intermediate image exists.
//     Workspace, per video and axis, in 4-byte words: int32 x0[count] (a source index, the box origin included), int32 n[count],
//     float w[count][K].
// (b) aa_apply_kernel: a workgroup of four waves owns a 16-row x 32-column output tile of one frame, all three channels.  It copies
//     its rows of both tables into LDS, then walks the source rows of its footprint in chunks of CR rows: stage the chunk's uint8
//     bytes in LDS (the decoder's packed rows as aligned dwords where they lie inside the allocation, every other layout byte by
//     byte: the same bytes either way; eight loads in flight per thread), horizontal pass into fp32 LDS (a lane owns a SOURCE ROW,
//     a half-wave an output column at a time: window and weights are uniform, the byte reads of 32 rows fall on 32 banks; taps
//     ascending), then each thread adds the chunk's rows, ascending, to its two output pixels.  Chunks ascend too, so the summation
//     order is fixed: the horizontal sums first, then the vertical, as the definition has it (what else was tried: DESIGN.md 7g).
//     Colour stage and Normalize on the registers; a half-wave
//     stores one full 128-byte line of a channel plane.  CR and the row pitch are sized by the host from bounds on the footprint
//     (axis_taps / axis_span below); the kernel clamps to them, so a wrong bound could cost accuracy but never memory.
#include <climits>

#include "common.h"
#include "frames_common.h"

namespace {

constexpr int TH = 16, TW = 32, THREADS = 256;      // output tile; a half-wave is one output row of the tile
constexpr int UNROLL = 8;                           // loads a thread keeps in flight while a chunk is staged
constexpr int MAXT = XP_FRAMES_TRANSFORM_MAX_VIDEOS, MAXK = XP_FRAMES_AA_MAX_TAPS;
constexpr int CUBIC = XP_FRAMES_FILTER_BICUBIC, BILINEAR2 = XP_FRAMES_FILTER_BILINEAR2;
constexpr double KEYS_A = -0.5;
constexpr int LDS_SOFT = 40 << 10, LDS_HARD = 64 << 10;      // four workgroups a CU where the footprint allows, never above 64 KiB

// one axis of one video, as the table kernel needs it
struct AaAxis {
  int32_t box, box0, out, win0, count, flip;        // box -> out (rh / rw); the window's first coordinate, its length (oh / ow)
  int32_t mid, crop0, crop;                         // BILINEAR2: box -> mid, window [crop0, crop0 + crop) -> out
  int32_t K, tab;                                   // table columns; the table's first word in the workspace
};
struct AaTableArgs { AaAxis axis[2 * MAXT]; };      // [2 v]: y, [2 v + 1]: x
static_assert(sizeof(AaTableArgs) + 64 <= 4096, "the axis table must fit the kernel-argument block");

// one video, as the apply kernel needs it
struct AaVideo {
  const uint8_t* src; int64_t src_bytes, stride_t, stride_y, stride_x, stride_c;
  int32_t tab_y, tab_x, Ky, Kx;
  int32_t n_color, color_op[3];
  float color_factor[3];
  int32_t pad_;
};
struct AaArgs {
  AaVideo v[MAXT];
  int32_t frame_end[MAXT];
  float mean[3], std[3];
};
static_assert(sizeof(AaArgs) + 128 <= 4096, "the descriptor table must fit the kernel-argument block");

// [x0, end) of resized coordinate r: max(int(c - support + 0.5), 0) and min(int(c + support + 0.5), box) of c = (r + 0.5) box / out,
// support = (k / 2) max(box / out, 1), as quotients of integers (a non-positive numerator gives 0 either way: int() truncates)
__host__ __device__ inline void aa_range(int r, int box, int out, int k, int* x0, int* end) {
  const int c2 = (2 * r + 1) * box + out, s2 = k * (box > out ? box : out), den = 2 * out;
  *x0 = c2 - s2 <= 0 ? 0 : (c2 - s2) / den;
  const int e = (c2 + s2) / den;
  *end = e < box ? e : box;
}

// the filter of k: Keys' cubic (4) or the triangle (2)
__device__ __forceinline__ double aa_filter(double x, int k) {
  x = fabs(x);
  if (k == 2) return x < 1.0 ? 1.0 - x : 0.0;
  if (x < 1.0) return ((KEYS_A + 2.0) * x - (KEYS_A + 3.0)) * x * x + 1.0;
  if (x < 2.0) return ((KEYS_A * x - 5.0 * KEYS_A) * x + 8.0 * KEYS_A) * x - 4.0 * KEYS_A;
  return 0.0;
}

// the normalised weight of source index s (relative to the box) for resized coordinate r whose window is [x0, end)
__device__ double aa_weight(int s, int r, int box, int out, int k, int x0, int end) {
  const double scale = (double)box / (double)out, c = scale * (r + 0.5), inv = scale >= 1.0 ? 1.0 / scale : 1.0;
  double total = 0.0;
  for (int j = x0; j < end; ++j) total += aa_filter((j - c + 0.5) * inv, k);
  return aa_filter((s - c + 0.5) * inv, k) / total;
}

__global__ __launch_bounds__(THREADS) void aa_table_kernel(AaTableArgs a, int filter, uint32_t* __restrict__ ws) {
  const AaAxis& ax = a.axis[blockIdx.y];
  const int e = blockIdx.x * THREADS + threadIdx.x;
  if (e >= ax.count * ax.K) return;
  const int coord = e / ax.K, j = e - coord * ax.K;
  const int r = ax.win0 + (ax.flip ? ax.count - 1 - coord : coord);
  int lo, hi;
  double w = 0.0;
  if (filter == CUBIC) {
    aa_range(r, ax.box, ax.out, 4, &lo, &hi);
    if (lo + j < hi) w = aa_weight(lo + j, r, ax.box, ax.out, 4, lo, hi);
  } else {
    int m0, m1, a0, a1;
    aa_range(r, ax.crop, ax.out, 2, &m0, &m1);                       // stage 2 reads stage-1 coordinates crop0 + [m0, m1)
    aa_range(ax.crop0 + m0, ax.box, ax.mid, 2, &lo, &a1);
    aa_range(ax.crop0 + m1 - 1, ax.box, ax.mid, 2, &a0, &hi);
    const int s = lo + j;
    for (int m = m0; m < m1; ++m) {
      aa_range(ax.crop0 + m, ax.box, ax.mid, 2, &a0, &a1);
      if (s >= a0 && s < a1)
        w += aa_weight(m, r, ax.crop, ax.out, 2, m0, m1) * aa_weight(s, ax.crop0 + m, ax.box, ax.mid, 2, a0, a1);
    }
  }
  const int n = min(hi - lo, ax.K);
  int32_t* const x0tab = reinterpret_cast<int32_t*>(ws) + ax.tab;
  if (j == 0) {
    x0tab[coord] = ax.box0 + lo;
    x0tab[ax.count + coord] = n;
  }
  reinterpret_cast<float*>(x0tab + 2 * ax.count)[coord * ax.K + j] = j < n ? (float)w : 0.0f;
}

template <bool COLOR>
__global__ __launch_bounds__(THREADS) void aa_apply_kernel(AaArgs a, int n_videos, const uint32_t* __restrict__ ws,
                                                           float* __restrict__ out, int oh, int ow, int tiles_x, int tiles_y,
                                                           int KyMax, int KxMax, int pitch, int CR) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t* const s_y0 = reinterpret_cast<int32_t*>(smem);            // [TH] first source row, [TH] taps, [TW] first column, [TW] taps
  int32_t* const s_yn = s_y0 + TH;
  int32_t* const s_x0 = s_yn + TH;
  int32_t* const s_xn = s_x0 + TW;
  float* const wys = reinterpret_cast<float*>(s_xn + TW);            // [TH][KyMax]
  float* const wxs = wys + TH * KyMax;                                // [KxMax][TW]
  float* const hs = wxs + KxMax * TW;                                 // [3][TW][CR | 1]: the horizontal sums of a chunk
  uint8_t* const u8 = reinterpret_cast<uint8_t*>(hs + 3 * TW * (CR | 1));      // [CR][pitch]: the chunk's source bytes

  const unsigned b = blockIdx.x;
  const int tile_x = b % tiles_x, tile_y = (b / tiles_x) % tiles_y, frame = b / (tiles_x * tiles_y);
  int vid = 0;
  while (vid < n_videos - 1 && frame >= a.frame_end[vid]) ++vid;
  const AaVideo& v = a.v[vid];
  const int f = frame - (vid ? a.frame_end[vid - 1] : 0);
  const int tid = threadIdx.x, x = tid & (TW - 1), g = tid / TW;
  const int ty0 = tile_y * TH, th = min(TH, oh - ty0), tx0 = tile_x * TW, tw = min(TW, ow - tx0);
  const int Ky = v.Ky, Kx = v.Kx;

  const int32_t* const ytab = reinterpret_cast<const int32_t*>(ws) + v.tab_y;
  const int32_t* const xtab = reinterpret_cast<const int32_t*>(ws) + v.tab_x;
  const float* const ywt = reinterpret_cast<const float*>(ytab + 2 * oh) + ty0 * Ky;
  const float* const xwt = reinterpret_cast<const float*>(xtab + 2 * ow) + tx0 * Kx;
  if (tid < TH) {
    s_y0[tid] = tid < th ? ytab[ty0 + tid] : 0;
    s_yn[tid] = tid < th ? min(ytab[oh + ty0 + tid], Ky) : 0;
  } else if (tid >= 64 && tid < 64 + TW) {
    const int i = tid - 64;
    s_x0[i] = i < tw ? xtab[tx0 + i] : 0;
    s_xn[i] = i < tw ? min(xtab[ow + tx0 + i], Kx) : 0;
  }
  for (int e = tid; e < th * Ky; e += THREADS) {
    const int i = e / Ky;
    wys[i * KyMax + (e - i * Ky)] = ywt[e];
  }
  for (int e = tid; e < tw * Kx; e += THREADS) {
    const int i = e / Kx;
    wxs[(e - i * Kx) * TW + i] = xwt[e];
  }
  __syncthreads();

  int row_lo = INT_MAX, row_hi = 0, col_lo = INT_MAX, col_hi = 0;
  for (int i = 0; i < th; ++i) {
    row_lo = min(row_lo, s_y0[i]);
    row_hi = max(row_hi, s_y0[i] + s_yn[i]);
  }
  for (int i = 0; i < tw; ++i) {
    col_lo = min(col_lo, s_x0[i]);
    col_hi = max(col_hi, s_x0[i] + s_xn[i]);
  }
  const int wf = min(col_hi - col_lo, (pitch - 3) / 3);              // (the host's bound holds; the clamp keeps a wrong one inside LDS)
  const bool packed = v.stride_x == 3 && v.stride_c == 1;
  const int64_t frame_off = f * v.stride_t;
  const int crp = CR | 1;                                             // odd row count of hs: a half-wave's 32 columns hit 32 banks

  float acc[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  for (int r0 = row_lo; r0 < row_hi; r0 += CR) {
    const int cr = min(CR, row_hi - r0);
    // ---- stage rows r0 .. r0 + cr - 1, columns col_lo .. col_lo + wf - 1.  One flat index over the chunk, UNROLL loads in flight
    // per thread before the first LDS store: the chunk costs a few memory latencies, not one per row.
    if (packed) {
      const int ndw = (3 * wf + 6) >> 2, total = cr * ndw;            // dwords of a row behind up to 3 bytes of alignment
      for (int base = tid; base < total; base += THREADS * UNROLL) {
        uint32_t val[UNROLL];
        int dst[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          const int idx = base + u * THREADS;
          val[u] = 0;
          dst[u] = -1;
          if (idx < total) {
            const int p = idx / ndw, i = idx - p * ndw;
            const int64_t a0 = frame_off + (r0 + p) * v.stride_y + (int64_t)col_lo * 3;
            const int sh = (int)((uintptr_t)(v.src + a0) & 3);
            const int64_t off = a0 - sh + 4 * i;
            dst[u] = p * pitch + 4 * i;
            if (4 * i < sh + 3 * wf) {
              if (off >= 0 && off + 4 <= v.src_bytes) {
                val[u] = *reinterpret_cast<const uint32_t*>(v.src + off);
              } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                  if (off + k >= 0 && off + k < v.src_bytes) val[u] |= (uint32_t)v.src[off + k] << (8 * k);
              }
            }
          }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
          if (dst[u] >= 0) *reinterpret_cast<uint32_t*>(u8 + dst[u]) = val[u];
      }
    } else {
      const int nb = 3 * wf, total = cr * nb;
      for (int base = tid; base < total; base += THREADS * UNROLL) {
        uint8_t val[UNROLL];
        int dst[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          const int idx = base + u * THREADS;
          val[u] = 0;
          dst[u] = -1;
          if (idx < total) {
            const int p = idx / nb, k = idx - p * nb, col = k / 3;
            dst[u] = p * pitch + k;
            val[u] = v.src[frame_off + (r0 + p) * v.stride_y + (col_lo + col) * v.stride_x + (k - 3 * col) * v.stride_c];
          }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
          if (dst[u] >= 0) u8[dst[u]] = val[u];
      }
    }
    __syncthreads();
    // ---- horizontal pass: a lane owns a source row (the pitch is an odd number of dwords: 32 rows, 32 banks), a half-wave walks
    // every eighth output column; x0, n and the weights are uniform over it
    for (int p = tid & 31; p < cr; p += 32) {
      int sh = 0;
      if (packed) sh = (int)((uintptr_t)(v.src + frame_off + (r0 + p) * v.stride_y + (int64_t)col_lo * 3) & 3);
      const uint8_t* const row = u8 + p * pitch + sh;
      for (int xx = tid >> 5; xx < tw; xx += THREADS / 32) {
        const int x0 = s_x0[xx] - col_lo, n = min(s_xn[xx], wf - x0);
        const uint8_t* const q = row + 3 * x0;
        float h0 = 0.f, h1 = 0.f, h2 = 0.f;
        for (int j = 0; j < n; ++j) {
          const float w = wxs[j * TW + xx];
          h0 = fmaf(w, (float)q[3 * j], h0);
          h1 = fmaf(w, (float)q[3 * j + 1], h1);
          h2 = fmaf(w, (float)q[3 * j + 2], h2);
        }
        float* const h = hs + xx * crp + p;
        h[0] = h0;
        h[TW * crp] = h1;
        h[2 * TW * crp] = h2;
      }
    }
    __syncthreads();
    // ---- vertical pass: the chunk's rows inside each of the thread's two windows, ascending
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int y = g + i * (THREADS / TW);
      const int y0 = s_y0[y], lo = max(r0, y0), hi = min(r0 + cr, y0 + s_yn[y]);
      for (int p = lo; p < hi; ++p) {
        const float w = wys[y * KyMax + (p - y0)];
        const float* const h = hs + x * crp + (p - r0);
        acc[i][0] = fmaf(w, h[0], acc[i][0]);
        acc[i][1] = fmaf(w, h[TW * crp], acc[i][1]);
        acc[i][2] = fmaf(w, h[2 * TW * crp], acc[i][2]);
      }
    }
    // (the next chunk's staging writes u8 only, which every thread has finished reading at the barrier above; its horizontal
    //  pass writes hs behind the next barrier, which every thread reaches after this vertical pass)
  }

  if (x >= tw) return;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int y = g + i * (THREADS / TW);
    if (y >= th) continue;
    float px[3] = {acc[i][0] / 255.0f, acc[i][1] / 255.0f, acc[i][2] / 255.0f};
    if constexpr (COLOR) color_stage(v, px);
    float* const o = out + ((int64_t)frame * 3 * oh + ty0 + y) * ow + tx0 + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(int64_t)c * oh * ow] = (px[c] - a.mean[c]) / a.std[c];
  }
}

// ------------------------------------------------------------------------------------------------------------------- host
// 2 ceil(support) + 1 with support = (k / 2) max(box / out, 1): n = int(c + support + 0.5) - int(c - support + 0.5) < 2 support + 1
int64_t axis_taps(int64_t box, int64_t out, int64_t k) { return 2 * cdiv(k * (box > out ? box : out), 2 * out) + 1; }
// source indices `count` consecutive resized coordinates read between them: end(last) - x0(first) < scale (count - 1) + 2 support + 1
int64_t axis_span(int64_t box, int64_t out, int64_t k, int64_t count) {
  const int64_t s = cdiv(box * (count - 1), out) + axis_taps(box, out, k);
  return s < box ? s : box;
}

struct AaPlan {
  AaTableArgs tab;
  int32_t tab_y[MAXT], tab_x[MAXT], Ky[MAXT], Kx[MAXT];
  int64_t words, frames, table_threads;             // workspace words; output frames; the table kernel's widest axis
  int KyMax, KxMax, rows, cols;                     // over the videos: table columns, a tile's footprint
};

// Everything both entry points ask of the descriptors; fills the plan.  `fn` is the entry point's name in the message.
int aa_plan(const char* fn, const XpFrameTransform* videos_host, int n_videos, int oh, int ow, AaPlan* p) {
  XP_REQUIRE(videos_host, "%s: videos_host is null", fn);
  XP_REQUIRE(n_videos >= 1 && n_videos <= MAXT, "%s: n_videos=%d not in 1..%d", fn, n_videos, MAXT);
  XP_REQUIRE(oh > 0 && oh <= XP_FRAMES_MAX_SIZE, "%s: oh=%d not in 1..%d", fn, oh, XP_FRAMES_MAX_SIZE);
  XP_REQUIRE(ow > 0 && ow <= XP_FRAMES_MAX_SIZE, "%s: ow=%d not in 1..%d", fn, ow, XP_FRAMES_MAX_SIZE);
  const int filter = videos_host[0].filter;
  XP_REQUIRE(filter == CUBIC || filter == BILINEAR2, "%s: videos_host[0].filter=%d is neither XP_FRAMES_FILTER_BICUBIC (%d) nor "
             "XP_FRAMES_FILTER_BILINEAR2 (%d)", fn, filter, CUBIC, BILINEAR2);
  *p = AaPlan{};
  for (int i = 0; i < n_videos; ++i) {
    const XpFrameTransform& e = videos_host[i];
    const XpFrameSrc& d = e.src;
    XP_REQUIRE(e.filter == filter, "%s: videos_host[%d].filter=%d differs from videos_host[0].filter=%d (one filter per call)", fn, i,
               e.filter, filter);
    if (int rc = xp_frames_check_geometry(fn, d, &e, i, oh, ow)) return rc;
    if (int rc = xp_frames_check_color(fn, e, i)) return rc;
    int64_t ext[2][2];                              // [axis][first, last source index]
    for (int ax = 0; ax < 2; ++ax) {
      AaAxis& t = p->tab.axis[2 * i + ax];
      t = ax == 0 ? AaAxis{d.box_h, d.box_y, d.rh, d.top, oh, 0, e.mid_h, e.crop_y, e.crop_h, 0, 0}
                  : AaAxis{d.box_w, d.box_x, d.rw, d.left, ow, d.flip != 0, e.mid_w, e.crop_x, e.crop_w, 0, 0};
      const int tile = ax == 0 ? TH : TW, last = t.win0 + t.count - 1;
      int64_t K, span;
      int lo, hi, m0, m1, unused;
      if (filter == CUBIC) {
        K = axis_taps(t.box, t.out, 4);
        span = axis_span(t.box, t.out, 4, tile);
        aa_range(t.win0, t.box, t.out, 4, &lo, &unused);
        aa_range(last, t.box, t.out, 4, &unused, &hi);
      } else {
        const int64_t K2 = axis_taps(t.crop, t.out, 2), K1 = axis_taps(t.box, t.mid, 2);
        K = cdiv((int64_t)t.box * (K2 - 1), t.mid) + K1;
        span = axis_span(t.box, t.mid, 2, axis_span(t.crop, t.out, 2, tile));
        aa_range(t.win0, t.crop, t.out, 2, &m0, &unused);
        aa_range(last, t.crop, t.out, 2, &unused, &m1);
        aa_range(t.crop0 + m0, t.box, t.mid, 2, &lo, &unused);
        aa_range(t.crop0 + m1 - 1, t.box, t.mid, 2, &unused, &hi);
      }
      XP_REQUIRE(K <= MAXK, "%s: videos_host[%d]: the %s axis (%s=%d -> %s=%d) needs %lld taps, above XP_FRAMES_AA_MAX_TAPS=%d", fn, i,
                 ax == 0 ? "vertical" : "horizontal", ax == 0 ? "box_h" : "box_w", t.box, ax == 0 ? "rh" : "rw", t.out, (long long)K,
                 MAXK);
      t.K = (int32_t)K;
      t.tab = (int32_t)p->words;
      p->words += (int64_t)t.count * (2 + K);
      XP_REQUIRE(p->words <= INT32_MAX, "%s: the tables of %d videos exceed 2^31 words (oh=%d, ow=%d)", fn, n_videos, oh, ow);
      const int64_t threads = (int64_t)t.count * K;
      p->table_threads = threads > p->table_threads ? threads : p->table_threads;
      if (ax == 0) { p->KyMax = K > p->KyMax ? (int)K : p->KyMax; p->rows = span > p->rows ? (int)span : p->rows; }
      else { p->KxMax = K > p->KxMax ? (int)K : p->KxMax; p->cols = span > p->cols ? (int)span : p->cols; }
      ext[ax][0] = t.box0 + lo;
      ext[ax][1] = t.box0 + hi - 1;
    }
    if (int rc = xp_frames_check_extent(fn, d, i, ext[0][0], ext[0][1], ext[1][0], ext[1][1])) return rc;
    p->tab_y[i] = p->tab.axis[2 * i].tab;
    p->tab_x[i] = p->tab.axis[2 * i + 1].tab;
    p->Ky[i] = p->tab.axis[2 * i].K;
    p->Kx[i] = p->tab.axis[2 * i + 1].K;
    p->frames += d.T;
  }
  for (int i = 2 * n_videos; i < 2 * MAXT; ++i) p->tab.axis[i] = p->tab.axis[0];
  return XP_OK;
}

}  // namespace

extern "C" size_t xp_frames_transform_aa_workspace_bytes(const XpFrameTransform* videos_host, int32_t n_videos, int32_t oh,
                                                         int32_t ow) {
  AaPlan p;
  if (aa_plan("xp_frames_transform_aa_workspace_bytes", videos_host, n_videos, oh, ow, &p)) return 0;
  return (size_t)p.words * 4;
}

extern "C" int xp_frames_transform_aa(const XpFrameTransform* videos_host, int32_t n_videos, const float* mean3_host,
                                      const float* std3_host, float* out, int32_t oh, int32_t ow, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  static const char* const fn = "xp_frames_transform_aa";
  if (int rc = xp_frames_check_call(fn, videos_host, n_videos, MAXT, mean3_host, std3_host, out, oh, ow)) return rc;
  AaPlan p;
  if (int rc = aa_plan(fn, videos_host, n_videos, oh, ow, &p)) return rc;
  XP_REQUIRE(workspace, "%s: workspace is null", fn);
  XP_REQUIRE_ALIGNED(fn, 4, XP_P(workspace));           // the tables are dwords; (src and out: class `any`, bytes / one float per access)
  XP_REQUIRE(workspace_bytes >= (size_t)p.words * 4, "%s: workspace_bytes=%zu is below the %lld bytes "
             "xp_frames_transform_aa_workspace_bytes reports", fn, workspace_bytes, (long long)p.words * 4);

  AaArgs a;
  bool color = false;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean3_host[c];
    a.std[c] = std3_host[c];
  }
  int64_t frames = 0;
  for (int i = 0; i < MAXT; ++i) {
    const int s = i < n_videos ? i : 0;
    const XpFrameTransform& e = videos_host[s];
    AaVideo& v = a.v[i];
    v = AaVideo{e.src.src, e.src.src_bytes, e.src.stride_t, e.src.stride_y, e.src.stride_x, e.src.stride_c,
                p.tab_y[s], p.tab_x[s], p.Ky[s], p.Kx[s], e.n_color, {e.color_op[0], e.color_op[1], e.color_op[2]},
                {e.color_factor[0], e.color_factor[1], e.color_factor[2]}, 0};
    if (i < n_videos) {
      frames += e.src.T;
      color = color || e.n_color > 0;
    }
    a.frame_end[i] = (int32_t)frames;
  }
  const int tiles_x = (int)cdiv(ow, TW), tiles_y = (int)cdiv(oh, TH);
  const int64_t blocks = frames * tiles_x * tiles_y;
  XP_REQUIRE(blocks <= INT32_MAX, "%s: %lld frames of %d x %d exceed one launch (n_videos / T too large)", fn, (long long)frames, oh, ow);

  // LDS: the tile's table rows, then CR rows of (source bytes + horizontal sums): as many rows as the footprint has, inside
  // LDS_SOFT; at least eight where that still fits LDS_HARD
  // (the pitch is an odd number of dwords and the sums have CR | 1 rows: the kernel's bank reasoning)
  const int pitch = ((3 * p.cols + 6) & ~3) + ((3 * p.cols + 6) & 4 ? 0 : 4);      // a row's bytes behind 0 .. 3 bytes of alignment
  const int fixed = (2 * TH + 2 * TW + TH * p.KyMax + TW * p.KxMax + 3 * TW) * 4, per_row = pitch + 3 * TW * 4;
  int CR = (LDS_SOFT - fixed) / per_row;
  const int hard = (LDS_HARD - fixed) / per_row;
  if (CR < 8) CR = hard < 8 ? hard : 8;
  if (CR > 32) CR &= ~31;                           // whole half-waves of rows in the horizontal pass
  if (CR > p.rows) CR = p.rows;
  XP_REQUIRE(CR >= 1, "%s: a source row of a tile's footprint (%d columns) does not fit LDS", fn, p.cols);
  const size_t lds = (size_t)(2 * TH + 2 * TW + TH * p.KyMax + TW * p.KxMax) * 4 + (size_t)3 * TW * 4 * (CR | 1) + (size_t)CR * pitch;

  const hipStream_t st = (hipStream_t)stream;
  const dim3 tgrid((unsigned)cdiv(p.table_threads, THREADS), (unsigned)(2 * n_videos));
  aa_table_kernel<<<tgrid, THREADS, 0, st>>>(p.tab, videos_host[0].filter, static_cast<uint32_t*>(workspace));
  XP_CHECK_LAUNCH("xp_frames_transform_aa (table)");
  const uint32_t* const ws = static_cast<const uint32_t*>(workspace);
  if (color)
    aa_apply_kernel<true><<<(unsigned)blocks, THREADS, lds, st>>>(a, n_videos, ws, out, oh, ow, tiles_x, tiles_y, p.KyMax, p.KxMax, pitch, CR);
  else
    aa_apply_kernel<false><<<(unsigned)blocks, THREADS, lds, st>>>(a, n_videos, ws, out, oh, ow, tiles_x, tiles_y, p.KyMax, p.KxMax, pitch, CR);
  XP_CHECK_LAUNCH("xp_frames_transform_aa");
  return XP_OK;
}
