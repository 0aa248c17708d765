// Decoded uint8 frames of any source resolution -> the fp32 model input [sum T, 3, oh, ow]: bicubic resize of a source box, a
// window of the resized image (centre crop), optional horizontal flip, /255 and Normalize, for a whole batch of videos in ONE
// launch (xp_frames_resize_norm; the arithmetic is stated in include/xpretrain_hip.h and, in fp64, in tests/frame_transform_ref.py).
//
// A memory-bound gather: per output pixel 16 uint8 taps x 3 channels in, 3 floats out.  Work decomposition: a workgroup of four
// waves covers a 64-column x 4-row tile of one frame's output; a wave owns one output row, its lanes consecutive x, so every store
// instruction of a wave writes 256 contiguous bytes of one channel plane.  The vertical taps and weights depend on the row only
// (wave-uniform: the row index goes through readfirstlane, the compiler keeps that axis in scalar registers), the horizontal ones
// on the lane only; both are formed once and shared by the three channels.  The source rows are NOT staged in LDS: neighbouring
// lanes' taps overlap in the same few cache lines (a down-scale by 1.07 .. 3 reads 64 .. 200 source pixels per wave row), the
// vector L1 serves the overlap, and arbitrary strides (THWC, TCHW, sliced views) go through one byte-by-byte path.  That path is
// bound by the issue of its 48 byte loads per pixel, not by bandwidth (measured: DESIGN.md 7d), so the decoder's own packed layout
// reads each tap row as four aligned dwords instead (in the kernel, below).
//
// Coordinates are exact: floor(s) and frac(s) of s = ((2 r + 1) box - out) / (2 out) come from integer division (true floor for
// the negative first coordinate), and t = rem / den is ONE correctly rounded fp32 division of two integers below 2^24; 1 - t is
// formed the same way from den - rem.  The Keys weights (A = -0.75) use the factored outer forms A t (1-t)^2 and A (1-t) t^2: no
// cancellation, and exactly 0 / 1 at t = 0, so an identity geometry returns (u / 255 - mean) / std to the bit.
//
// xp_frames_transform is the same launch with two compile-time choices (one body, frames_pixel): the axis function -- the cubic above,
// or a two-stage bilinear resize (Resize, CenterCrop, Resize) folded into four source taps with product weights per axis, so that
// no intermediate image exists -- and a colour stage (brightness, saturation, hue of torchvision's tensor backend, in a per-video
// order) on the three channel values the thread already holds.  The <cubic, no colour> instantiation is xp_frames_resize_norm's
// kernel: same bits.  The aligned-dword reads serve the cubic only: the two-stage taps of a pixel are rarely four consecutive columns.
#include <cfloat>

#include "common.h"
#include "frames_common.h"

namespace {

constexpr int TX = 64, TY = 4;               // output tile of a workgroup: TY waves, one row of TX columns each
constexpr int MAXV = XP_FRAMES_MAX_VIDEOS, MAXT = XP_FRAMES_TRANSFORM_MAX_VIDEOS;
constexpr float KEYS_A = -0.75f;
constexpr int CUBIC = XP_FRAMES_FILTER_BICUBIC, BILINEAR2 = XP_FRAMES_FILTER_BILINEAR2;

struct FramesArgs {
  XpFrameSrc v[MAXV];
  int32_t frame_end[MAXV];                   // number of frames of videos 0 .. i (the output's frame index past video i)
  float mean[3], std[3];
};
static_assert(sizeof(FramesArgs) + 64 <= 4096, "the descriptor table must fit the kernel-argument block");

struct TransformArgs {
  XpFrameTransform v[MAXT];
  int32_t frame_end[MAXT];
  float mean[3], std[3];
};
static_assert(sizeof(TransformArgs) + 64 <= 4096, "the descriptor table must fit the kernel-argument block");

// r: coordinate in the resized axis of length `out` over a source box of length `box` starting at `box0`
__device__ __forceinline__ void cubic_axis(int r, int box, int out, int box0, int (&tap)[4], float (&w)[4]) {
  const int num = (2 * r + 1) * box - out, den = 2 * out;
  int i = num / den, rem = num - i * den;
  if (rem < 0) { rem += den; --i; }          // C division truncates: make it a floor
  const float t = (float)rem / (float)den, s = (float)(den - rem) / (float)den;
  w[0] = KEYS_A * t * (s * s);
  w[1] = ((KEYS_A + 2.0f) * t - (KEYS_A + 3.0f)) * (t * t) + 1.0f;
  w[2] = ((KEYS_A + 2.0f) * s - (KEYS_A + 3.0f)) * (s * s) + 1.0f;
  w[3] = KEYS_A * s * (t * t);
#pragma unroll
  for (int k = 0; k < 4; ++k) tap[k] = box0 + min(max(i - 1 + k, 0), box - 1);
}

// one bilinear stage (F.interpolate, align_corners=False): floor i0 and fraction l of max(0, ((2 r + 1) in - out) / (2 out)) -- the
// negative first coordinate clamps to 0 as PyTorch's does --, the neighbour i1 = min(i0 + 1, in - 1), and 1 - l formed from den - rem
__device__ __forceinline__ void linear_stage(int r, int in, int out, int& i0, int& i1, float& l, float& s) {
  const int num = max((2 * r + 1) * in - out, 0), den = 2 * out;
  i0 = num / den;
  const int rem = num - i0 * den;
  l = (float)rem / (float)den;
  s = (float)(den - rem) / (float)den;
  i1 = min(i0 + 1, in - 1);
}

// r: coordinate in the stage-2 image of length `out`, resized from the window [crop0, crop0 + crop) of the stage-1 image of length
// `mid`, itself resized from the source box: two stage-1 coordinates with two source taps each, product weights
__device__ __forceinline__ void bilinear2_axis(int r, int box, int mid, int crop0, int crop, int out, int box0, int (&tap)[4],
                                               float (&w)[4]) {
  int m[2], j0, j1;
  float l2, s2, l1, s1;
  linear_stage(r, crop, out, m[0], m[1], l2, s2);
  const float w2[2] = {s2, l2};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    linear_stage(crop0 + m[k], box, mid, j0, j1, l1, s1);
    tap[2 * k] = box0 + j0;
    tap[2 * k + 1] = box0 + j1;
    w[2 * k] = w2[k] * s1;
    w[2 * k + 1] = w2[k] * l1;
  }
}

// One output pixel, three channels: taps and weights of both axes (FILTER), the 4 x 4 gather and accumulate, the colour stage
// (COLOR; `e` is read only where FILTER or COLOR needs it), Normalize.  `frame` is the frame's index in the output, `f` in its video.
template <int FILTER, bool COLOR>
__device__ __forceinline__ void frames_pixel(const XpFrameSrc& d, const XpFrameTransform* e, const float (&mean)[3],
                                             const float (&stdv)[3], int frame, int f, int tile_x, int tile_y,
                                             float* __restrict__ out, int oh, int ow) {
  const int y = tile_y * TY + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int x = tile_x * TX + (threadIdx.x & 63);
  if (y >= oh || x >= ow) return;

  int ty[4], tx[4];
  float wy[4], wx[4];
  if constexpr (FILTER == CUBIC) {
    cubic_axis(d.top + y, d.box_h, d.rh, d.box_y, ty, wy);
    cubic_axis(d.left + (d.flip ? ow - 1 - x : x), d.box_w, d.rw, d.box_x, tx, wx);
  } else {
    bilinear2_axis(d.top + y, d.box_h, e->mid_h, e->crop_y, e->crop_h, d.rh, d.box_y, ty, wy);
    bilinear2_axis(d.left + (d.flip ? ow - 1 - x : x), d.box_w, e->mid_w, e->crop_x, e->crop_w, d.rw, d.box_x, tx, wx);
  }
  int64_t xoff[4], yoff[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    xoff[k] = tx[k] * d.stride_x;
    yoff[k] = f * d.stride_t + ty[k] * d.stride_y;
  }
  // The decoder's packed rows (THWC: stride_x 3, stride_c 1): the 4 taps x 3 channels of a pixel whose taps are not clamped are
  // 12 consecutive bytes, read as the 4 ALIGNED dwords that hold them (a quarter of the load instructions) -- wherever those 16
  // bytes lie inside [src, src + src_bytes) for all four rows; every other pixel, and every other layout, loads byte by byte.
  // Both ways feed the same bytes to the same arithmetic: the layouts agree to the bit (tests).  (The cubic's clamped taps never
  // decrease, so a span of 3 means four consecutive columns; the two-stage taps give no such guarantee and load byte by byte.)
  bool packed = FILTER == CUBIC && d.stride_x == 3 && d.stride_c == 1 && tx[3] - tx[0] == 3;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t lo = yoff[j] + xoff[0] - (int64_t)((uintptr_t)(d.src + yoff[j] + xoff[0]) & 3);
    packed = packed && lo >= 0 && lo + 16 <= d.src_bytes;
  }
  float h[3][4];                             // per channel: the four row sums
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float p[12];                             // p[3 i + c]: tap i, channel c of source row ty[j]
    if (packed) {
      const uint8_t* const q = d.src + yoff[j] + xoff[0];
      const unsigned sh = ((unsigned)(uintptr_t)q & 3u) * 8u;
      const uint32_t* const w = reinterpret_cast<const uint32_t*>(q - (sh >> 3));
      const uint64_t w01 = (uint64_t)w[1] << 32 | w[0], w12 = (uint64_t)w[2] << 32 | w[1], w23 = (uint64_t)w[3] << 32 | w[2];
      const uint32_t u[3] = {(uint32_t)(w01 >> sh), (uint32_t)(w12 >> sh), (uint32_t)(w23 >> sh)};
#pragma unroll
      for (int k = 0; k < 12; ++k) p[k] = (float)((u[k >> 2] >> (8 * (k & 3))) & 0xffu);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) p[k] = (float)d.src[yoff[j] + xoff[k / 3] + (k % 3) * d.stride_c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c][j] = fmaf(wx[3], p[9 + c], fmaf(wx[2], p[6 + c], fmaf(wx[1], p[3 + c], wx[0] * p[c])));
  }
  float px[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    px[c] = fmaf(wy[3], h[c][3], fmaf(wy[2], h[c][2], fmaf(wy[1], h[c][1], wy[0] * h[c][0]))) / 255.0f;
  if constexpr (COLOR) color_stage(*e, px);
  float* const o = out + ((int64_t)frame * 3 * oh + y) * ow + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[(int64_t)c * oh * ow] = (px[c] - mean[c]) / stdv[c];
}

__global__ __launch_bounds__(TX * TY) void frames_resize_norm_kernel(FramesArgs a, int n_videos, float* __restrict__ out, int oh,
                                                                    int ow, int tiles_x, int tiles_y) {
  const unsigned b = blockIdx.x;
  const int tile_x = b % tiles_x, tile_y = (b / tiles_x) % tiles_y, frame = b / (tiles_x * tiles_y);
  int vid = 0;
  while (vid < n_videos - 1 && frame >= a.frame_end[vid]) ++vid;
  frames_pixel<CUBIC, false>(a.v[vid], nullptr, a.mean, a.std, frame, frame - (vid ? a.frame_end[vid - 1] : 0), tile_x, tile_y, out,
                             oh, ow);
}

template <int FILTER, bool COLOR>
__global__ __launch_bounds__(TX * TY) void frames_transform_kernel(TransformArgs a, int n_videos, float* __restrict__ out, int oh,
                                                                  int ow, int tiles_x, int tiles_y) {
  const unsigned b = blockIdx.x;
  const int tile_x = b % tiles_x, tile_y = (b / tiles_x) % tiles_y, frame = b / (tiles_x * tiles_y);
  int vid = 0;
  while (vid < n_videos - 1 && frame >= a.frame_end[vid]) ++vid;
  frames_pixel<FILTER, COLOR>(a.v[vid].src, &a.v[vid], a.mean, a.std, frame, frame - (vid ? a.frame_end[vid - 1] : 0), tile_x,
                              tile_y, out, oh, ow);
}

// the first and the last source index an axis reads: the clamped taps of the window's first and last coordinate (host side of the
// same integer arithmetic as cubic_axis)
void axis_extent(int r_lo, int r_hi, int box, int out, int box0, int64_t* lo, int64_t* hi) {
  auto fl = [&](int64_t r) {
    const int64_t num = (2 * r + 1) * box - out, den = 2 * (int64_t)out;
    int64_t i = num / den;
    if (num - i * den < 0) --i;
    return i;
  };
  auto clampi = [&](int64_t i) { return i < 0 ? 0 : (i > box - 1 ? box - 1 : i); };
  *lo = box0 + clampi(fl(r_lo) - 1);
  *hi = box0 + clampi(fl(r_hi) + 2);
}

// the same for the two-stage axis (host side of bilinear2_axis: both stages never decrease, so the first tap of the window's first
// coordinate and the last tap of its last coordinate bound every tap between)
void axis_extent2(int r_lo, int r_hi, int box, int mid, int crop0, int crop, int out, int box0, int64_t* lo, int64_t* hi) {
  auto fl = [](int64_t r, int64_t in, int64_t o) {
    const int64_t num = (2 * r + 1) * in - o;
    return num < 0 ? 0 : num / (2 * o);
  };
  auto next = [](int64_t i, int64_t in) { return i + 1 < in ? i + 1 : in - 1; };
  *lo = box0 + fl(crop0 + fl(r_lo, crop, out), box, mid);
  *hi = box0 + next(fl(crop0 + next(fl(r_hi, crop, out), crop), box, mid), box);
}

// adds the smallest / largest value of stride * index over [lo, hi] to *mn / *mx; false on int64 overflow
bool add_span(int64_t stride, int64_t lo, int64_t hi, int64_t* mn, int64_t* mx) {
  int64_t p, q;
  if (__builtin_mul_overflow(stride, lo, &p) || __builtin_mul_overflow(stride, hi, &q)) return false;
  return !__builtin_add_overflow(*mn, p < q ? p : q, mn) && !__builtin_add_overflow(*mx, p < q ? q : p, mx);
}

// one video's source descriptor with the tap extent of this file's two filters
int check_video(const char* fn, const XpFrameSrc& d, const XpFrameTransform* e, int i, int oh, int ow) {
  if (int rc = xp_frames_check_geometry(fn, d, e, i, oh, ow)) return rc;
  int64_t y0, y1, x0, x1;
  if (e && e->filter == BILINEAR2) {
    axis_extent2(d.top, d.top + oh - 1, d.box_h, e->mid_h, e->crop_y, e->crop_h, d.rh, d.box_y, &y0, &y1);
    axis_extent2(d.left, d.left + ow - 1, d.box_w, e->mid_w, e->crop_x, e->crop_w, d.rw, d.box_x, &x0, &x1);
  } else {
    axis_extent(d.top, d.top + oh - 1, d.box_h, d.rh, d.box_y, &y0, &y1);
    axis_extent(d.left, d.left + ow - 1, d.box_w, d.rw, d.box_x, &x0, &x1);
  }
  return xp_frames_check_extent(fn, d, i, y0, y1, x0, x1);
}

}  // namespace

// Everything the entry points ask of call-level arguments, then of one video's source descriptor (frames_common.h)
int xp_frames_check_call(const char* fn, const void* videos_host, int n_videos, int max_videos, const float* mean3_host,
                         const float* std3_host, const float* out, int oh, int ow) {
  XP_REQUIRE(videos_host, "%s: videos_host is null", fn);
  XP_REQUIRE(mean3_host, "%s: mean3_host is null", fn);
  XP_REQUIRE(std3_host, "%s: std3_host is null", fn);
  XP_REQUIRE(out, "%s: out is null", fn);
  XP_REQUIRE(n_videos >= 1 && n_videos <= max_videos, "%s: n_videos=%d not in 1..%d", fn, n_videos, max_videos);
  XP_REQUIRE(oh > 0 && oh <= XP_FRAMES_MAX_SIZE, "%s: oh=%d not in 1..%d", fn, oh, XP_FRAMES_MAX_SIZE);
  XP_REQUIRE(ow > 0 && ow <= XP_FRAMES_MAX_SIZE, "%s: ow=%d not in 1..%d", fn, ow, XP_FRAMES_MAX_SIZE);
  for (int c = 0; c < 3; ++c)
    XP_REQUIRE(std3_host[c] > 0.f, "%s: std3_host[%d]=%g is not positive", fn, c, (double)std3_host[c]);
  return XP_OK;
}

int xp_frames_check_geometry(const char* fn, const XpFrameSrc& d, const XpFrameTransform* e, int i, int oh, int ow) {
  XP_REQUIRE(d.src, "%s: videos_host[%d].src is null", fn, i);
  XP_REQUIRE(d.src_bytes > 0, "%s: videos_host[%d].src_bytes=%lld is not positive", fn, i, (long long)d.src_bytes);
  XP_REQUIRE(d.T > 0 && d.T <= (1 << 24), "%s: videos_host[%d].T=%d not in 1..%d", fn, i, d.T, 1 << 24);
  XP_REQUIRE(d.H > 0 && d.H <= XP_FRAMES_MAX_SIZE && d.W > 0 && d.W <= XP_FRAMES_MAX_SIZE,
             "%s: videos_host[%d]: source size H=%d W=%d not in 1..%d", fn, i, d.H, d.W, XP_FRAMES_MAX_SIZE);
  XP_REQUIRE(d.box_h > 0 && d.box_w > 0, "%s: videos_host[%d]: box size box_h=%d box_w=%d is not positive", fn, i, d.box_h, d.box_w);
  XP_REQUIRE(d.box_y >= 0 && d.box_x >= 0 && d.box_y <= d.H - d.box_h && d.box_x <= d.W - d.box_w,
             "%s: videos_host[%d]: box (box_y=%d box_x=%d box_h=%d box_w=%d) lies outside the %d x %d image", fn, i, d.box_y, d.box_x,
             d.box_h, d.box_w, d.H, d.W);
  if (e && e->filter == BILINEAR2) {
    XP_REQUIRE(e->mid_h > 0 && e->mid_h <= XP_FRAMES_MAX_SIZE && e->mid_w > 0 && e->mid_w <= XP_FRAMES_MAX_SIZE,
               "%s: videos_host[%d]: stage-1 size mid_h=%d mid_w=%d not in 1..%d", fn, i, e->mid_h, e->mid_w, XP_FRAMES_MAX_SIZE);
    XP_REQUIRE(e->crop_h > 0 && e->crop_w > 0 && e->crop_y >= 0 && e->crop_x >= 0 && e->crop_y <= e->mid_h - e->crop_h &&
                   e->crop_x <= e->mid_w - e->crop_w,
               "%s: videos_host[%d]: crop (crop_y=%d crop_x=%d crop_h=%d crop_w=%d) lies outside the %d x %d stage-1 image (there is no "
               "padding path)", fn, i, e->crop_y, e->crop_x, e->crop_h, e->crop_w, e->mid_h, e->mid_w);
  }
  XP_REQUIRE(d.rh > 0 && d.rh <= XP_FRAMES_MAX_SIZE && d.rw > 0 && d.rw <= XP_FRAMES_MAX_SIZE,
             "%s: videos_host[%d]: resized size rh=%d rw=%d not in 1..%d", fn, i, d.rh, d.rw, XP_FRAMES_MAX_SIZE);
  XP_REQUIRE(d.top >= 0 && d.left >= 0 && d.top <= d.rh - oh && d.left <= d.rw - ow,
             "%s: videos_host[%d]: window (top=%d left=%d, %d x %d) lies outside the %d x %d resized image "
             "(there is no padding path)", fn, i, d.top, d.left, oh, ow, d.rh, d.rw);
  return XP_OK;
}

int xp_frames_check_extent(const char* fn, const XpFrameSrc& d, int i, int64_t y0, int64_t y1, int64_t x0, int64_t x1) {
  int64_t mn = 0, mx = 0;
  const bool fits = add_span(d.stride_t, 0, d.T - 1, &mn, &mx) && add_span(d.stride_y, y0, y1, &mn, &mx) &&
                    add_span(d.stride_x, x0, x1, &mn, &mx) && add_span(d.stride_c, 0, 2, &mn, &mx);
  XP_REQUIRE(fits && mn >= 0 && mx < d.src_bytes,
             "%s: videos_host[%d]: strides (stride_t=%lld stride_y=%lld stride_x=%lld stride_c=%lld) put a tap "
             "outside [0, src_bytes=%lld)", fn, i, (long long)d.stride_t, (long long)d.stride_y, (long long)d.stride_x,
             (long long)d.stride_c, (long long)d.src_bytes);
  return XP_OK;
}

int xp_frames_check_color(const char* fn, const XpFrameTransform& e, int i) {
  XP_REQUIRE(e.n_color >= 0 && e.n_color <= 3, "%s: videos_host[%d].n_color=%d not in 0..3", fn, i, e.n_color);
  for (int k = 0; k < e.n_color; ++k) {
    const int op = e.color_op[k];
    const float f = e.color_factor[k];
    XP_REQUIRE(op == XP_FRAMES_COLOR_BRIGHTNESS || op == XP_FRAMES_COLOR_SATURATION || op == XP_FRAMES_COLOR_HUE,
               "%s: videos_host[%d].color_op[%d]=%d is no colour op (brightness %d, saturation %d, hue %d; there is no contrast)", fn,
               i, k, op, XP_FRAMES_COLOR_BRIGHTNESS, XP_FRAMES_COLOR_SATURATION, XP_FRAMES_COLOR_HUE);
    for (int j = 0; j < k; ++j)
      XP_REQUIRE(e.color_op[j] != op, "%s: videos_host[%d].color_op[%d]=%d repeats color_op[%d]", fn, i, k, op, j);
    if (op == XP_FRAMES_COLOR_HUE)
      XP_REQUIRE(f >= -0.5f && f <= 0.5f, "%s: videos_host[%d].color_factor[%d]=%g (hue) not in [-0.5, 0.5]", fn, i, k, (double)f);
    else
      XP_REQUIRE(f >= 0.f && f <= FLT_MAX, "%s: videos_host[%d].color_factor[%d]=%g (%s) is negative or not finite", fn, i, k,
                 (double)f, op == XP_FRAMES_COLOR_BRIGHTNESS ? "brightness" : "saturation");
  }
  return XP_OK;
}

extern "C" int xp_frames_resize_norm(const XpFrameSrc* videos_host, int32_t n_videos, const float* mean3_host,
                                     const float* std3_host, float* out, int32_t oh, int32_t ow, void* stream) {
  static const char* const fn = "xp_frames_resize_norm";
  if (int rc = xp_frames_check_call(fn, videos_host, n_videos, MAXV, mean3_host, std3_host, out, oh, ow)) return rc;
  FramesArgs a;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean3_host[c];
    a.std[c] = std3_host[c];
  }
  int64_t frames = 0;
  for (int i = 0; i < n_videos; ++i) {
    if (int rc = check_video(fn, videos_host[i], nullptr, i, oh, ow)) return rc;
    a.v[i] = videos_host[i];
    frames += videos_host[i].T;
    a.frame_end[i] = (int32_t)frames;
  }
  for (int i = n_videos; i < MAXV; ++i) { a.v[i] = videos_host[0]; a.frame_end[i] = (int32_t)frames; }
  const int tiles_x = (int)cdiv(ow, TX), tiles_y = (int)cdiv(oh, TY);
  const int64_t blocks = frames * tiles_x * tiles_y;
  XP_REQUIRE(blocks <= INT32_MAX, "xp_frames_resize_norm: %lld frames of %d x %d exceed one launch (n_videos / T too large)",
             (long long)frames, oh, ow);
  frames_resize_norm_kernel<<<(unsigned)blocks, TX * TY, 0, (hipStream_t)stream>>>(a, n_videos, out, oh, ow, tiles_x, tiles_y);
  XP_CHECK_LAUNCH("xp_frames_resize_norm");
  return XP_OK;
}

extern "C" int xp_frames_transform(const XpFrameTransform* videos_host, int32_t n_videos, const float* mean3_host,
                                   const float* std3_host, float* out, int32_t oh, int32_t ow, void* stream) {
  static const char* const fn = "xp_frames_transform";
  if (int rc = xp_frames_check_call(fn, videos_host, n_videos, MAXT, mean3_host, std3_host, out, oh, ow)) return rc;
  TransformArgs a;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean3_host[c];
    a.std[c] = std3_host[c];
  }
  const int filter = videos_host[0].filter;
  XP_REQUIRE(filter == CUBIC || filter == BILINEAR2, "%s: videos_host[0].filter=%d is neither XP_FRAMES_FILTER_BICUBIC (%d) nor "
             "XP_FRAMES_FILTER_BILINEAR2 (%d)", fn, filter, CUBIC, BILINEAR2);
  int64_t frames = 0;
  bool color = false;
  for (int i = 0; i < n_videos; ++i) {
    const XpFrameTransform& e = videos_host[i];
    XP_REQUIRE(e.filter == filter, "%s: videos_host[%d].filter=%d differs from videos_host[0].filter=%d (one filter per call)", fn, i,
               e.filter, filter);
    if (int rc = check_video(fn, e.src, &e, i, oh, ow)) return rc;
    if (int rc = xp_frames_check_color(fn, e, i)) return rc;
    color = color || e.n_color > 0;
    a.v[i] = e;
    frames += e.src.T;
    a.frame_end[i] = (int32_t)frames;
  }
  for (int i = n_videos; i < MAXT; ++i) { a.v[i] = videos_host[0]; a.frame_end[i] = (int32_t)frames; }
  const int tiles_x = (int)cdiv(ow, TX), tiles_y = (int)cdiv(oh, TY);
  const int64_t blocks = frames * tiles_x * tiles_y;
  XP_REQUIRE(blocks <= INT32_MAX, "%s: %lld frames of %d x %d exceed one launch (n_videos / T too large)", fn, (long long)frames, oh, ow);
  const dim3 grid((unsigned)blocks), block(TX * TY);
  const hipStream_t st = (hipStream_t)stream;
  if (filter == CUBIC && !color) frames_transform_kernel<CUBIC, false><<<grid, block, 0, st>>>(a, n_videos, out, oh, ow, tiles_x, tiles_y);
  else if (filter == CUBIC) frames_transform_kernel<CUBIC, true><<<grid, block, 0, st>>>(a, n_videos, out, oh, ow, tiles_x, tiles_y);
  else if (!color) frames_transform_kernel<BILINEAR2, false><<<grid, block, 0, st>>>(a, n_videos, out, oh, ow, tiles_x, tiles_y);
  else frames_transform_kernel<BILINEAR2, true><<<grid, block, 0, st>>>(a, n_videos, out, oh, ow, tiles_x, tiles_y);
  XP_CHECK_LAUNCH("xp_frames_transform");
  return XP_OK;
}

