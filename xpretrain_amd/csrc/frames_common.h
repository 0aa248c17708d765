// What the frame transforms share (frames.hip: xp_frames_resize_norm, xp_frames_transform; frames_aa.hip: xp_frames_transform_aa):
// the host-side argument checks (defined in frames.hip) and the colour stage -- brightness, saturation and hue of torchvision's
// tensor backend on the three channel values a thread holds, in a per-video order.
#pragma once
#include "common.h"

// Call-level arguments; one video's source descriptor without its tap extent (`e`: the transform descriptor it belongs to, null for
// xp_frames_resize_norm); that the source indices [y0, y1] x [x0, x1] a launch reads lie inside [src, src + src_bytes); the colour
// ops.  `fn` is the entry point's name in the message.  XP_OK, or XP_ERR_ARG with the message set.
int xp_frames_check_call(const char* fn, const void* videos_host, int n_videos, int max_videos, const float* mean3_host,
                         const float* std3_host, const float* out, int oh, int ow);
int xp_frames_check_geometry(const char* fn, const XpFrameSrc& d, const XpFrameTransform* e, int i, int oh, int ow);
int xp_frames_check_extent(const char* fn, const XpFrameSrc& d, int i, int64_t y0, int64_t y1, int64_t x0, int64_t x1);
int xp_frames_check_color(const char* fn, const XpFrameTransform& e, int i);

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// torchvision's adjust_hue on a float pixel (_rgb2hsv, h = (h + f) % 1, _hsv2rgb), behind a clamp of the input to [0, 1]
__device__ __forceinline__ void hue_shift(float (&x)[3], float f) {
  const float r = clamp01(x[0]), g = clamp01(x[1]), b = clamp01(x[2]);
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.0f : maxc);
  const float dv = eqc ? 1.0f : cr;
  const float rc = (maxc - r) / dv, gc = (maxc - g) / dv, bc = (maxc - b) / dv;
  float h = maxc == r ? bc - gc : (maxc == g ? 2.0f + rc - bc : 4.0f + gc - rc);
  h = fmodf(h / 6.0f + 1.0f, 1.0f);
  h += f;
  h -= floorf(h);                            // Python's % 1: into [0, 1]
  const float h6 = h * 6.0f, fl = floorf(h6), fr = h6 - fl;
  const int i = (int)fl % 6;
  const float v = maxc;
  const float p = clamp01(v * (1.0f - s)), q = clamp01(v * (1.0f - s * fr)), t = clamp01(v * (1.0f - s * (1.0f - fr)));
  x[0] = (i == 0 || i == 5) ? v : (i == 1 ? q : (i == 4 ? t : p));
  x[1] = (i == 1 || i == 2) ? v : (i == 0 ? t : (i == 3 ? q : p));
  x[2] = (i == 3 || i == 4) ? v : (i == 2 ? t : (i == 5 ? q : p));
}

// the colour ops of one video on the float pixel x (v / 255, overshoot included), in the descriptor's order; E: any descriptor
// with XpFrameTransform's n_color, color_op[] and color_factor[]
template <class E>
__device__ __forceinline__ void color_stage(const E& e, float (&x)[3]) {
  for (int k = 0; k < e.n_color; ++k) {
    const float f = e.color_factor[k];
    const int op = e.color_op[k];
    if (op == XP_FRAMES_COLOR_BRIGHTNESS) {
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = clamp01(f * x[c]);
    } else if (op == XP_FRAMES_COLOR_SATURATION) {
      const float gray = 0.2989f * x[0] + 0.587f * x[1] + 0.114f * x[2];
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = clamp01(f * x[c] + (1.0f - f) * gray);
    } else {
      hue_shift(x, f);
    }
  }
}
