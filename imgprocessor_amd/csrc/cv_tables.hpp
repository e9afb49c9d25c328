// cv_tables.hpp — OpenCV's interpolation tables at 1/32 px as the library uploads them.  Host code only: no HIP
// header, compiles with a plain C++ compiler.  Three implementations must agree on these bit for bit (the oracle,
// these tables, numpy), so nothing here may be fused into a multiply-add: every function is under fp contract(off).
#pragma once

#include <math.h>

namespace cv_tables {

// OpenCV interpolateLanczos4: float coefficients from double sines, normalised in float
inline void lanczos4_row(float x, float* c) {
#pragma clang fp contract(off)
  static const double s45 = 0.70710678118654752440084436210485;
  static const double cs[][2] = {{1, 0},  {-s45, -s45}, {0, 1},  {s45, -s45},
                                 {-1, 0}, {s45, s45},   {0, -1}, {-s45, s45}};
  if (x < 1.1920929e-07f) {  // FLT_EPSILON
    for (int i = 0; i < 8; i++) c[i] = 0;
    c[3] = 1;
    return;
  }
  float sum = 0;
  const double y0 = -(x + 3) * M_PI * 0.25, s0 = sin(y0), c0 = cos(y0);
  for (int i = 0; i < 8; i++) {
    const double y = -(x + 3 - i) * M_PI * 0.25;
    c[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
    sum += c[i];
  }
  sum = 1.f / sum;
  for (int i = 0; i < 8; i++) c[i] *= sum;
}

// OpenCV interpolateCubic (A = -0.75) in float32
inline void cubic_row(float x, float* c) {
#pragma clang fp contract(off)
  const float A = -0.75f;
  c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
  c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
  c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
  c[3] = 1.f - c[0] - c[1] - c[2];
}

template <int KS> inline void tap_row(float x, float* c);
template <> inline void tap_row<4>(float x, float* c) { cubic_row(x, c); }
template <> inline void tap_row<8>(float x, float* c) { lanczos4_row(x, c); }

// cv::saturate_cast<short>(float): cvRound (half to even), then clamp
inline int sat_short(float v) {
  double r = nearbyint((double)v);
  if (r < -32768.0) r = -32768.0;
  if (r > 32767.0) r = 32767.0;
  return (int)r;
}

// The rows table: [0, 256) the 32 Lanczos4 rows of 8 floats, [256, 384) the 32 bicubic rows of 4.
constexpr int kRowsFloats = 32 * 8 + 32 * 4;
inline void rows_table(float* tab) {
  for (int k = 0; k < 32; k++) lanczos4_row((float)k * (1.f / 32), tab + k * 8);
  for (int k = 0; k < 32; k++) cubic_row((float)k * (1.f / 32), tab + 256 + k * 4);
}

// Which two shorts of a tap row share dword q: the operands of v_dot2_i32_i16 against the tap bytes as the kernels
// hold them.  Bicubic (remap_kernel, bytes (b0, b2) and (b1, b3)): {w0 | w2 << 16, w1 | w3 << 16}.  Lanczos4
// (remap_u8_lz_kernel): adjacent pairs {w0 | w1 << 16, w2 | w3 << 16, w4 | w5 << 16, w6 | w7 << 16}.
template <int KS> struct tap_pack;
template <> struct tap_pack<4> { static constexpr int lo(int q) { return q; } static constexpr int hi(int q) { return q + 2; } };
template <> struct tap_pack<8> { static constexpr int lo(int q) { return 2 * q; } static constexpr int hi(int q) { return 2 * q + 1; } };

// OpenCV's 8U fixed-point weights as a table (imgwarp.cpp initInterTab2D, fixpt): per fraction pair (fy, fx) the
// KS x KS shorts saturate_cast<short>(wy[k1] * wx[k2] * 2^15), their sum forced to 2^15 on one entry of the 2 x 2
// block at (KS/2, KS/2): the largest when the sum is too small, the smallest when it is too large.  Layout: row
// fy * 32 + fx = KS * KS / 2 dwords, tap row after tap row, each packed by tap_pack<KS>.  KS = 4: 32 KB, KS = 8: 128 KB
// (the kernels keep them in LDS).
template <int KS> constexpr int kTab2dDwords = 1024 * KS * KS / 2;
template <int KS> inline void fixed_tab2d(int* packed) {
#pragma clang fp contract(off)
  float t1[32][KS];
  for (int k = 0; k < 32; k++) tap_row<KS>((float)k * (1.f / 32), t1[k]);
  constexpr int H = KS / 2;
  for (int fy = 0; fy < 32; fy++)
    for (int fx = 0; fx < 32; fx++) {
      int itab[KS * KS], isum = 0;
      for (int k1 = 0; k1 < KS; k1++) {
        const float vy = t1[fy][k1];
        for (int k2 = 0; k2 < KS; k2++) {
          const float v = vy * t1[fx][k2];
          isum += itab[k1 * KS + k2] = sat_short(v * 32768.f);
        }
      }
      if (isum != 32768) {
        const int diff = isum - 32768;
        int Mk1 = H, Mk2 = H, mk1 = H, mk2 = H;
        for (int k1 = H; k1 < H + 2; k1++)
          for (int k2 = H; k2 < H + 2; k2++) {
            if (itab[k1 * KS + k2] < itab[mk1 * KS + mk2]) { mk1 = k1; mk2 = k2; }
            else if (itab[k1 * KS + k2] > itab[Mk1 * KS + Mk2]) { Mk1 = k1; Mk2 = k2; }
          }
        if (diff < 0) itab[Mk1 * KS + Mk2] = (short)(itab[Mk1 * KS + Mk2] - diff);
        else itab[mk1 * KS + mk2] = (short)(itab[mk1 * KS + mk2] - diff);
      }
      int* row = packed + (fy * 32 + fx) * (KS * H);
      for (int r = 0; r < KS; r++)
        for (int q = 0; q < H; q++) {
          const int* w = itab + r * KS;
          row[r * H + q] = (w[tap_pack<KS>::lo(q)] & 0xffff) | (int)((unsigned)w[tap_pack<KS>::hi(q)] << 16);
        }
    }
}

}  // namespace cv_tables
