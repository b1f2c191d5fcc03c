// Shared pieces of the Winograd F(2x2,3x3) convolution kernels (wino3x3.hip: LDS-staged tile blocks; wino_strip.hip: one wave per
// tile block, operands built in registers): launch arguments, packed-subtraction helper, internal epilogue selectors.
#pragma once
#include <cstddef>

#include "mg_common.h"
#include "wino_plan.h"

// (global: wino3x3.hip hands its arguments to wino_strip.hip)
struct WinoArgs {
  const float* x;
  const float* up;
  const float* bias;
  const float* aux;
  float* y;
  float* p;
  float* rn;
  int N, Cin, Cout, H, W;
  int flags;
  float slope;
  int TBW, TBH, TBN, lgTBW, lgTBH;  // tile-block geometry in TILES: TBW * TBH * TBN == TPB
  int blocks_x, blocks_y, blocks_n;
  int nchunk;
  int NT;  // out-channel tiles in the packed weights (padded)
  const unsigned char* mi;  // tile mask read by the epilogue (MG_CONV_MASK_BYTES, fade-in tangent / backward forms)
  unsigned char* mo;        // tile mask written by the epilogue (MG_CONV_MASK_OUT, fade-in forward form)
  const float* other;       // fade-in forms: the old branch (forward / tangent) or its activation (backward)
  const float* coef;        // fade-in forms: {alpha, 1 - alpha} in device memory
};
// (the layout the kernels read: the strip kernel finds its grid in the geometry fields, launch_strip in wino_strip.hip)
static_assert(sizeof(WinoArgs) == 160 && offsetof(WinoArgs, N) == 56 && offsetof(WinoArgs, TBW) == 84 &&
              offsetof(WinoArgs, blocks_x) == 104 && offsetof(WinoArgs, NT) == 120 && offsetof(WinoArgs, mi) == 128);

// the strip kernel (wino_strip.hip) on a call whose plan says p.takes: its grid (p is completed) and the launch
int mgi_wino_strip_run(WinoArgs& a, WinoStripPlan& p, const WinoLayer& L, const WinoSwitches& sw, hipStream_t s);

namespace {

constexpr int WCC = WINO_CC;  // input channels per LDS chunk
constexpr float PN_EPS = 1e-8f;

// Packed fp32 subtraction as ONE instruction (hipcc lowers vector subtraction to one v_sub_f32 per element; fp32 MFMA and VALU
// time add up on gfx950, so every vector instruction of the staging code and the epilogue is matrix time lost).
typedef float wf32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ wf32x2 pk_sub(wf32x2 x, wf32x2 y) {
  wf32x2 d;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(x), "v"(y));
  return d;
}
__device__ __forceinline__ f32x4 pk_sub4(f32x4 x, f32x4 y) {
  const wf32x2 lo = pk_sub(__builtin_shufflevector(x, x, 0, 1), __builtin_shufflevector(y, y, 0, 1));
  const wf32x2 hi = pk_sub(__builtin_shufflevector(x, x, 2, 3), __builtin_shufflevector(y, y, 2, 3));
  return f32x4{lo[0], lo[1], hi[0], hi[1]};
}

}  // namespace
