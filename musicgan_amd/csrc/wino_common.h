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

// The filter image of a workgroup in LDS -- [chunk][PER 16-byte pieces], a verbatim copy of `nchunk` runs of the packed bank (run ch =
// pieces src_first + ch * src_stride .. + PER - 1) -- filled by LDS-DMA (`buffer_load_dwordx4 ... lds`, wino_wgrad_rows.hip): one wave
// instruction copies 64 consecutive pieces = 1 KiB, needs no staging registers, and EVERY instruction of the fill is requested before
// anybody waits (the copy through registers it replaces compiled to load / s_waitcnt vmcnt(0) / ds_write per 16 bytes and thread:
// 12-27 dependent memory round trips in front of every launch's first MFMA).  Wave `wave` of NWAVE issues instructions wave, wave +
// NWAVE, ... of nchunk * ceil(PER / 64); an instruction never crosses a chunk boundary, and the last one of a chunk whose PER is no
// multiple of 64 runs with the lanes behind the chunk switched off (an out-of-range lane would write zeros, tools/hwtests/
// lds_dma_oob.hip -- onto the next chunk's image or behind the allocation).  The descriptor ends with the packed bank.
// Asynchronous: wino_bank_landed() (this wave's pieces), then the workgroup barrier, before the first read.
typedef __attribute__((address_space(3))) void* wino_lds_ptr;
template <int PER, int NWAVE>
__device__ __forceinline__ void wino_bank_fill(float* lds, const float* bank, int bank_bytes, int nchunk, int src_stride, int src_first,
                                               int wave, int lane) {
  constexpr int IPC = (PER + 63) / 64;  // instructions per chunk
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bank), 0, bank_bytes, 0x00020000);
  const int n = nchunk * IPC;
  for (int q = wave; q < n; q += NWAVE) {  // (wave-uniform)
    const int ch = q / IPC, j = q - ch * IPC;
    float* dst = lds + (ch * PER + 64 * j) * 4;
    const int so = (src_first + ch * src_stride + 64 * j) * 16;
    if ((PER % 64) == 0 || 64 * j + lane < PER) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (wino_lds_ptr)dst, 16, lane * 16, so, 0, 0);
  }
}
// (a "memory" clobber: the kernels' LDS reads are inline assembly and must not move above the wait)
__device__ __forceinline__ void wino_bank_landed() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

}  // namespace
