// What the three translation units of the Winograd weight gradient share: kernel arguments, LDS constants, the packed subtract,
// the (CT, OT) dispatcher and the launchers of the kernel families.
//   wino_wgrad.hip         chunk-staged wide form (ww_body, wino_wgrad_mfma), grouped launch, slab reduce, the C entry points
//   wino_wgrad_narrow.hip  chunk-staged narrow form (wino_wgrad_narrow_mfma)
//   wino_wgrad_rows.hip    row-staged form (wino_wgrad_rows_mfma)
//   wino_wgrad_plan.h      the launch planner, plain host C++
#pragma once
#include <climits>
#include <type_traits>
#include <utility>

#include "mg_common.h"
#include "wino_wgrad_plan.h"

typedef float wg_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ wg_f32x2 pk_sub(wg_f32x2 x, wg_f32x2 y) {  // x - y as one packed instruction
  wg_f32x2 d;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(x), "v"(y));
  return d;
}

constexpr int CH = 64;                 // channel slots per operand image (CT, OT <= 4)
constexpr int IMG = 8 * 4 * CH * 4;    // floats per operand image: [8 comp pairs][4 tile pairs][64 channels][k-step 2][parity 2]
constexpr int STAGE = 2 * IMG;         // V image + Y image
constexpr size_t WW_LDS_WIDE = (size_t)2 * STAGE * sizeof(float);  // two stages: ww_body (wino_wgrad_mfma, wino_wgrad_group_mfma)

struct WwPtrs {
  const float* x;
  const float* gy;
  float* slab;    // [nsplit][9 taps][CinP][CoutP]
  float* slab_b;  // [nsplit][CoutP]
};
// pointers, then the plan's geometry, then the byte limits: the kernels read a.x, a.N, a.per, ... of one flat argument block
struct WwArgs : WwPtrs, WwGeo {
  int bias_n;
  unsigned x_bytes, gy_bytes;
};
static_assert(sizeof(WwArgs) == sizeof(WwPtrs) + sizeof(WwGeo) + 16, "WwArgs: no padding between its parts");

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct WwGroup {
  int n;
  int first[WW_GROUP + 1];
  int nsplit[WW_GROUP];
  int var[WW_GROUP];  // ww_var(CT, OT, UPS)
  WwArgs a[WW_GROUP];
};

constexpr int WW_JOBS = 40;
struct WwJobs {
  int n;
  int first[WW_JOBS + 1];  // prefix sums of the jobs' block counts: workgroup b belongs to the job with first[i] <= b < first[i + 1]
  mg_wgrad_job_t j[WW_JOBS];
};

// Runtime (CT, OT) in 1..4 -> f(integral_constant<int, CT>, integral_constant<int, OT>) of the matching pair.  f returns
// WW_NO_TILE for a pair its kernel family is not instantiated for.
constexpr int WW_NO_TILE = INT_MIN;
template <class F, size_t... I>
int ww_for_tiles_impl(int CT, int OT, F&& f, std::index_sequence<I...>) {
  int rc = WW_NO_TILE;
  (void)((((int)(I / 4) + 1 == CT && (int)(I % 4) + 1 == OT) &&
          (rc = f(std::integral_constant<int, (int)(I / 4) + 1>{}, std::integral_constant<int, (int)(I % 4) + 1>{}), true)) || ...);
  if (rc == WW_NO_TILE) {
    mg_set_error("mg_wino3x3_wgrad: internal tile error (CT=%d, OT=%d)", CT, OT);
    return MG_EINVAL;
  }
  return rc;
}
template <class F>
int ww_for_tiles(int CT, int OT, F&& f) {
  return ww_for_tiles_impl(CT, OT, f, std::make_index_sequence<16>{});
}

template <class F>
int ww_for_flags(bool ups, bool fast, F&& f) {  // runtime (ups, fast) -> f(bool_constant, bool_constant)
  if (ups) return fast ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
  return fast ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

// Launch of one kernel instantiation with workgroups of 512; its dynamic-LDS limit is a per-device function attribute, set on first use
template <auto KERNEL, class A>
int ww_launch(const char* what, size_t lds, const A& a, dim3 grid, hipStream_t s) {
  static MgPerDevice once;
  if (mg_first_use_on_device(once)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  hipLaunchKernelGGL(KERNEL, grid, dim3(512), lds, s, a);
  MG_CHECK_LAUNCH(what);
  return MG_OK;
}

// One layer, one launch, grid = (splits, channel block pairs); the wide form's launcher is local to wino_wgrad.hip
int mg_ww_launch_narrow(int CT, int OT, bool ups, bool fast, const WwArgs& a, dim3 grid, hipStream_t s);  // CT + OT <= 4
int mg_ww_launch_rows(int CT, int OT, bool ups, bool fast, const WwArgs& a, dim3 grid, hipStream_t s);    // not (4, 4); `fast` unused
