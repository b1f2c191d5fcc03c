// Winograd F(3x3, 2x2) weight gradient (wino_wgrad.hip), row-staged form.
#include "wino_wgrad.h"

namespace {

// ---- row-staged form (round 6): the operands are transformed IN REGISTERS, in MFMA operand layout, from RAW rows that the memory
// system writes straight into LDS (LDS-DMA, `buffer_load_dwordx4 ... lds`).
// The two kernels above transform on the way INTO LDS: a thread owns a (tile, channel) item, computes all 16 Winograd components of it
// and scatters them over eight component-pair images (64 B per item and operand), so a stage holds only 8 tiles, every 8 tiles cost a
// workgroup barrier, and the per-item work (halo exchange by DPP + selects, 16 packed adds, 8 LDS writes, the loads' address
// arithmetic) is 1.6 vector + 1.7 scalar instructions per MFMA on the widest block shape and 3.7 + 4.2 on the narrow ones
// (profiles/r06_pmc_w20n_base.txt, r06_pmc_ww16_base.txt: 64 % of the wave cycles waiting).  Here
//   * a stage is 16 horizontally adjacent tiles (one k-step = 4 tiles, 4 k-steps) of all channels of the block as RAW pixels:
//     x rows 2by-1 .. 2by+2, pixels -1 .. 34 of the stage (nine 16-byte pieces per row), gy rows 2by, 2by+1 (eight pieces) -- 8 bytes
//     per item and row instead of 64: half the barriers in 45 % of the LDS.  The stage image is a sequence of 16-byte pieces and wave
//     w copies pieces 64 (w + 8 m) .. + 63 with ONE LDS-DMA instruction per m (5-7 per wave and stage): no staging registers, no LDS
//     store instructions (`ds_write_b128` moves 79 B per clock: measured, the register-staged version of this kernel spent 12 % of
//     its time in them and another 13 % around the loads), lane offsets fixed for the kernel, the stage in a scalar offset.  Pieces of
//     rows above / below the image, of channels beyond the tensor and the padding pieces have an out-of-range offset: the bounds
//     check writes ZEROS for them, per dword (tools/hwtests/lds_dma_oob.hip), which is also what clips the last row's pixels behind the
//     tensor's end.  Pixel -1 of a row's first stage and pixel 32 of its last one are fetched (they exist: the neighbouring row's) and
//     overwritten with zeros by the wave that copied them; x[-1] itself, before the tensor, is never touched (the first stage's first
//     piece is patched from pixel 0 on);
//   * an x row is stored from pixel -1 on, so the 4-pixel patch row of tile T (pixels 2T-1 .. 2T+2) starts at an even word:
//     [e0, p0 | p1, e1]; wave w owns component pair w as before -- row i = w / 2 of the component matrix, columns (0, 3) for even and
//     (1, 2) for odd w -- and lane (rq, col) reads, for tile 4 ks + rq and channel 16 i + col, exactly the TWO patch rows its component
//     row needs (B^T d: d0 - d2, d1 + d2, d2 - d1, d1 - d3): two packed adds for the row step, and the column step is ONE packed add of
//     the two halves -- (u0 - u2, u1 - u3) = (v0, v3) for even waves, (u1 + u2, u2 - u1) = (v1, v2) for odd ones -- whose result IS the
//     A operand pair; the gy side is 0-2 packed adds per out-channel tile (A t A^T: row i is t0, t0 + t1, t0 - t1 or t1; the signs of
//     the components that carry a minus are applied once, to the accumulators, after the tile loop);
//   * nothing else in the loop: no DPP, no selects, no per-lane address arithmetic (LDS offsets are immediates);
//   * every operand read is a `ds_read_b64` (two 32-lane groups, bank = word mod 64, 256 B per clock): lane (rq, col) reads words
//     col * stride + 2 rq + {0, 1}, so channel strides of 4 x odd modulo 64 (148, 68 words) give the 16 channels x 2 tiles of a group
//     64 different banks.  The reads are inline assembly: hipcc merges adjacent 8-byte LDS reads into `ds_read2_b64`, which this LDS
//     serves at HALF the rate with banks modulo 32 (MI355X_MICROARCH.md, LDS).  Measured on the way (profiles/r06_wgrad_rows_steps.txt,
//     48 x 64 @128 x 192 images, chunk-staged kernel 914 us): strides of 16 modulo 64 with 4-byte halo reads 1 306 us
//     (SQ_LDS_BANK_CONFLICT 84 % of the LDS cycles); 16-byte patch rows as ds_read2_b64 on strides of 24 / 8: 1 075 us (72 %).
// Each wave runs ONE of eight specialisations of the tile loop (component row x parity), chosen once; all of them execute the
// same barriers.  Accumulator layout, G^T M G slab pass and reduce kernel are those of wino_wgrad_mfma.
constexpr int RW_RS = 36;              // words per staged x row: pixel p (-1 .. 34) at word p + 1 = 9 pieces
constexpr int RW_CSX = 4 * RW_RS + 4;  // words per x channel (4 rows + one padding piece = 37 pieces); 148 = 4 * 5 mod 64
constexpr int RW_CSY = 68;             // words per gy channel: 2 rows x 32 pixels + one padding piece = 17 pieces (= 4 mod 64)
// UPS (the convolution input is the nearest x2 up-sampling of x, generator.py:24-25): the patch of tile (TY, TX) is the 3x3 low-res
// neighbourhood with its centre row / column doubled, so a stage holds low-res rows TY-1 .. TY+1, pixels -1 .. 18 (five pieces)
constexpr int RW_RSU = 20;
constexpr int RW_CSXU = 3 * RW_RSU + 8;  // 3 rows + two padding pieces = 17 pieces; 68 = 4 mod 32 (4-byte reads: banks modulo 32)

template <int CT, int OT, bool UPS = false>
struct RwGeom {
  static constexpr int RS = UPS ? RW_RSU : RW_RS, CSX = UPS ? RW_CSXU : RW_CSX;
  static constexpr int PPR = UPS ? 5 : 9, ROWS = UPS ? 3 : 4, PPC = CSX / 4;  // pieces per row, rows and pieces per x channel
  static constexpr int XI = (16 * CT * PPC + 63) / 64;  // LDS-DMA instructions (64 pieces each) of the x part, of the gy part
  static constexpr int YI = (16 * OT * 17 + 63) / 64;
  static constexpr int NI = XI + YI;
  static constexpr int NM = (NI + 7) / 8;  // per wave
  static constexpr int YB = XI * 256;      // words
  static constexpr int STG = NI * 256;
  static constexpr size_t lds_bytes() {
    const size_t stages = (size_t)2 * STG * sizeof(float), slab = (size_t)16 * 32 * 64 * sizeof(float);
    return stages > slab ? stages : slab;
  }
};

template <class F, int... Is>
__device__ __forceinline__ void rw_static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void rw_static_for(F&& f) {
  rw_static_for_impl(f, std::make_integer_sequence<int, N>{});
}
// 8 bytes of LDS at byte address `addr` + OFF.  NOT tracked by hipcc's s_waitcnt insertion: rw_lds_wait() before the first use.
template <int OFF>
__device__ __forceinline__ f32x2 rw_lds64(unsigned addr) {
  f32x2 v;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
template <int OFF>
__device__ __forceinline__ float rw_lds32(unsigned addr) {
  float v;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
__device__ __forceinline__ void rw_lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void rw_tie(float& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void rw_tie(f32x2& v) { asm volatile("" : "+v"(v)); }  // orders the uses of v behind the wait
typedef __attribute__((address_space(3))) void* rw_lds_ptr;

template <int CT, int OT, bool UPS>
__global__ void __launch_bounds__(512) wino_wgrad_rows_mfma(const WwArgs a) {
  using GEO = RwGeom<CT, OT, UPS>;
  constexpr int YB = GEO::YB, STG = GEO::STG, XI = GEO::XI, NI = GEO::NI, NM = GEO::NM;
  constexpr int RS = GEO::RS, CSX = GEO::CSX, PPR = GEO::PPR, PPC = GEO::PPC, XROWS = GEO::ROWS;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // = component pair
  const int col = lane & 15, rq = lane >> 4;
  const int split = blockIdx.x;
  const int cb = blockIdx.y / a.nob, ob = blockIdx.y % a.nob;
  const int c0 = cb * CT * 16, o0 = ob * OT * 16;
  const int HW = a.H * a.W;
  const int Ht = a.H >> 1;
  const int Wx = UPS ? a.W >> 1 : a.W, HWx = UPS ? HW >> 2 : HW;  // the x tensor's row and plane
  constexpr unsigned INV = 0x80000000u;

  // ---- loader: slot m of this wave is LDS-DMA instruction k = wave + 8 m of a stage, this lane's piece P = 64 k + lane.
  // x part (k < XI): P = 37 ch + 9 r + seg -- pixels 4 seg - 1 .. 4 seg + 2 of patch row r of channel ch (P mod 37 = 36: padding);
  // gy part: P - 64 XI = 17 ch + 8 r + seg.  x is addressed relative to x - (W + 4) floats, so that row -1 and pixel -1 have
  // non-negative offsets.  voff[m]: byte offset of the piece inside a stage, INV = write zeros.  cls: per slot, bit 4m: the piece is
  // patch row 0 (outside the image in the top tile row), 4m+1: patch row 3 (bottom), 4m+2: its first word is pixel -1, 4m+3: its
  // second word is pixel 32.
  unsigned voff[NM];
  unsigned cls = 0;
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    const int k = wave + 8 * m;
    const int P = 64 * k + lane;
    unsigned v = INV;
    if (k < XI) {
      const int ch = P / PPC, rem = P - PPC * ch, r = rem / PPR, sg = rem - PPR * r;
      if (ch < 16 * CT && rem < XROWS * PPR && c0 + ch < a.Cin) {
        v = (unsigned)((ch * HWx + r * Wx + 4 * sg + 3) * 4);
        cls |= (unsigned)(r == 0) << (4 * m) | (unsigned)(r == XROWS - 1) << (4 * m + 1) | (unsigned)(sg == 0) << (4 * m + 2) |
               (unsigned)(sg == PPR - 1) << (4 * m + 3);
      }
    } else if (k < NI) {
      const int Q = P - 64 * XI;
      const int ch = Q / 17, rem = Q - 17 * ch, r = rem >> 3, sg = rem & 7;
      if (ch < 16 * OT && rem < 16 && o0 + ch < a.Cout) v = (unsigned)((ch * HW + r * a.W + 4 * sg) * 4);
    }
    voff[m] = v;
  }
  const unsigned xshift = (unsigned)(Wx + 4) * 4u;
  const char* xbase = reinterpret_cast<const char*>(a.x) - xshift;
  // The piece that begins at x[-1], BEFORE the tensor, must not be fetched: image row 0 of channel 0 of image 0, piece 0 -- patch row 1
  // of the tensor's first stage (lane PPR of wave 0's slot 0) and, in the up-sampled form, also patch row 0 of the stage below it
  // (lane 0).  That lane's piece is zero-filled and x[0 .. 2] are written behind it once the stage has landed.

  bool zl = false, zr = false;  // the stage copied last begins / ends at the image's left / right edge
  int nq = 0, bx, by, bn;
  {
    const int b0 = split * a.per;
    bx = b0 % a.blocks_x;
    const int t2 = b0 / a.blocks_x;
    by = t2 % a.blocks_y;
    bn = t2 / a.blocks_y;
  }
  // the slab's next stage -> LDS at word offset so (asynchronous: landed() before the barrier that precedes its first read).  The
  // stage's 5-7 copy instructions per wave are issued a few at a time (issue_begin, issue_slots<LO, HI>, ...): all 45-54 of a
  // workgroup in one burst right behind the barrier fill the CU's memory pipeline, and every wave sits at its last copy instruction
  // instead of issuing MFMAs (measured: the burst cost 13 % of the kernel's cycles).
  __amdgpu_buffer_rsrc_t st_xs, st_ys;
  int st_sx = 0, st_sy = 0, st_so = 0;
  bool st_top = false, st_bot = false, st_patch = false;
  int st_lowlane = -1;
  auto issue_begin = [&](int so) __attribute__((always_inline)) {
    const bool ok = nq < a.per && split * a.per + nq < a.nblk;
    st_top = by == 0;
    st_bot = by == Ht - 1;
    st_xs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(xbase), 0, ok ? (int)(a.x_bytes + xshift) : 0, 0x00020000);
    st_ys = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.gy), 0, ok ? (int)a.gy_bytes : 0, 0x00020000);
    st_sx = UPS ? ((bn * a.Cin + c0) * HWx + by * Wx + 16 * bx) * 4 : ((bn * a.Cin + c0) * HW + 2 * by * a.W + 32 * bx) * 4;
    st_sy = ((bn * a.Cout + o0) * HW + 2 * by * a.W + 32 * bx) * 4;
    if (!UPS && (a.TBN & 16)) { st_sx = (c0 * HW + (2 + (split & 31) * 2) * a.W) * 4; st_sy = (o0 * HW + (2 + (split & 31) * 2) * a.W) * 4; }  // (rows >= 1: inside the tensor)
    st_lowlane = (bn == 0 && c0 == 0 && bx == 0 && ok) ? (by == 0 ? PPR : ((UPS && by == 1) ? 0 : -1)) : -1;
    st_patch = wave == 0 && st_lowlane >= 0;
    st_so = so;
    zl = bx == 0;
    zr = bx == a.blocks_x - 1;
    ++nq;
    ++bx;
    const int wx = bx == a.blocks_x ? 1 : 0;
    bx = wx ? 0 : bx;
    by += wx;
    const int wy = by == a.blocks_y ? 1 : 0;
    by = wy ? 0 : by;
    bn += wy;
  };
  auto issue_slots = [&](auto lo_, auto hi_) __attribute__((always_inline)) {
    constexpr int LO = decltype(lo_)::value, HI = decltype(hi_)::value < NM ? decltype(hi_)::value : NM;
#pragma unroll
    for (int m = LO; m < HI; ++m) {
      const int k = wave + 8 * m;
      if (k < NI) {  // (wave-uniform)
        float* dst = smem + st_so + 256 * k;
        if (k < XI) {
          if ((a.TBN & 64) && (k & 1)) continue;  // (measurement: every second x copy instruction dropped)
          unsigned v = voff[m];
          if (st_top || st_bot || st_patch) {  // (wave-uniform; the common stage takes the offsets as they are)
            const bool kill = (st_top && ((cls >> (4 * m)) & 1u)) || (st_bot && ((cls >> (4 * m + 1)) & 1u)) || (st_patch && m == 0 && lane == st_lowlane);
            v = kill ? INV : v;
          }
          __builtin_amdgcn_raw_ptr_buffer_load_lds(st_xs, (rw_lds_ptr)dst, 16, (int)v, st_sx, 0, 0);
        } else {
          __builtin_amdgcn_raw_ptr_buffer_load_lds(st_ys, (rw_lds_ptr)dst, 16, (int)voff[m], st_sy, 0, 0);
        }
      }
    }
  };
  using M0_ = std::integral_constant<int, 0>; using M2_ = std::integral_constant<int, 2>; using M4_ = std::integral_constant<int, 4>;
  using M6_ = std::integral_constant<int, 6>; using M8_ = std::integral_constant<int, 8>;
  auto issue_stage = [&](int so) __attribute__((always_inline)) {
    issue_begin(so);
    issue_slots(M0_{}, M8_{});
  };
  // the stage at word offset so has landed (this wave's pieces): zero the pixels beside the image that this wave copied
  auto landed = [&](int so) __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (st_patch && lane == st_lowlane) {  // (the piece that begins at x[-1]: zero-filled, now x[0 .. 2] behind the zero)
      float* pc = smem + so + 4 * lane;
      pc[1] = a.x[0];
      pc[2] = a.x[1];
      pc[3] = a.x[2];
    }
    if (zl || zr) {  // (wave-uniform)
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const int k = wave + 8 * m;
        if (k < XI) {
          float* pc = smem + so + 256 * k + 4 * lane;
          if (zl && ((cls >> (4 * m + 2)) & 1u)) pc[0] = 0.f;
          if (zr && ((cls >> (4 * m + 3)) & 1u)) pc[1] = 0.f;
        }
      }
    }
  };

  f32x4 acc[2][CT][OT];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
      for (int j = 0; j < OT; ++j) acc[p][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum[OT];
#pragma unroll
  for (int j = 0; j < OT; ++j) bsum[j] = 0.f;

  // LDS byte addresses of this lane's operand reads (the low 32 bits of a shared-aperture address are the LDS offset)
  // (UPS: tile T's low-res pixels T-1, T, T+1 are words T, T+1, T+2 of a row)
  const unsigned xrd_a = (unsigned)reinterpret_cast<size_t>(smem + col * CSX + (UPS ? 1 : 2) * rq);  // + 16 i CSX + row RS + 8 ks: [e0, p0 | p1, e1] of tile 4 ks + rq
  const unsigned yrd_a = (unsigned)reinterpret_cast<size_t>(smem + YB + col * RW_CSY + 2 * rq);  // + 16 j CSY + row 32 + 8 ks: (t.0, t.1)

  auto tile_loop = [&](auto i_, auto odd_) __attribute__((always_inline)) {
    constexpr int I = decltype(i_)::value;
    constexpr bool ODD = decltype(odd_)::value;
    constexpr int RA = I == 0 ? 0 : (I == 2 ? 2 : 1), RB = I == 0 ? 2 : (I == 1 ? 2 : (I == 2 ? 1 : 3));  // u = d[RA] +- d[RB]
    constexpr bool PLUS = I == 1;
    constexpr bool Y0 = I != 3, Y1 = I != 0;  // which gy rows the component row needs
    // UPS: the component row is  i = 0: l[TY-1] - l[TY];  1: 2 l[TY];  2: ZERO;  3: l[TY] - l[TY+1]  over the low-res pixels (L, C, R) =
    // (TX-1, TX, TX+1), the columns  0: uL - uC;  1: 2 uC;  2: ZERO;  3: uC - uR -- 9 of the 16 components.  Row 2 has no wave work
    // at all (IDLE), an odd wave computes column 1 only (NP = 1); the factors of two are applied once, to the accumulators.
    constexpr bool IDLE = UPS && I == 2;
    constexpr int NP = (UPS && ODD) ? 1 : 2;                        // components this wave accumulates
    constexpr int UA = I == 0 ? 0 : 1, UB = I == 0 ? 1 : 2;         // UPS: low-res rows of u = l[UA] - l[UB]  (I = 1: l[1] alone)
    struct Raw {
      f32x2 al[CT], ah[CT], bl[CT], bh[CT], t0[OT], t1[OT];  // rows RA / RB as (e0, p0) | (p1, e1); gy rows
      float ua[CT][3], ub[CT][3];                             // UPS: (L, C, R) of the two low-res rows
    };
    struct Ops {
      f32x2 av[CT], bv[OT];  // the wave's two x components per in-channel tile / two gy components (unsigned) per out-channel tile
    };
    auto read_x = [&](Raw& r, unsigned xa, auto ks_) __attribute__((always_inline)) {
      constexpr int KS = decltype(ks_)::value;
      rw_static_for<CT>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        if constexpr (UPS) {
          constexpr int o = (16 * i * CSX + 4 * KS) * 4;
          if constexpr (!ODD) {
            r.ua[i][0] = rw_lds32<o + UA * RS * 4>(xa);
            r.ua[i][2] = rw_lds32<o + UA * RS * 4 + 8>(xa);
          }
          r.ua[i][1] = rw_lds32<o + UA * RS * 4 + 4>(xa);
          if constexpr (I != 1) {
            if constexpr (!ODD) {
              r.ub[i][0] = rw_lds32<o + UB * RS * 4>(xa);
              r.ub[i][2] = rw_lds32<o + UB * RS * 4 + 8>(xa);
            }
            r.ub[i][1] = rw_lds32<o + UB * RS * 4 + 4>(xa);
          }
        } else {
          constexpr int o = (16 * i * CSX + 8 * KS) * 4;
          r.al[i] = rw_lds64<o + RA * RS * 4>(xa);
          r.ah[i] = rw_lds64<o + RA * RS * 4 + 8>(xa);
          r.bl[i] = rw_lds64<o + RB * RS * 4>(xa);
          r.bh[i] = rw_lds64<o + RB * RS * 4 + 8>(xa);
        }
      });
    };
    auto read_y = [&](Raw& r, unsigned ya, auto ks_) __attribute__((always_inline)) {
      constexpr int KS = decltype(ks_)::value;
      rw_static_for<OT>([&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        constexpr int o = (16 * j * RW_CSY + 8 * KS) * 4;
        if constexpr (Y0) r.t0[j] = rw_lds64<o>(ya);
        if constexpr (Y1) r.t1[j] = rw_lds64<o + 128>(ya);
      });
    };
    auto wait_raw = [&](Raw& r) __attribute__((always_inline)) {
      rw_lds_wait();
#pragma unroll
      for (int i = 0; i < CT; ++i) {
        if constexpr (UPS) {
          if constexpr (!ODD) { rw_tie(r.ua[i][0]); rw_tie(r.ua[i][2]); }
          rw_tie(r.ua[i][1]);
          if constexpr (I != 1) {
            if constexpr (!ODD) { rw_tie(r.ub[i][0]); rw_tie(r.ub[i][2]); }
            rw_tie(r.ub[i][1]);
          }
        } else {
          rw_tie(r.al[i]); rw_tie(r.ah[i]); rw_tie(r.bl[i]); rw_tie(r.bh[i]);
        }
      }
#pragma unroll
      for (int j = 0; j < OT; ++j) {
        if constexpr (Y0) rw_tie(r.t0[j]);
        if constexpr (Y1) rw_tie(r.t1[j]);
      }
    };
    // raw rows -> MFMA operands
    auto transform_x = [&](const Raw& r, Ops& o) __attribute__((always_inline)) {
      if constexpr (UPS) {
#pragma unroll
        for (int i = 0; i < CT; ++i) {
          float uL = 0.f, uC, uR = 0.f;
          if constexpr (I == 1) {
            uC = r.ua[i][1];
            if constexpr (!ODD) { uL = r.ua[i][0]; uR = r.ua[i][2]; }
          } else {
            uC = r.ua[i][1] - r.ub[i][1];
            if constexpr (!ODD) { uL = r.ua[i][0] - r.ub[i][0]; uR = r.ua[i][2] - r.ub[i][2]; }
          }
          if constexpr (!ODD) o.av[i] = f32x2{uL - uC, uC - uR};
          else o.av[i] = f32x2{uC, 0.f};
        }
        return;
      }
#pragma unroll
      for (int i = 0; i < CT; ++i) {
        const f32x2 ul = PLUS ? r.al[i] + r.bl[i] : pk_sub(r.al[i], r.bl[i]);  // (u0, u1)
        const f32x2 uh = PLUS ? r.ah[i] + r.bh[i] : pk_sub(r.ah[i], r.bh[i]);  // (u2, u3)
        if constexpr (!ODD) asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(o.av[i]) : "v"(ul), "v"(uh));  // (u0 - u2, u1 - u3)
        else asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,0] neg_lo:[0,0] neg_hi:[1,0]" : "=v"(o.av[i]) : "v"(ul), "v"(uh));  // (u1 + u2, u2 - u1)
      }
    };
    auto transform_y = [&](const Raw& r, Ops& o, bool bias_on) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < OT; ++j) {
        f32x2 rr;
        if constexpr (I == 0) rr = r.t0[j];
        else if constexpr (I == 1) rr = r.t0[j] + r.t1[j];
        else if constexpr (I == 2) rr = pk_sub(r.t0[j], r.t1[j]);
        else rr = r.t1[j];
        if constexpr (I == 1 && !ODD) {
          if (bias_on) bsum[j] += rr[0] + rr[1];  // t00 + t10 + t01 + t11: the bias gradient rides in wave 2
        }
        if constexpr (!ODD) o.bv[j] = rr;
        else asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_lo:[0,0] neg_hi:[0,1]" : "=v"(o.bv[j]) : "v"(rr));  // (r0 + r1, r0 - r1)
      }
    };
    // (gfx950: registers written by vector instructions inside inline assembly and read as MFMA sources right behind them need wait
    // states hipcc only inserts for instructions it schedules itself -- wino_strip.hip; the fence names them)
    auto fence = [&](Ops& o) __attribute__((always_inline)) {
      if constexpr (CT == 1) asm volatile("s_nop 1" : "+v"(o.av[0]));
      if constexpr (CT == 2) asm volatile("s_nop 1" : "+v"(o.av[0]), "+v"(o.av[1]));
      if constexpr (CT == 3) asm volatile("s_nop 1" : "+v"(o.av[0]), "+v"(o.av[1]), "+v"(o.av[2]));
      if constexpr (CT == 4) asm volatile("s_nop 1" : "+v"(o.av[0]), "+v"(o.av[1]), "+v"(o.av[2]), "+v"(o.av[3]));
      if constexpr (OT == 1) asm volatile("" : "+v"(o.bv[0]));
      if constexpr (OT == 2) asm volatile("" : "+v"(o.bv[0]), "+v"(o.bv[1]));
      if constexpr (OT == 3) asm volatile("" : "+v"(o.bv[0]), "+v"(o.bv[1]), "+v"(o.bv[2]));
      if constexpr (OT == 4) asm volatile("" : "+v"(o.bv[0]), "+v"(o.bv[1]), "+v"(o.bv[2]), "+v"(o.bv[3]));
    };
    // MFMAs LO .. HI - 1 of a k-step, n = (p CT + i) OT + j
    constexpr int NMF = NP * CT * OT;
    auto mma = [&](const Ops& o, auto lo_, auto hi_) __attribute__((always_inline)) {
      constexpr int LO = decltype(lo_)::value, HI = decltype(hi_)::value;
      rw_static_for<HI - LO>([&](auto nc) __attribute__((always_inline)) {
        constexpr int n = LO + decltype(nc)::value;
        constexpr int p = n / (CT * OT), i = (n / OT) % CT, j = n % OT;
        acc[p][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(o.av[i][p], o.bv[j][p], acc[p][i][j], 0, 0, 0);
      });
      __builtin_amdgcn_sched_barrier(0);
    };
    // One k-step.  Its MFMAs carry, in their shadow, the operand reads and the transform of the NEXT k-step (vector and LDS
    // instructions issued right behind an MFMA of the same wave cost 2-4 cycles each instead of 8.5, tools/hwtests/
    // valu_latency_under_mfma.hip; in a phase of their own both waves of a SIMD sit in it at the same time and the matrix pipe idles:
    // measured, 24 % of the kernel).  The LAST k-step of a stage also carries the stage change: wait for the own pieces of the next
    // stage, barrier, request the stage after it into the buffer just left -- all between its first MFMAs and the reads.
    constexpr int C1 = NMF / 4, C2 = (3 * NMF) / 8, C3 = NMF / 2, C4 = (3 * NMF) / 4, C5 = (7 * NMF) / 8;
    using N0_ = std::integral_constant<int, 0>; using N1_ = std::integral_constant<int, C1>; using N2_ = std::integral_constant<int, C2>;
    using N3_ = std::integral_constant<int, C3>; using N4_ = std::integral_constant<int, C4>; using N5_ = std::integral_constant<int, C5>;
    using N6_ = std::integral_constant<int, NMF>;
    auto step = [&](const Ops& cur, Ops& nxt, Raw& r, unsigned xa, unsigned ya, auto nks_, bool bias_on, auto&& between) __attribute__((always_inline)) {
      if constexpr (IDLE) {  // (copies its share of the stages and keeps the barriers; its accumulators stay zero)
        between();
        return;
      }
      mma(cur, N0_{}, N1_{});
      between();
      __builtin_amdgcn_sched_barrier(0);
      mma(cur, N1_{}, N2_{});
      read_x(r, xa, nks_);
      __builtin_amdgcn_sched_barrier(0);
      mma(cur, N2_{}, N3_{});
      read_y(r, ya, nks_);
      __builtin_amdgcn_sched_barrier(0);
      mma(cur, N3_{}, N4_{});
      wait_raw(r);
      transform_x(r, nxt);
      __builtin_amdgcn_sched_barrier(0);
      mma(cur, N4_{}, N5_{});
      transform_y(r, nxt, bias_on);
      fence(nxt);
      __builtin_amdgcn_sched_barrier(0);
      mma(cur, N5_{}, N6_{});
    };

    using K0 = std::integral_constant<int, 0>; using K1 = std::integral_constant<int, 1>;
    using K2 = std::integral_constant<int, 2>; using K3 = std::integral_constant<int, 3>;
    // the image of a stage (bias gradient: images below bias_n count)
    const int per_img = a.blocks_x * a.blocks_y;
    int img = (split * a.per) / per_img, img_left = per_img - (split * a.per) % per_img;
    const bool staging = !(a.TBN & 2);
    Raw r;
    Ops o0, o1;
    // prologue: stage 0 in buffer 0, stage 1 on its way into buffer 1, the operands of stage 0's first k-step
    issue_stage(0);
    landed(0);
    __syncthreads();
    if (a.per > 1 && staging) issue_stage(STG);
    if constexpr (!IDLE) {
      read_x(r, xrd_a, K0{});
      read_y(r, yrd_a, K0{});
      wait_raw(r);
      transform_x(r, o0);
      transform_y(r, o0, img < a.bias_n);
      fence(o0);
    }
    __builtin_amdgcn_sched_barrier(0);
    for (int q = 0; q < a.per; ++q) {
      const int so = (q & 1) * STG, sn = STG - so;
      const unsigned xa = xrd_a + (unsigned)so * 4u, ya = yrd_a + (unsigned)so * 4u;
      const unsigned xn = xrd_a + (unsigned)sn * 4u, yn = yrd_a + (unsigned)sn * 4u;
      const bool bias_on = img < a.bias_n;
      const bool dma = staging && q > 0 && q + 1 < a.per;  // stage q + 1 is being copied: its slots 2 .. go out under k-steps 0 .. 2
      step(o0, o1, r, xa, ya, K1{}, bias_on, [&]() __attribute__((always_inline)) { if (dma) issue_slots(M2_{}, M4_{}); });
      step(o1, o0, r, xa, ya, K2{}, bias_on, [&]() __attribute__((always_inline)) { if (dma) issue_slots(M4_{}, M6_{}); });
      step(o0, o1, r, xa, ya, K3{}, bias_on, [&]() __attribute__((always_inline)) { if (dma) issue_slots(M6_{}, M8_{}); });
      if (--img_left == 0) { img_left = per_img; ++img; }
      step(o1, o0, r, xn, yn, K0{}, q + 1 < a.per && img < a.bias_n, [&]() __attribute__((always_inline)) {  // (behind the last stage: stale LDS, unused)
        if (staging && !(a.TBN & 8)) landed(sn);  // stage q + 1: this wave's pieces are in LDS (and its edge pixels zeroed)
        if (!(a.TBN & 4)) __syncthreads();       // ... everybody's; and nobody reads buffer `so` any more
        if (staging && q + 2 < a.per) {          // stage q + 2: its first copy instructions
          issue_begin(so);
          issue_slots(M0_{}, M2_{});
        }
      });
    }
    // signs of the gy components computed unsigned: (i, 3) for i < 3, (3, 0), (3, 1), (3, 2)
    // (UPS: x 2 for component row 1, x 2 for column 1 -- the transforms above leave those factors out)
    constexpr float F0 = UPS ? (I == 1 ? 2.f : 1.f) * (ODD ? 2.f : 1.f) : 1.f, F1 = UPS ? (I == 1 ? 2.f : 1.f) : 1.f;
    constexpr float S0 = (I == 3 ? -1.f : 1.f) * F0;                                  // p = 0: column 0 (even) / 1 (odd)
    constexpr float S1 = (ODD ? (I == 3 ? -1.f : 1.f) : (I == 3 ? 1.f : -1.f)) * F1;  // p = 1: column 3 (even) / 2 (odd)
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
      for (int j = 0; j < OT; ++j) {
        if constexpr (S0 != 1.f) acc[0][i][j] = acc[0][i][j] * S0;
        if constexpr (S1 != 1.f && NP == 2) acc[1][i][j] = acc[1][i][j] * S1;
      }
  };
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
  // component pair of this wave: rw = 2 i + parity.  UPS: row 2 is idle and an odd wave has half the work, and waves w and w + 4 of a
  // workgroup share a SIMD (MI355X_MICROARCH.md: cyclic placement), so the pairs there are (row even, row odd) for rows 0, 1, 3 and
  // (idle, idle): three component-units on three SIMDs instead of four on each
  const int rw = UPS ? 2 * ((wave & 3) == 2 ? 3 : ((wave & 3) == 3 ? 2 : (wave & 3))) + (wave >> 2) : wave;
  switch (rw) {
    case 0: tile_loop(I0{}, std::false_type{}); break;
    case 1: tile_loop(I0{}, std::true_type{}); break;
    case 2: tile_loop(I1{}, std::false_type{}); break;
    case 3: tile_loop(I1{}, std::true_type{}); break;
    case 4: tile_loop(I2{}, std::false_type{}); break;
    case 5: tile_loop(I2{}, std::true_type{}); break;
    case 6: tile_loop(I3{}, std::false_type{}); break;
    default: tile_loop(I3{}, std::true_type{}); break;
  }

  // slab of this split: G^T M G per (c, o) -- wino_wgrad_mfma's pass, the same accumulator layout
  float* G = smem;  // [slot 16][cc 32][o 64]
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        const int i = 2 * h + ii;
        if (i < CT) {
#pragma unroll
          for (int j = 0; j < OT; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g)
              G[((2 * rw + p) * 32 + ii * 16 + rq * 4 + g) * 64 + ((j ^ rq) * 16 + col)] = acc[p][i][j][g];
        }
      }
    __syncthreads();
    constexpr int SL[4] = {0, 2, 3, 1};
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) {
      const int cc = (tid >> 6) + 8 * k4;
      const int ol = tid & 63;
      const int i = 2 * h + (cc >> 4);
      const int c = c0 + i * 16 + (cc & 15), o = o0 + ol;
      if (i < CT && ol < OT * 16 && c < a.CinP && o < a.CoutP) {
        const int osw = ((ol >> 4) ^ ((cc >> 2) & 3)) * 16 + (ol & 15);
        float M[4][4];
#pragma unroll
        for (int xi = 0; xi < 4; ++xi)
#pragma unroll
          for (int nu = 0; nu < 4; ++nu) M[xi][nu] = G[((4 * xi + SL[nu]) * 32 + cc) * 64 + osw];
        float hh[3][4];
#pragma unroll
        for (int nu = 0; nu < 4; ++nu) {
          hh[0][nu] = M[0][nu] + 0.5f * (M[1][nu] + M[2][nu]);
          hh[1][nu] = 0.5f * (M[1][nu] - M[2][nu]);
          hh[2][nu] = 0.5f * (M[1][nu] + M[2][nu]) + M[3][nu];
        }
        float* sl = a.slab + (size_t)split * 9 * a.CinP * a.CoutP + (size_t)c * a.CoutP + o;
        const size_t plane = (size_t)a.CinP * a.CoutP;
#pragma unroll
        for (int aa = 0; aa < 3; ++aa) {
          sl[(size_t)(aa * 3 + 0) * plane] = hh[aa][0] + 0.5f * (hh[aa][1] + hh[aa][2]);
          sl[(size_t)(aa * 3 + 1) * plane] = 0.5f * (hh[aa][1] - hh[aa][2]);
          sl[(size_t)(aa * 3 + 2) * plane] = 0.5f * (hh[aa][1] + hh[aa][2]) + hh[aa][3];
        }
      }
    }
  }
  // bias gradient: the wave of component pair 2 holds, per out-channel tile, lane (rq, col) = its tiles' sums of channel 16 j + col
  if (rw == 2 && cb == 0) {
#pragma unroll
    for (int j = 0; j < OT; ++j) {
      float v = bsum[j];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (rq == 0 && o0 + 16 * j + col < a.CoutP) a.slab_b[(size_t)split * a.CoutP + o0 + 16 * j + col] = v;
    }
  }
}

}  // namespace

int mg_ww_launch_rows(int CT, int OT, bool ups, bool, const WwArgs& a, dim3 grid, hipStream_t s) {
  return ww_for_tiles(CT, OT, [&](auto ct, auto ot) -> int {
    constexpr int C = decltype(ct)::value, O = decltype(ot)::value;
    if constexpr (C != 4 || O != 4) {  // ((4, 4) would keep accumulators in scratch: not instantiated, ww_rows_takes)
      return ww_for_flags(ups, false, [&](auto u, auto) {
        constexpr bool U = decltype(u)::value;
        return ww_launch<wino_wgrad_rows_mfma<C, O, U>>("mg_wino3x3_wgrad (rows)", RwGeom<C, O, U>::lds_bytes(), a, grid, s);
      });
    }
    return WW_NO_TILE;
  });
}
