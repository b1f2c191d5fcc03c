// Weight gradient of the 3x3 / stride 1 / pad 1 convolution in Winograd F(3x3, 2x2) form on the fp32 matrix cores of gfx950
// (aten::convolution_backward, weight + bias grads, of nn.Conv2d(3x3) in /root/reference/music_gan/networks/generator.py:9-40 and
// discriminator.py:8-34).  For every 2x2 tile of the output gradient t and the 4x4 input patch d around it
//
//   dW (3x3)  =  G^T [ sum_tiles (A t A^T) .* (B^T d B) ] G        B^T, G: the matrices of wino3x3.hip;  A = (A^T)^T  (4x2)
//
// (the transposed F(2x2,3x3) algorithm: same input transform as the forward pass), i.e. 16 multiplies per tile and channel pair
// instead of 36.  Per Winograd component xi the sum over tiles is a GEMM  M_xi[c, o] = sum_tile V_xi[tile, c] * Y_xi[tile, o]:
//   M (A rows) = in-channels  (CT tiles of 16),  N (B cols) = out-channels (OT tiles of 16),  K = tiles, 8 per LDS chunk
//   (two MFMA k-steps: lane k-index rq holds tiles 2rq and 2rq+1 of the chunk)
// One workgroup of 8 waves owns a (CT*16) x (OT*16) block of ALL 16 components -- wave w accumulates component pair w, 2*CT*OT
// accumulator tiles -- over a slab of tiles (split-K over workgroups); both operands are transformed on the way from HBM to LDS
// (x: coalesced 8-byte row loads + DPP halo exchange + packed adds exactly as in wino3x3.hip; gy: two 8-byte loads), the LDS
// stages are double-buffered with one barrier per chunk, G^T . G is applied per slab (the components of a channel pair meet in LDS
// once the tile loop is done), and a second kernel sums the 9-tap slabs in a fixed order
// (bitwise deterministic, no float atomics).  The bias gradient rides along in the gy staging threads.
// The narrow block shapes and the row-staged form live in wino_wgrad_narrow.hip and wino_wgrad_rows.hip, the launch planner in
// wino_wgrad_plan.h (plain host C++), what they share in wino_wgrad.h.
#include <cstdlib>

#include "wino_wgrad.h"

namespace {

// UPS: x is (N, Cin, H/2, W/2) and the convolution input is its nearest x2 up-sampling (generator.py:24-25): the 4x4 patch of tile
// (TY, TX) is then the 3x3 low-res neighbourhood with the centre row / column doubled -- one dword per row and lane.
// The body takes its block coordinates as arguments: `split` (slab index, blockIdx.x of a single-layer launch) and `yblk`
// (channel block pair, blockIdx.y) -- a grouped launch (wino_wgrad_group_mfma below) derives them from a table instead.
// FAST: chunks of 8 x 1 x 1 tiles on maps whose width is a multiple of 16 (every layer from 16x16 maps up): which rows and halo pixels
// of a chunk exist is then the same for all its lanes, so a lane's byte offset is fixed for the kernel (+ one add of the chunk's
// column), rows travel in the scalar offset, and a row / chunk outside the tensor is read through a descriptor of zero records --
// the general form spends ~45 of its ~115 vector instructions per chunk and wave on per-lane predicates and offsets.
template <int CT, int OT, bool UPS, bool FAST = false>
__device__ __forceinline__ void ww_body(const WwArgs& a, const int split, const int yblk) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // = component pair
  const int col = lane & 15, rq = lane >> 4;
  const int cb = yblk / a.nob, ob = yblk % a.nob;
  const int c0 = cb * CT * 16, o0 = ob * OT * 16;
  const int HW = a.H * a.W;
  const int Ht = a.H >> 1, Wt = a.W >> 1;

  // staging item of this thread: tile t of the chunk, channel slot chs: x channel c0 + chs and gy channel o0 + chs
  const int t = tid & 7, chs = tid >> 3;
  const int txl = t & (a.TBW - 1);
  const int tyl = (t >> a.lgTBW) & (a.TBH - 1);
  const int nl = t >> (a.lgTBW + a.lgTBH);
  const bool xch = (chs < CT * 16) && (c0 + chs < a.Cin);
  const bool ych = (chs < OT * 16) && (o0 + chs < a.Cout);
  const bool ledge = txl == 0, redge = txl == a.TBW - 1;
  const int HWx = UPS ? Ht * Wt : HW;
  const int xlane = UPS ? (nl * a.Cin + c0 + chs) * HWx + tyl * Wt + txl             // low-res pixel (TY, TX)
                        : (nl * a.Cin + c0 + chs) * HWx + (2 * tyl - 1) * a.W + 2 * txl;  // patch row 0, own pair
  const int ylane = (nl * a.Cout + o0 + chs) * HW + (2 * tyl) * a.W + 2 * txl;
  // LDS float offset of the item's first component pair: [cp][tile pair t>>1][swizzled channel][k-step t&1][parity]
  const int ldst = ((t >> 1) * CH + (chs ^ ((t >> 1) << 1))) * 4 + (t & 1) * 2;

  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.gy), 0, (int)a.gy_bytes, 0x00020000);
  // FAST: lane parts of the byte offsets (channel plane + own pixel pair inside the chunk's 16 pixels); out of range = no such channel
  const unsigned fxP = xch ? (unsigned)(((c0 + chs) * HWx + (UPS ? t : 2 * t)) * 4) : 0x80000000u;
  const unsigned fyP = ych ? (unsigned)(((o0 + chs) * HW + 2 * t) * 4) : 0x80000000u;
  const int fdelta = t == 0 ? -4 : (UPS ? 4 : 8);  // halo pixel of an edge lane relative to its own pair

  f32x4 acc[2][CT][OT];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
      for (int j = 0; j < OT; ++j) acc[p][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x2 rP[4], rG[2];
  float rE[4];  // halo column of an edge lane (left OR right: a lane is at most one; a 1-tile-wide chunk has both outside)
  float bsum = 0.f;
  bool bnext = false;  // whether the gy tile in flight counts for the bias gradient

  // chunk `blk` (8 tiles): global loads into registers; tiles / rows / columns outside the image get an out-of-range offset and
  // read back as 0.0
  // the chunks of a slab are consecutive tile blocks: (bx, by, bn) of the next chunk to request is carried along (scalar selects)
  // instead of being divided out of the chunk index for every chunk (~80 scalar instructions per chunk and wave)
  int nq = 0, bx, by, bn;
  {
    const int b0 = split * a.per;
    bx = b0 % a.blocks_x;
    const int t2 = b0 / a.blocks_x;
    by = t2 % a.blocks_y;
    bn = t2 / a.blocks_y;
  }
  auto load_chunk = [&]() {  // the slab's next chunk (all-zero once past its end)
    const int blk = nq < a.per ? split * a.per + nq : a.nblk;
    if constexpr (FAST) {
      // scalar: the chunk is tile row `by` of image `bn`, tiles 8 bx .. 8 bx + 7
      const bool ok = blk < a.nblk;
      const unsigned vP = fxP + (unsigned)((UPS ? 8 : 16) * bx * 4);
      const bool ev = t == 0 ? bx > 0 : bx < a.blocks_x - 1;
      const unsigned vE = (xch && (t == 0 || t == 7) && ev) ? vP + (unsigned)fdelta : 0x80000000u;
      constexpr int NR = UPS ? 3 : 4;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const bool rv = ok && (r == 0 ? by > 0 : (r == NR - 1 ? by < Ht - 1 : true));
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, rv ? (int)a.x_bytes : 0, 0x00020000);
        const int so = UPS ? ((bn * a.Cin) * HWx + (by - 1 + r) * Wt) * 4 : ((bn * a.Cin) * HWx + (2 * by - 1 + r) * a.W) * 4;
        if constexpr (UPS) {
          const float v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)vP, so, 0));
          const float ve = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)vE, so, 0));
          const int rr = r == 0 ? 0 : (r == 1 ? 1 : 3);
          rP[rr] = f32x2{v, v};
          rE[rr] = ve;
          if (r == 1) { rP[2] = f32x2{v, v}; rE[2] = ve; }
        } else {
          rP[r] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)vP, so, 0));
          rE[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)vE, so, 0));
        }
      }
      const __amdgpu_buffer_rsrc_t ys = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.gy), 0, ok ? (int)a.gy_bytes : 0, 0x00020000);
      const unsigned vY = fyP + (unsigned)(16 * bx * 4);
      const int sy = ((bn * a.Cout) * HW + (2 * by) * a.W) * 4;
      rG[0] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(ys, (int)vY, sy, 0));
      rG[1] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(ys, (int)vY, sy + a.W * 4, 0));
      bnext = bn < a.bias_n;
      ++nq;
      ++bx;
      const int wx = bx == a.blocks_x ? 1 : 0;
      bx = wx ? 0 : bx;
      by += wx;
      const int wy = by == a.blocks_y ? 1 : 0;
      by = wy ? 0 : by;
      bn += wy;
      return;
    }
    const int n = bn * a.TBN + nl, TY = by * a.TBH + tyl, TX = bx * a.TBW + txl;
    const bool ok = (blk < a.nblk) && (n < a.N) && (TY < Ht) && (TX < Wt);
    const int ux = UPS ? (bn * a.TBN * a.Cin) * HWx + (by * a.TBH) * Wt + bx * a.TBW
                       : (bn * a.TBN * a.Cin) * HWx + (2 * by * a.TBH) * a.W + 2 * bx * a.TBW;
    const int uy = (bn * a.TBN * a.Cout) * HW + (2 * by * a.TBH) * a.W + 2 * bx * a.TBW;
    const unsigned xo = (unsigned)(xlane + ux) * 4u;
    const bool xok = ok && xch;
    if constexpr (UPS) {
#pragma unroll
      for (int r3 = 0; r3 < 3; ++r3) {  // low-res rows TY-1, TY, TY+1 -> patch rows 0, (1, 2), 3
        const bool rv = xok && (r3 == 1 || (r3 == 0 ? TY > 0 : TY < Ht - 1));
        const unsigned o = xo + (unsigned)((r3 - 1) * Wt) * 4u;
        const float v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, (int)(rv ? o : 0x80000000u), 0, 0));
        const unsigned oe = (rv && ledge && TX > 0) ? o - 4u : ((rv && redge && TX < Wt - 1) ? o + 4u : 0x80000000u);
        const float ve = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, (int)oe, 0, 0));
        const int r = r3 == 0 ? 0 : (r3 == 1 ? 1 : 3);
        rP[r] = f32x2{v, v};
        rE[r] = ve;
        if (r3 == 1) { rP[2] = f32x2{v, v}; rE[2] = ve; }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool rv = xok && (r == 1 || r == 2 || (r == 0 ? TY > 0 : TY < Ht - 1));
        const unsigned o = xo + (unsigned)(r * a.W) * 4u;
        rP[r] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(xrs, (int)(rv ? o : 0x80000000u), 0, 0));
        const unsigned oe = (rv && ledge && TX > 0) ? o - 4u : ((rv && redge && TX < Wt - 1) ? o + 8u : 0x80000000u);
        rE[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, (int)oe, 0, 0));
      }
    }
    const unsigned yo = (unsigned)(ylane + uy) * 4u;
    const bool yok = ok && ych;
    rG[0] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(yrs, (int)(yok ? yo : 0x80000000u), 0, 0));
    rG[1] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(yrs, (int)(yok ? yo + (unsigned)a.W * 4u : 0x80000000u), 0, 0));
    bnext = n < a.bias_n;
    ++nq;
    ++bx;
    const int wx = bx == a.blocks_x ? 1 : 0;
    bx = wx ? 0 : bx;
    by += wx;
    const int wy = by == a.blocks_y ? 1 : 0;
    by = wy ? 0 : by;
    bn += wy;
  };

  // registers -> transformed operand images of one stage
  auto store_chunk = [&](float* st) {
    {  // V = B^T d B, component slots of row i: [v0, v3 | v1, v2]  (see wino3x3.hip)
      f32x2 E[4], P[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        P[r] = rP[r];
        const float own_x = rP[r][0], own_y = rP[r][1];
        const float fl = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, own_y), 0x138, 0xf, 0xf, false));  // lane-1
        const float fr = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, own_x), 0x130, 0xf, 0xf, false));  // lane+1
        E[r] = f32x2{ledge ? (a.TBW > 1 ? rE[r] : 0.f) : fl, redge ? (a.TBW > 1 ? rE[r] : 0.f) : fr};
      }
      // one v_pk_add_f32 per result pair, swaps and negations in the operand modifiers (hipcc builds them with v_mov / v_xor)
      f32x2 UE[4], UP[4];
      UE[0] = pk_sub(E[0], E[2]);  UP[0] = pk_sub(P[0], P[2]);
      UE[1] = E[1] + E[2];         UP[1] = P[1] + P[2];
      UE[2] = pk_sub(E[2], E[1]);  UP[2] = pk_sub(P[2], P[1]);
      UE[3] = pk_sub(E[1], E[3]);  UP[3] = pk_sub(P[1], P[3]);
      float* dst = st + ldst;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x2 v03, v12;
        asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[1,0]" : "=v"(v03) : "v"(UE[i]), "v"(UP[i]));  // (e0 - p1, p0 - e1)
        asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,0] neg_hi:[0,1]" : "=v"(v12) : "v"(UP[i]));             // (p0 + p1, p1 - p0)
        *reinterpret_cast<f32x2*>(dst + (2 * i) * (4 * CH * 4)) = v03;
        *reinterpret_cast<f32x2*>(dst + (2 * i + 1) * (4 * CH * 4)) = v12;
      }
    }
    {  // Y = A t A^T with A = [[1,0],[1,1],[1,-1],[0,-1]], same slot order: row i -> [y0, y3 | y1, y2]
      const f32x2 t0 = rG[0], t1 = rG[1];
      if (bnext) bsum += (t0[0] + t0[1]) + (t1[0] + t1[1]);
      f32x2 R[4];
      R[0] = t0;
      R[1] = t0 + t1;
      R[2] = pk_sub(t0, t1);
      R[3] = t1;  // stands for -t1: the sign is folded into the modifiers below
      float* dst = st + IMG + ldst;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x2 y03, y12;
        if (i < 3) {
          asm("v_pk_mul_f32 %0, %1, %2 neg_hi:[1,0]" : "=v"(y03) : "v"(R[i]), "v"(f32x2{1.f, 1.f}));                               // (r0, -r1)
          asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_lo:[0,0] neg_hi:[0,1]" : "=v"(y12) : "v"(R[i]));           // (r0 + r1, r0 - r1)
        } else {
          asm("v_pk_mul_f32 %0, %1, %2 neg_lo:[1,0]" : "=v"(y03) : "v"(R[i]), "v"(f32x2{1.f, 1.f}));                               // (-t0, t1)
          asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_lo:[1,1] neg_hi:[1,0]" : "=v"(y12) : "v"(R[i]));           // (-t0 - t1, -t0 + t1)
        }
        *reinterpret_cast<f32x2*>(dst + (2 * i) * (4 * CH * 4)) = y03;
        *reinterpret_cast<f32x2*>(dst + (2 * i + 1) * (4 * CH * 4)) = y12;
      }
    }
  };

  // The operand reads of a chunk are issued first (pinned by a scheduling fence), the next chunk's transform + LDS writes and
  // the loads of the one after run while they are in flight, and the MFMAs come last: +1..3 % over reads placed directly in
  // front of the MFMAs, where the matrix pipe waits out an LDS round trip per chunk.
  f32x4 av[CT], bv[OT];  // {par0 k0, par1 k0, par0 k1, par1 k1}
  auto read_operands = [&](const float* st) {
    const float* vb = st + (wave * 4 + rq) * (CH * 4);
    const float* yb = vb + IMG;
#pragma unroll
    for (int i = 0; i < CT; ++i) av[i] = *reinterpret_cast<const f32x4*>(vb + ((i * 16 + col) ^ (rq << 1)) * 4);
#pragma unroll
    for (int j = 0; j < OT; ++j) bv[j] = *reinterpret_cast<const f32x4*>(yb + ((j * 16 + col) ^ (rq << 1)) * 4);
  };
  auto mma_chunk = [&]() {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int i = 0; i < CT; ++i)
#pragma unroll
          for (int j = 0; j < OT; ++j)
            acc[p][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][ks * 2 + p], bv[j][ks * 2 + p], acc[p][i][j], 0, 0, 0);
  };

  // pipeline: iteration q computes chunk q from stage q&1, writes chunk q+1 (registers) into the other stage and issues the
  // loads of chunk q+2; chunks past the slab (or past the tensor) are all-zero and add nothing
  load_chunk();
  store_chunk(smem);
  load_chunk();
  __syncthreads();
  for (int q = 0; q < a.per; ++q) {
    float* cur = smem + (q & 1) * STAGE;
    float* nxt = smem + ((q + 1) & 1) * STAGE;
    read_operands(cur);
    __builtin_amdgcn_sched_barrier(0);
    store_chunk(nxt);
    load_chunk();
    mma_chunk();
    __syncthreads();
  }

  // Slab of this split: dW_split = G^T M G per (c, o), 9 planes [split][k][c][o] -- the transform is linear, so it is applied per
  // split and the reduce kernel only sums (9/16 of the bytes, which is what the small-map layers' weight gradients cost: their
  // slabs are larger than their inputs).  A (c, o) pair's 16 components sit in 8 different waves: they meet in LDS (the two
  // stages are free now), 32 in-channels x 64 out-channels x 16 slots = exactly its 128 KB, in two passes over the in-channel
  // tiles; the out-channel tile index is XOR-ed with the row group so that the four row groups of a wave hit disjoint banks.
  float* G = smem;  // [slot 16][cc 32][o 64]
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();  // MFMA loop / previous pass done with the buffer
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
              G[((2 * wave + p) * 32 + ii * 16 + rq * 4 + g) * 64 + ((j ^ rq) * 16 + col)] = acc[p][i][j][g];
        }
      }
    __syncthreads();
    constexpr int SL[4] = {0, 2, 3, 1};  // slot of column nu within a row of components
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) {
      const int cc = (tid >> 6) + 8 * k4;  // wave-uniform row of the half block
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
        float hh[3][4];  // G^T M
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
  // bias gradient: the 8 tile lanes of a channel slot, then one value per (split, out-channel); in-channel block 0 only
  bsum += __shfl_xor(bsum, 1);
  bsum += __shfl_xor(bsum, 2);
  bsum += __shfl_xor(bsum, 4);
  if (cb == 0 && t == 0 && chs < OT * 16 && o0 + chs < a.CoutP) a.slab_b[(size_t)split * a.CoutP + o0 + chs] = bsum;
}

template <int CT, int OT, bool UPS, bool FAST>
__global__ void __launch_bounds__(512) wino_wgrad_mfma(const WwArgs a) {
  ww_body<CT, OT, UPS, FAST>(a, blockIdx.x, blockIdx.y);
}

// ---- several layers in ONE launch.  At small batch / on small maps a layer's weight gradient is a 10-30 us launch of a few dozen
// to 256 workgroups, a step has ten of them back to back, and every one is split over ~256 workgroups just to fill the chip, each
// split writing (and the reduce re-reading) a full 9-tap slab of the filter.  The small layers of a sweep share a launch: workgroup
// b looks its layer up in a table of at most WW_GROUP entries (first[] = prefix sums of workgroups) and runs that layer's body --
// the block shapes <CT, OT, UPS> of layers that are ever small (>= 96 channels: 3 or 4 channel tiles per block) are all inlined
// here; the host sizes the splits so that the GROUP fills the chip once (mg_wino3x3_wgrad_partial_multi).
__global__ void __launch_bounds__(512) wino_wgrad_group_mfma(const WwGroup g) {
  int j = 0;
#pragma unroll 1
  while (j + 1 < g.n && (int)blockIdx.x >= g.first[j + 1]) ++j;
  const int local = (int)blockIdx.x - g.first[j];
  const int ns = g.nsplit[j];
  const int split = local % ns, yblk = local / ns;
  switch (g.var[j]) {
    case ww_var(3, 3, false): ww_body<3, 3, false>(g.a[j], split, yblk); break;
    case ww_var(3, 3, true): ww_body<3, 3, true>(g.a[j], split, yblk); break;
    case ww_var(3, 4, false): ww_body<3, 4, false>(g.a[j], split, yblk); break;
    case ww_var(3, 4, true): ww_body<3, 4, true>(g.a[j], split, yblk); break;
    case ww_var(4, 3, false): ww_body<4, 3, false>(g.a[j], split, yblk); break;
    case ww_var(4, 3, true): ww_body<4, 3, true>(g.a[j], split, yblk); break;
    case ww_var(4, 4, false): ww_body<4, 4, false>(g.a[j], split, yblk); break;
    case ww_var(4, 4, true): ww_body<4, 4, true>(g.a[j], split, yblk); break;
    default: break;
  }
}

// Sum the split-K slabs (already transformed to the 9 taps by the partial kernel) in a fixed order.  Block = EL consecutive (c, o)
// pairs x KL split-lanes, EL * KL = 512 (a thread sums every KL-th split of the 9 taps, four slabs of loads in flight: this is a
// pure latency problem), LDS-combined as a fixed tree => deterministic.  KL = 8 normally; 32 for the layers with few filter
// elements and hundreds of splits (16..48-channel layers on 256x256 / 512x512 maps): at 8 lanes their 8 workgroups walked 64 slabs
// each while the chip waited -- and their bias sum, 512 loads four at a time in ONE thread per out-channel, took 86 us at level 7.
// The bias gradient is summed the same way by the threads of in-channel 0.
template <int KL>
__device__ __forceinline__ void wino_wgrad_reduce_lanes(const float* __restrict__ slab, const float* __restrict__ slab_b, int nsplit,
                                                        float* __restrict__ gw, float* __restrict__ gb, int Cout, int Cin,
                                                        int CoutP, int CinP, int accumulate, int block, float (*red)[512]) {
  constexpr int EL = 512 / KL;
  const int el = threadIdx.x % EL, kl = threadIdx.x / EL;
  const int e = block * EL + el;  // e = c * CoutP + o over the padded block
  const int total = CinP * CoutP;
  float m[10];  // 9 taps + the bias gradient (threads of in-channel 0: e = o)
#pragma unroll
  for (int s = 0; s < 10; ++s) m[s] = 0.f;
  if (e < total) {
    // four slabs' worth of loads (36) in flight, then their adds in slab order: as a plain loop hipcc waits for each slab's nine
    // loads before it requests the next one -- nsplit / KL memory round trips in a row
    int k = kl;
    for (; k + 3 * KL < nsplit; k += 4 * KL) {
      float v[4][9];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* src = slab + (size_t)(k + KL * u) * 9 * total + e;
#pragma unroll
        for (int s = 0; s < 9; ++s) v[u][s] = src[(size_t)s * total];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int s = 0; s < 9; ++s) m[s] += v[u][s];
    }
    for (; k < nsplit; k += KL) {
      const float* src = slab + (size_t)k * 9 * total + e;
#pragma unroll
      for (int s = 0; s < 9; ++s) m[s] += src[(size_t)s * total];
    }
    if (gb != nullptr && e < CoutP) {  // c == 0: this thread's share of the bias slabs of out-channel o = e
      int kb = kl;
      for (; kb + 7 * KL < nsplit; kb += 8 * KL) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = slab_b[(size_t)(kb + KL * u) * CoutP + e];
#pragma unroll
        for (int u = 0; u < 8; ++u) m[9] += v[u];
      }
      for (; kb < nsplit; kb += KL) m[9] += slab_b[(size_t)kb * CoutP + e];
    }
  }
#pragma unroll
  for (int s = 0; s < 10; ++s) red[s][kl * EL + el] = m[s];
  __syncthreads();
  if (kl != 0 || e >= total) return;
  const int c = e / CoutP, o = e % CoutP;
  auto lanes = [&](int s) {  // fixed pairwise tree over the KL split-lanes
    float t[KL];
#pragma unroll
    for (int q = 0; q < KL; ++q) t[q] = red[s][q * EL + el];
#pragma unroll
    for (int w = 1; w < KL; w *= 2)
#pragma unroll
      for (int q = 0; q < KL; q += 2 * w) t[q] += t[q + w];
    return t[0];
  };
  if (c < Cin && o < Cout) {
    float* dst = gw + ((size_t)o * Cin + c) * 9;
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      const float w = lanes(s);
      dst[s] = accumulate ? dst[s] + w : w;
    }
  }
  if (gb != nullptr && c == 0 && o < Cout) {
    const float sb = lanes(9);
    gb[o] = accumulate ? gb[o] + sb : sb;
  }
}

__device__ __forceinline__ void wino_wgrad_reduce_body(const float* __restrict__ slab, const float* __restrict__ slab_b, int nsplit,
                                                       float* __restrict__ gw, float* __restrict__ gb, int Cout, int Cin,
                                                       int CoutP, int CinP, int accumulate, int block) {
  __shared__ float red[10][512];
  if (ww_reduce_lanes(nsplit, CinP * CoutP) == 32)
    wino_wgrad_reduce_lanes<32>(slab, slab_b, nsplit, gw, gb, Cout, Cin, CoutP, CinP, accumulate, block, red);
  else
    wino_wgrad_reduce_lanes<8>(slab, slab_b, nsplit, gw, gb, Cout, Cin, CoutP, CinP, accumulate, block, red);
}

// One launch for the reduce of SEVERAL layers (the weight-gradient sweep of an update ends with one of these per layer: 8 launches of
// ~20 us each, latency-bound, at level 5): jobs travel by value, blockIdx.y selects the job, blocks past a job's extent return.
__global__ void __launch_bounds__(512) wino_wgrad_reduce_multi(const WwJobs jobs) {
  // (a 2-D grid of "largest job x jobs" launched ~10x the workgroups a sweep needs: 19 us for the slabs of level 3)
  int i = 0;
#pragma unroll 1
  while (i + 1 < jobs.n && (int)blockIdx.x >= jobs.first[i + 1]) ++i;
  const mg_wgrad_job_t j = jobs.j[i];
  wino_wgrad_reduce_body(j.slab, j.slab_b, j.nsplit, j.gw, j.gb, j.Cout, j.Cin, j.CoutP, j.CinP, j.accumulate,
                         (int)blockIdx.x - jobs.first[i]);
}

int launch_wide(int CT, int OT, bool ups, bool fast, const WwArgs& a, dim3 grid, hipStream_t s) {  // CT + OT > 4
  return ww_for_tiles(CT, OT, [&](auto ct, auto ot) -> int {
    constexpr int C = decltype(ct)::value, O = decltype(ot)::value;
    if constexpr (C + O > 4) {  // (the others: mg_ww_launch_narrow)
      return ww_for_flags(ups, fast, [&](auto u, auto f) {
        return ww_launch<wino_wgrad_mfma<C, O, decltype(u)::value, decltype(f)::value>>("mg_wino3x3_wgrad", WW_LDS_WIDE, a, grid, s);
      });
    }
    return WW_NO_TILE;
  });
}

// The planner's switches from the environment.  Read per entry-point call: tests and A/B runs switch them inside one process.
WwSwitches ww_switches() {
  WwSwitches sw;
  int v;
  auto num = [&v](const char* name) {
    const char* e = getenv(name);
    if (e != nullptr) v = atoi(e);
    return e != nullptr;
  };
  if (num("MG_WGRAD_ROWS")) sw.rows = v;
  if (num("MG_WGRAD_ROWS_UPS")) sw.rows_ups = v != 0;
  if (num("MG_WGRAD_ROWS_ABLATE")) sw.ablate = v & 126;
  if (num("MG_WGRAD_FAST")) sw.fast = v != 0;
  if (num("MG_WGRAD_GROUP_FIXED") && v >= 0) sw.group_fixed = v;
  if (num("MG_WGRAD_GROUP_SLOTS") && v > 0) sw.group_slots_q = v;
  return sw;
}

int check_ww(const mg_wgrad_desc_t& d) {
  MG_CHECK_ARG(d.x && d.gy && d.gw && d.ws && d.N > 0 && d.Cin > 0 && d.Cout > 0 && d.H > 0 && d.W > 0, "mg_wino3x3_wgrad: bad arguments");
  MG_CHECK_ARG((d.H % 2 == 0) && (d.W % 2 == 0), "mg_wino3x3_wgrad: H=%d W=%d must be even", d.H, d.W);
  MG_CHECK_ARG(!(d.flags & ~MG_CONV_UPS_IN), "mg_wino3x3_wgrad: unknown flag");
  MG_CHECK_ARG((long long)d.N * d.Cin * d.H * d.W < (1ll << 29) && (long long)d.N * d.Cout * d.H * d.W < (1ll << 29),
               "mg_wino3x3_wgrad: tensor too large for 32-bit byte offsets");
  return MG_OK;
}

int plan_error() {  // (cannot happen: the row plan never has more blocks per channel block pair, the group plan clamps)
  mg_set_error("mg_wino3x3_wgrad: a layer was re-planned to more splits than its workspace is sized for");
  return MG_EWORKSPACE;
}

// final plan of a layer -> kernel arguments (pointers, byte limits)
WwArgs args_of(const WwPlan& pl, const mg_wgrad_desc_t& d) {
  const bool ups = (d.flags & MG_CONV_UPS_IN) != 0;
  WwArgs a;
  static_cast<WwGeo&>(a) = pl.a;
  a.x = d.x; a.gy = d.gy;
  a.slab = static_cast<float*>(d.ws);
  a.slab_b = a.slab + (size_t)pl.nsplit * 9 * a.CinP * a.CoutP;
  a.bias_n = (d.bias_n <= 0 || d.bias_n > d.N) ? d.N : d.bias_n;
  a.x_bytes = (unsigned)((size_t)d.N * d.Cin * (ups ? (d.H / 2) * (d.W / 2) : d.H * d.W) * 4);
  a.gy_bytes = (unsigned)((size_t)d.N * d.Cout * d.H * d.W * 4);
  return a;
}

int launch_single_ww(const WwPlan& pl, const WwArgs& a, bool ups, const WwSwitches& sw, hipStream_t s) {
  const dim3 grid(pl.nsplit, pl.ncb * pl.a.nob);
  if (pl.rows) return mg_ww_launch_rows(pl.CT, pl.OT, ups, false, a, grid, s);
  return (pl.CT + pl.OT <= 4 ? mg_ww_launch_narrow : launch_wide)(pl.CT, pl.OT, ups, ww_fast(pl.a, sw), a, grid, s);
}

}  // namespace

extern "C" int mg_wino3x3_wgrad_form(int N, int Cin, int Cout, int H, int W, int flags, int group_max_chunks) {
  if (N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (H % 2) || (W % 2)) return -1;
  return ww_form(N, Cin, Cout, H, W, (flags & MG_CONV_UPS_IN) != 0, group_max_chunks, mg_cu_count(), ww_switches());
}

extern "C" size_t mg_wino3x3_wgrad_ws_bytes(int N, int Cin, int Cout, int H, int W) {
  WwPlan pl;
  plan_ww(N, Cin, Cout, H, W, mg_cu_count(), pl);
  return pl.ws_floats * sizeof(float);
}

extern "C" int mg_wino3x3_wgrad_partial(const float* x, const float* gy, float* gw, float* gb, void* ws, size_t ws_bytes, int N,
                                        int Cin, int Cout, int H, int W, int flags, int accumulate, int bias_n,
                                        mg_wgrad_job_t* job, mg_stream_t stream) {
  MG_CHECK_ARG(job, "mg_wino3x3_wgrad: bad arguments");
  const mg_wgrad_desc_t d = {x, gy, gw, gb, ws, ws_bytes, N, Cin, Cout, H, W, flags, accumulate, bias_n};
  return mg_wino3x3_wgrad_partial_multi(&d, 1, 0, job, stream);  // a sweep of one layer, no grouping
}

extern "C" int mg_wino3x3_wgrad_partial_multi(const mg_wgrad_desc_t* d, int n, int group_max_chunks, mg_wgrad_job_t* jobs,
                                              mg_stream_t stream) {
  MG_CHECK_ARG(d && jobs && n > 0 && n <= WW_MAX_LAYERS, "mg_wino3x3_wgrad_partial_multi: bad arguments (n = %d, at most 64 layers)", n);
  hipStream_t s = (hipStream_t)stream;
  const int n_cu = mg_cu_count();
  const WwSwitches sw = ww_switches();
  WwSweep S;
  for (int i = 0; i < n; ++i) {
    const int rc = check_ww(d[i]);
    if (rc != MG_OK) return rc;
    WwPlan& pl = S.pl[i];
    const bool fits = ww_plan_layer(d[i].N, d[i].Cin, d[i].Cout, d[i].H, d[i].W, (d[i].flags & MG_CONV_UPS_IN) != 0, group_max_chunks,
                                    n_cu, sw, pl);
    if (d[i].ws_bytes < pl.ws_floats * sizeof(float)) {
      mg_set_error("mg_wino3x3_wgrad: workspace %zu < %zu bytes", d[i].ws_bytes, pl.ws_floats * sizeof(float));
      return MG_EWORKSPACE;
    }
    if (!fits) return plan_error();
  }
  if (!ww_plan_groups(S, n, n_cu, sw)) return plan_error();
  WwArgs a[WW_MAX_LAYERS];  // (the slab_b offset follows a layer's FINAL split count)
  for (int i = 0; i < n; ++i) a[i] = args_of(S.pl[i], d[i]);
  for (int gi = 0; gi < S.ngroups; ++gi) {
    WwGroup g;
    g.n = 0;
    g.first[0] = 0;
    for (int i = 0; i < n; ++i) {
      if (S.group_of[i] != gi) continue;
      const int k = g.n++;
      g.a[k] = a[i];
      g.nsplit[k] = S.pl[i].nsplit;
      g.var[k] = S.pl[i].var;
      g.first[k + 1] = g.first[k] + S.pl[i].nsplit * S.pl[i].ncb * S.pl[i].a.nob;
    }
    const int rc = ww_launch<wino_wgrad_group_mfma>("mg_wino3x3_wgrad_partial_multi", WW_LDS_WIDE, g, dim3(g.first[g.n]), s);
    if (rc != MG_OK) return rc;
  }
  for (int i = 0; i < n; ++i) {
    if (S.group_of[i] < 0) {  // large, of a block shape that is not inlined in the group kernel, or alone
      const int rc = launch_single_ww(S.pl[i], a[i], (d[i].flags & MG_CONV_UPS_IN) != 0, sw, s);
      if (rc != MG_OK) return rc;
    }
  }
  for (int i = 0; i < n; ++i)
    jobs[i] = mg_wgrad_job_t{a[i].slab, a[i].slab_b, d[i].gw, d[i].gb, S.pl[i].nsplit, a[i].Cout, a[i].Cin, a[i].CoutP, a[i].CinP,
                             d[i].accumulate};
  return MG_OK;
}

extern "C" int mg_wino3x3_wgrad_reduce(const mg_wgrad_job_t* jobs, int n, mg_stream_t stream) {
  MG_CHECK_ARG(jobs && n > 0, "mg_wino3x3_wgrad_reduce: bad arguments");
  for (int first = 0; first < n; first += WW_JOBS) {
    const int m = n - first < WW_JOBS ? n - first : WW_JOBS;
    WwJobs c;
    c.n = m;
    c.first[0] = 0;
    for (int i = 0; i < m; ++i) {
      c.j[i] = jobs[first + i];
      MG_CHECK_ARG(c.j[i].slab && c.j[i].gw && c.j[i].nsplit > 0 && c.j[i].CinP > 0 && c.j[i].CoutP > 0,
                   "mg_wino3x3_wgrad_reduce: bad job %d", first + i);
      c.first[i + 1] = c.first[i] + ww_reduce_blocks(c.j[i].nsplit, c.j[i].CinP * c.j[i].CoutP);
    }
    hipLaunchKernelGGL(wino_wgrad_reduce_multi, dim3(c.first[m]), dim3(512), 0, (hipStream_t)stream, c);
    MG_CHECK_LAUNCH("mg_wino3x3_wgrad_reduce");
  }
  return MG_OK;
}

extern "C" int mg_wino3x3_wgrad(const float* x, const float* gy, float* gw, float* gb, void* ws, size_t ws_bytes, int N, int Cin,
                                int Cout, int H, int W, int flags, int accumulate, int bias_n, mg_stream_t stream) {
  mg_wgrad_job_t job;
  const int rc = mg_wino3x3_wgrad_partial(x, gy, gw, gb, ws, ws_bytes, N, Cin, Cout, H, W, flags, accumulate, bias_n, &job, stream);
  return rc != MG_OK ? rc : mg_wino3x3_wgrad_reduce(&job, 1, stream);
}
