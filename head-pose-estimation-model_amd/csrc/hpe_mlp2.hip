// hpe_mlp2.hip — fused forward + MSE + backward of the reference's 2-layer pose regressor
// (Model-96/train_96.py:65-110 create_model: Conv2D 1x1 F tanh -> SpatialDropout -> Conv2D 1x1 3
//  -> SpatialDropout; Model-88/train_88.py:66-158 create_model / :226-253 bestmodelV1; 410 of the
//  684 checkpoints have this shape) on fp32 MFMA, gfx950.
//
// Work decomposition (one workgroup per CU, persistent over row tiles of T = 32*RBW rows):
//   * wave w owns hidden columns n in [32w, 32w+32) for the whole launch.  Its 32 columns of W1
//     live in VGPRs (B operand of v_mfma_f32_32x32x2_f32, Kh = ceil8(C_in)/2 per lane), its dW1
//     32x32 blocks (C_in/32 accumulators) and its W2 / b1 / dW2 / db1 slices too.
//   * per tile: X (T x C_in, contiguous in HBM) is staged once in LDS with a conflict-free row
//     stride; Z1 = X.W1 comes out of the MFMA with the row in the accumulator registers and the
//     hidden unit on the lane, so A1 = act(Z1+b1), the 3-wide head's partial sums, dA1 = dZ2.W2^T,
//     dZ1 and every per-column reduction stay in registers; the head partials are reduced across
//     the 32 lanes of a half with a reduce-scatter butterfly (48 shuffles) and across waves through
//     a [waves][T][4] LDS buffer summed in fixed order;
//   * dW1 += X^T.dZ1 consumes dZ1 straight from the accumulator registers as the MFMA B operand
//     (contraction over the row = register index: no LDS round trip), A = X from LDS.
// HBM traffic per launch: the X rows once (+ labels, + the per-workgroup gradient slab).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>

#include "hpe_common.h"
#include "hpe_dev.h"

// This file is compiled twice (Makefile): the default object, and -DMLP2_BIG with the GCN scheduler's
// unclustered-high-RP / clustered-low-occupancy rescheduling stages disabled (SCHED_mlp2), which runs
// large launches 3 % faster (Model-96 3.79 -> 3.67 ms, Model-88 1.47 -> 1.41 ms) but small ones
// (P = 1 batches of 128 rows, latency-bound) 25 % slower; mlp2_launch picks by launch size.
#ifdef MLP2_BIG
#define MLP2_NS mlp2_big
#define MLP2_BIG_OBJ 1
#else
#define MLP2_NS mlp2_small
#define MLP2_BIG_OBJ 0
#endif
#define MLP2_BIG_ROWS (1 << 15)   // rows per launch from which the MLP2_BIG object runs
namespace MLP2_NS {

#define MLP2_MAXW 12          // waves per workgroup (hidden width <= 384)
#ifndef MLP2_BAR1_SKIP
#define MLP2_BAR1_SKIP 1   // 0: the first barrier on every tile (round 5), for A/B
#endif
#ifndef MLP2_W88
#define MLP2_W88 2
#endif
#define MLP2_XS 100             // LDS row stride of an X tile (floats): conflict-free, 16-B aligned
#define MLP2_XF (32 * MLP2_XS)  // floats per X tile buffer
#define MLP2_LAB 128            // floats per label buffer: [32 rows][4] (yaw, pitch, roll, pad)
#define MLP2_RED 32             // floats of the end-of-launch loss reduction (2 x MLP2_MAXW, rounded up)
// pre-split X tiles (SPLIT kernels of the 12-wave variant, see presplit_tile): the three fp16
// fragments of the data side of split_d8 (hpe_common.h): ch = fp16(C x), cl = fp16(C x - ch), h = fp16(x)
#define MLP2_FS 104             // row stride (halves) of the fp16 image [32 rows][2 x 48]: conflict-free b128
#define MLP2_IMG (3 * 32 * MLP2_FS)  // halves of one tile's image: fragments ch, cl, h
#define MLP2_A1W (15 * 68 + 64)  // floats of a wave's A1 park (a1_row)
#define MLP2_PRE_HALVES (2 * MLP2_IMG)  // two parities: tile t + 1 is split while tile t's backward reads its own

struct E2 {
  int act, drop;
  uint32_t thr;
  float keep;
};

// image of tile row r: tile = rows [row0, row0 + 32) with row0 = img0 * P + rem0 (no 64-bit
// division per row; at P >= 32 a tile straddles at most one image boundary)
struct TileImg {
  int img0, rem0, P;
  // P32: P >= 32 known at compile time (the contiguous-rows instantiation: no division path)
  template <bool P32 = false>
  __device__ __forceinline__ int of(int r) const {
    const int t = rem0 + r;
    if (P32) return img0 + (t >= P ? 1 : 0);
    return img0 + (P >= 32 ? (t >= P ? 1 : 0) : (P == 1 ? t : t / P));
  }
  // advance by S rows, (dq, dr) = divmod(S, P) precomputed
  __device__ __forceinline__ void advance(int dq, int dr) {
    img0 += dq;
    rem0 += dr;
    if (rem0 >= P) { rem0 -= P; ++img0; }
  }
};

__device__ __forceinline__ float e_fwd(const E2& e, uint64_t seed, int64_t img, int ch, float z) {
  float a = act_f(e.act, z);
  if (e.drop >= 0) a = drop_hash(seed, e.drop, (uint64_t)img, ch) >= e.thr ? a / e.keep : 0.f;
  return a;
}

__device__ __forceinline__ float e_bwd(const E2& e, uint64_t seed, int64_t img, int ch, float g, float val) {
  if (e.drop >= 0) {
    if (drop_hash(seed, e.drop, (uint64_t)img, ch) < e.thr) return 0.f;
    g = g / e.keep;
    val = val * e.keep;
  }
  return e.act == ACT_LINEAR ? g : g * act_grad(e.act, val, 0.f);
}

// HBM -> LDS staging of one 32-row tile: one global_load_lds_dwordx4 per row with C_in/4 lanes
// active (lane i -> 16 B at the row's padded LDS base + 16 i), rows shared round-robin by the
// workgroup's waves; rows past the end repeat the last row (their loss gradient is zero).  The
// labels of the tile's rows for the loss: 2 x 64 dwords by wave 0.  Gather mode (fit's shuffled
// batches): lane l looks up the source image of tile row l once, before any piece is issued, so
// the only wait in here never drains an in-flight prefetch.
// NOW (the pre-split kernels of the big object): the label rows' source image by a ds_bpermute at the
// row's own lane address (rows < 32: no wrap term) — __shfl's lane-id term is one value hoisted to
// kernel entry, and at that kernel's register budget it sat in scratch, reloaded per tile.  Under the
// small object's flags the bpermute costs a spill instead (+0.2 us on a 128-row step): __shfl there
template <bool NOW = false>
__device__ __forceinline__ void stage_tile(const Args& args, float* xs, float* lab, int64_t row0,
                                           const TileImg& ti, int wave, int NCB, int lane, int Cin,
                                           bool labels, int XS = MLP2_XS) {
  const int64_t rem = args.nrows - 1 - row0;
  const int last = rem < 31 ? (int)rem : 31;
  const int P = args.P;
  const int q = Cin >> 2;
  if (!args.idx && P >= 32) {
    // contiguous rows, at most two images per tile: no lookups, no cross-lane traffic
    if (labels && wave == 0) {
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) {
        const int slot = pc * 64 + lane;
        const int r = min(slot >> 2, last), j = min(slot & 3, 2);
        glds4(args.ytrue + (int64_t)ti.of(r) * 3 + j, lds_addr(lab + pc * 64));
      }
    }
    for (int r = wave; r < 32; r += NCB) {
      const int64_t srow = row0 + min(r, last);
      if (lane < q) glds16(args.x + srow * Cin + 4 * lane, lds_addr(xs + r * XS));
    }
    return;
  }
  const int lr = min(lane & 31, last);
  const int limg = ti.of(lr);
  const int lpos = (int)(row0 + lr - (int64_t)limg * P);
  const int lsrc = args.idx ? args.idx[limg] : limg;  // source image of tile row lr
  // retire the index load here, visibly to hipcc's waitcnt pass (vmcnt(0)): otherwise it waits
  // for it (and so for every LDS-DMA piece issued below) at the next reuse of its register
  __builtin_amdgcn_s_waitcnt(0x0F70);
  if (labels && wave == 0) {
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      const int slot = pc * 64 + lane;
      const int r = min(slot >> 2, last), j = min(slot & 3, 2);
      const int64_t src = NOW ? __builtin_amdgcn_ds_bpermute(r << 2, lsrc) : __shfl(lsrc, r, 64);
      glds4(args.ytrue + src * 3 + j, lds_addr(lab + pc * 64));
    }
  }
  for (int r = wave; r < 32; r += NCB) {
    const int rr = min(r, last);
    const int64_t srow = (int64_t)__builtin_amdgcn_readlane(lsrc, rr) * P +
                         __builtin_amdgcn_readlane(lpos, rr);
    if (lane < q) glds16(args.x + srow * Cin + 4 * lane, lds_addr(xs + r * XS));
  }
}

// the lane id recomputed where it is used (two VALU ops) instead of a value hoisted to kernel entry:
// a kernel at its register budget spills such lane constants around its tile loop, and the reload's
// vmcnt(0) waits for every LDS-DMA piece in flight
__device__ __forceinline__ int lane_now() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}
// the value of lane l ^ 32, l the caller's lane_now(): __shfl_xor's own lane id (and the bound it
// derives from it) is one value for the whole kernel, carried from the first shuffle to the last
__device__ __forceinline__ float xor32_now(float v, int l) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute((l ^ 32) << 2, __float_as_int(v)));
}

// Staging of the contiguous-rows instantiation (no gather, P >= 32; mlp2_kernel<..., CONTIG>): tp is
// the tile's first row in HBM, carried by the tile loop (no 64-bit row * C_in product per piece), ti
// its image; one piece per row at the padded stride, as stage_tile's contiguous path.  (Twelve packed
// 1-KiB pieces per full 96-channel tile at the row stride 96 measured the same step time, A/B x3 on
// MI355X, and are not kept.)
__device__ __forceinline__ void stage_contig(const Args& args, float* xs, float* lab, const float* tp,
                                             int64_t row0, const TileImg& ti, int wave, int NCB, int Cin,
                                             bool labels) {
  const int lane = lane_now();
  const int64_t rem = args.nrows - 1 - row0;
  const int last = rem < 31 ? (int)rem : 31;
  if (labels && wave == 0) {
    const float* yp = args.ytrue + (int64_t)ti.img0 * 3;
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      const int slot = pc * 64 + lane;
      const int r = min(slot >> 2, last), j = min(slot & 3, 2);
      glds4(yp + (ti.rem0 + r >= ti.P ? 3 + j : j), lds_addr(lab + pc * 64));
    }
  }
  const int q = Cin >> 2;
  for (int r = wave; r < 32; r += NCB)
    if (lane < q) glds16(tp + min(r, last) * Cin + 4 * lane, lds_addr(xs + r * MLP2_XS));
}

typedef _Float16 h4 __attribute__((ext_vector_type(4)));

typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

// One split of the landed X tile per workgroup instead of one per wave (the 12 waves all read the
// whole tile, by rows and by columns): every thread turns 8 floats into the three data-side fp16
// fragments (ch, cl, h of split_d8), written into ONE image
//   xf[img_row(r)][48 h + m] = X[r][KH h + m] (zero for m >= KH), fragment f at xf + f * 32 * FS,
// that both GEMMs read:
//   * forward: lane (row r, half h) reads K-step s as one b128 per fragment at 48 h + 8 s of image
//     row img_row(r);
//   * dW1 (A = X^T): ds_read_b64_tr_b16 (tr_read8), which hands each lane one channel's values of
//     four rows — no second, transposed image and no second split of the tile.
// The rows are stored swapped (img_row: bits 0-1 <-> bits 2-3 of the tile row), so the four rows
// R0 .. R0 + 3 that one transposed read addresses lie 4 image rows = 208 dwords = 16 banks apart:
// each 32-lane group's four 16-dword spans tile the 64 banks, 2 LDS cycles per read where adjacent
// rows (52 dwords apart, neighbours overlapping in 4 banks) took 4.  The forward's b128 reads stay at
// 4 cycles and the pre-split's stores take 8 (10-11 unswapped); tests/test_lds_image_swap.py.
// img_pos is the position of channel c in a row: at KH = 44 the second half starts at position 48
// (16-byte aligned), so channels >= 44 sit 4 further on; positions [KH, 48) of both halves hold zeros,
// and the pad channels [C_in, 96) of the raw tile hold zeros.  A 4-channel chunk never straddles the
// gap; the chunks wholly past the image (channels 92..95 at KH = 44) map to the zeros at 92..95.
// (a position within a row: the row swap of img_row does not touch it)
template <int KH>
__device__ __forceinline__ int img_pos(int c) {
  if (KH == 48) return c;
  return c < KH ? c : min(c + 48 - KH, 92);
}
// tile row -> image row: bits 0-1 <-> bits 2-3, so tile row 16 s + 8 rd + 4 h + q is image row
// 16 s + 4 q + 2 rd + h.  The one place the map is written: the pre-split stores through it, the
// forward reads through it, and the transposed reader's lane term / second-read offset are its image
// of (h, q) / rd
__device__ __forceinline__ constexpr int img_row(int r) { return (r & 16) | ((r & 3) << 2) | ((r >> 2) & 3); }
// dW1's A operand of one (K-step, 32-channel block, fragment): tile rows R0 .. R0 + 3 and R0 + 8 ..
// R0 + 11 of the block's 32 channels, delivered channel-on-lane (lane 16 g + i of a half: channel
// 16 g + i; element j: row R0 + 8 (j >> 2) + (j & 3)).  p is the lane's address: lane 16 g + 4 q + p'
// supplies (image row img_row(R0 + q), channels 16 g + 4 p' .. + 3), 8-byte aligned; tile row + 8 is
// image row + 2 (img_row), the second read.  EXEC must be all ones here.
__device__ __forceinline__ h8 tr_read8(const _Float16* p) {
  typedef __attribute__((address_space(3))) fp16x4* lp;
  const fp16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lp)(p));
  const fp16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lp)(p + img_row(8) * MLP2_FS));
  return __builtin_shufflevector(__builtin_bit_cast(h4, a), __builtin_bit_cast(h4, b), 0, 1, 2, 3, 4, 5, 6, 7);
}
// A1 park of a wave: accumulator register g's 64 lanes at row a1_row(g), 68 floats per row slot, so
// slot t starts on bank quad t; register g takes slot g ^ ((g >> 1) & 4) (rows 8..11 on quads 12..15,
// 12..15 on 8..11), and the head's row-on-lane b128 reads (lane r reads row (r & 3) + 4 (r >> 3),
// quads 8 ((r >> 2) & 1) + 4 h + q of it) hit 16 distinct bank quads in every ds_read_b128 lane group
// (stride 64: two quads, 8-way — 112 of the 142 conflict cycles per wave and tile).  15 quads of
// padding is the least that gives 16 distinct start quads; the rows' b32 stores / reads stay
// contiguous, and a1_row(g) of an unrolled g is an immediate offset
__device__ __forceinline__ constexpr int a1_row(int g) { return 68 * (g ^ ((g >> 1) & 4)); }
// Returns the data side of the split kernels' overflow guard: whether a value of the tile lies
// outside the fp16 range of its fragment ch = fp16(C x), i.e. !(|x| < 65520 / C) — a round-to-nearest
// fp16 conversion gives infinity from 65520 on.  With finite W1 fragments (the prologue checks the
// scaled values it splits) that is exactly when the forward accumulator of the tile is non-finite:
// an in-range tile accumulates 3 x 96 products of finite fp16 fragments, and an infinite ch, or a
// NaN, reaches every column's accumulator of its row (0 x inf = NaN), the zero pad columns' too.
#define MLP2_X_LIMIT (65520.f / SPLIT_C)
template <int KH>
__device__ __forceinline__ bool presplit_tile(const float* xs, _Float16* xf, int tid, int NT) {
  bool out = false;
  // one 16-byte chunk of the image (8 floats of one row and half) per item: 384 items
  for (int i = tid; i < 32 * 12; i += NT) {
    const int r = i / 12, rem = i - r * 12, h = rem >= 6 ? 1 : 0, m0 = 8 * (rem - 6 * h);
    const float* s = xs + r * MLP2_XS + KH * h + m0;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 a = *(const f32x4*)(s), b = m0 + 4 < KH ? *(const f32x4*)(s + 4) : z;
    const f32x8 v = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) out |= !(fabsf(v[j]) < MLP2_X_LIMIT);
    const SplitD d8 = split_d8(v);
    _Float16* d = xf + img_row(r) * MLP2_FS + 48 * h + m0;
    *(h8*)(d) = d8.ch;
    *(h8*)(d + 32 * MLP2_FS) = d8.cl;
    *(h8*)(d + 64 * MLP2_FS) = d8.h;
  }
  return out;
}

// split_w8 (hpe_common.h) for the pre-split kernel's dZ1, same bits: the scaled remainder C (v - f32(h))
// as fma(f32(h), -C, C v) — C is a power of two and v - f32(h) is exact in fp32, so C v, C f32(h) and
// the result are all exact — which hipcc selects as one v_fma_mix_f32 reading the fp16 half in
// place: no v_cvt_f32_f16 back-conversion per value (presplit_tile's split_d8 gets the same
// instruction from contracting its own multiply)
__device__ __forceinline__ SplitW split_w8_mix(f32x8 v) {
  SplitW r;
  r.h = __builtin_convertvector(v, h8);
  f32x8 lo;
#pragma unroll
  for (int j = 0; j < 8; ++j) lo[j] = __builtin_fmaf((float)r.h[j], -SPLIT_C, v[j] * SPLIT_C);
  r.cl = __builtin_convertvector(lo, h8);
  return r;
}

// NWM: launch bound in waves (12: any width <= 384, 168-VGPR budget; 4: F <= 128, 256 budget)
// SPLIT: both GEMMs on fp16 MFMA at fp32 accuracy (split_w8 / split_d8 / mfma3_dw, hpe_common.h:
//   exponent-shifted lo halves, X the 3-fragment data side, accumulators at scale SPLIT_C), same registers:
//   forward  Z1 = X.W1: 6 K-steps of three v_mfma_f32_32x32x16_f16 (576 MFMA cycles per wave per
//            tile instead of 48 x 64 = 3,072); K-step s, lane half h, element j <-> channel
//            KH h + 8 s + j, so a lane splits 8 contiguous X floats of its row (two ds_read_b128) and
//            W1 sits in registers as hi / lo fp16 B fragments (48 VGPRs, as the fp32 W1 slice);
//   dW1 += X^T.dZ1: per 32-channel block two K-steps of three (576 instead of 3,072), the same 16
//            X^T reads per block as the fp32 path, split in registers, dZ1 split once per tile.
//   Loss gradients are carried unnormalised (2 (p - y): inside the fp16 range; the normalised
//   ones underflow it) and the workgroup's partials are scaled by inv_count at the flush.  A
//   non-finite forward accumulator or dW1 block (an input, dZ1 or weight outside the fp16 range)
//   sets the guard word; the exact instantiation launched behind this one then recomputes the
//   step into the same slabs (and exits at once otherwise).
// CONTIG (12-wave split kernel only): the launch has contiguous rows (no gather index) and P >= 32,
//   so the gather staging, the index lookup, the P < 32 division of TileImg::of and their
//   loop-carried state do not exist in the tile loop (stage_contig)
template <int KH, int ACT1, bool DROP, int NWM, bool SPLIT, bool CONTIG = false>
__global__ void __launch_bounds__(NWM * 64) __attribute__((amdgpu_waves_per_eu(NWM == MLP2_MAXW || ACT1 < 0 ? 1 : MLP2_W88, 8))) mlp2_kernel(Args args) {
  static_assert(!CONTIG || (SPLIT && NWM == MLP2_MAXW), "CONTIG is an instantiation of the pre-split kernel");
  if (!SPLIT && args.guard && __hip_atomic_load(args.guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != args.epoch) return;
#ifdef MLP2_STAMPS
  const uint64_t rt0 = __builtin_amdgcn_s_memrealtime();
#endif
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int NKB = (2 * KH + 31) / 32;  // 32-row blocks of dW1 (input channels)
  constexpr int T = 32;
  // PRE: the split kernel of the 12-wave variant splits each X tile once per workgroup
  // (presplit_tile) after it lands, one tile ahead, after the head phase's barrier; the raw tile
  // buffer is then single (consumed by the split before the barrier that opens its tile)
  constexpr bool PRE = SPLIT && NWM == MLP2_MAXW;
  constexpr int NXB = PRE ? 1 : 2;
  // LEAN: the pre-split kernel with a compiled-in layer-1 activation (tanh, softsign: act(0) = 0)
  // carries no per-value selects for its pad columns; the runtime-activation variant keeps them
  // (sigmoid(0) != 0)
  constexpr bool LEAN = PRE && ACT1 >= 0;
  // EXPK: the exponent's constant of the compiled-in tanh rides on the per-unit scalars (colt)
  constexpr bool EXPK = PRE && ACT1 == ACT_TANH;
  // A1 park in the bank-quad slots of a1_row; the 4-wave kernel pays for the padding with 3-float loss
  // accumulators (HS: [NT][3], 128 floats fewer at NT = 128) so it keeps four workgroups per CU — the
  // 12-wave one keeps [NT][4] (3-float rows there push its tile loop over the VGPR budget)
  constexpr bool PAD1 = true;
  constexpr int A1S = MLP2_A1W;
  constexpr int HS = NWM == MLP2_MAXW ? 4 : 3;
  const int* prog = args.prog;
  const int* o = prog + prog[H_OPS_OFF];
  const int mode = prog[H_MODE];
  const bool train = mode == MODE_TRAIN;
  const int Cin = o[O_K], F = o[O_N], NCB = o[O_MODE];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, half = lane >> 5, l32 = lane & 31;
  const int NT = blockDim.x;
  const int n = wave * 32 + l32;
  const bool nok = n < F;
  // LDS: X tiles [2][32][MLP2_XS] | labels [2][128] | head partials [NPR][T][4] | dZ2 [T][4] | scratch
  // (geom).  The 12-wave kernels keep MLP2_MAXW partial rows, rows [NCB, 12) zeroed once below, so
  // the head sums twelve unconditional loads (the + 0.f of an absent wave, as before); the 4-wave
  // kernel's LDS is sized for four workgroups per CU and keeps NCB rows
  const int NPR = NWM == MLP2_MAXW ? MLP2_MAXW : NCB;
  float* xbuf = lds;
  float* lbuf = xbuf + NXB * MLP2_XF;
  float* part = lbuf + 2 * MLP2_LAB;
  float* dz2 = part + NPR * T * 4;
  float* a1s = dz2 + T * 4;       // [NCB][MLP2_A1W]: layer-1 activations, forward -> backward (a1_row)
  float* w2t = a1s + NCB * A1S;  // [NCB * 32][4]: W2 rows (zero past F), then b2 [4]
  float* b2t = w2t + NCB * 128;
  float* hacc = b2t + 4;          // [NT][HS]: per-thread loss / db2 accumulators (sse, sae, db2)
  float* red = hacc + NCB * 64 * HS;  // [2 * MLP2_MAXW]: block reduction of the loss sums
  float* colt = red + MLP2_RED;   // [NCB * 32][4]: per hidden unit (inv1, b1, s2, -), re-read per tile
  _Float16* xfb = (_Float16*)(colt + NCB * 128);  // PRE: [2 parities][3][32][MLP2_FS] ch, cl, h
  // PRE, big object: dz2, which the backward reads as broadcast b128 rows, is packed [T][3], no pad
  // float: a lane half's four consecutive rows 8 k + 4 h .. + 3 are 48 contiguous, 16-byte aligned
  // bytes, three ds_read_b128 where four stood.  Elements are picked by compile-time index in the
  // unrolled loop; the FMAs and their order are those of the padded table.  The small object keeps the
  // padded table: its launches (< MLP2_BIG_ROWS rows, a tile or two per workgroup) are latency-bound,
  // and under its flags the packed reads spill 16 B more in the loop (+0.35 us on a 128-row step).
  // (The W2 table packed the same way for the head partials, twelve reads for sixteen, measured
  // inside the noise and is not kept: DESIGN.md)
  constexpr bool DZ2P = PRE && MLP2_BIG_OBJ;
  // BCH (big object): the head partials take their W2 rows by DPP row broadcast, one table read per tile
  // (the small object's step lines were not measured with it and keep the sixteen broadcast reads)
  constexpr bool BCH = PRE && MLP2_BIG_OBJ;
  constexpr int DZS = DZ2P ? 3 : 4;

  E2 e1 = {o[O_EACT], o[O_EDROP], (uint32_t)o[O_ETHR], __int_as_float(o[O_EKEEP])};
  E2 e2 = {o[O_AUX2], o[O_TBASE], (uint32_t)o[O_TCOUNT], __int_as_float(o[O_F0])};
  const float inv_keep1 = 1.f / e1.keep;
  const float* W1 = args.params + o[O_W];
  const float* W2 = args.params + o[O_AUX0];

  const int64_t nrows = args.nrows;
  const int64_t ntiles = (nrows + T - 1) / T;
  const int P = args.P;
  const bool labels = mode != MODE_FWD;
  // tile -> (first image, row within it), advanced incrementally (no 64-bit division per tile)
  const int S = gridDim.x * T, dq = S / P, dr = S - dq * P;
  TileImg ti;
  ti.P = P;
  ti.img0 = (int)(blockIdx.x * T / P);
  ti.rem0 = (int)(blockIdx.x * T - ti.img0 * P);
  // prologue: the first tile's LDS-DMA, then every parameter load in one batch ahead of any use —
  // one memory round trip instead of eight serial ones (W1 in two halves, W2[n], b1, the W2 table
  // twice, b2, the tile: ~16 k cycles, the largest phase of a one-tile launch, P = 1 per-step fit).
  // The DMA goes first: hipcc's vmcnt waits count only its own (younger) loads, so they stay exact.
  // CONTIG: the next tile to stage, advanced by one grid stride of rows per tile (unused, and so
  // not computed, in the other instantiations)
  const float* xnext = CONTIG ? args.x + (int64_t)blockIdx.x * T * Cin : nullptr;
  const int64_t xstep = CONTIG ? (int64_t)gridDim.x * T * Cin : 0;
  if (blockIdx.x < ntiles) {
    if constexpr (CONTIG) stage_contig(args, xbuf, lbuf, xnext, (int64_t)blockIdx.x * T, ti, wave, NCB, Cin, labels);
    else stage_tile<PRE && MLP2_BIG_OBJ>(args, xbuf, lbuf, (int64_t)blockIdx.x * T, ti, wave, NCB, lane, Cin, labels);
  }
  xnext += xstep;
  const int nc = min(n, F - 1);
  const float w2a = W2[nc * 3], w2b = W2[nc * 3 + 1], w2c = W2[nc * 3 + 2];
  const int o_bias = __builtin_amdgcn_readfirstlane(o[O_BIAS]), o_aux1 = __builtin_amdgcn_readfirstlane(o[O_AUX1]);
  const float b1r = args.params[max(o_bias, 0) + nc];
  float w2r[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {  // the W2 table: NCB * 128 entries over NT = 64 NCB threads
    const int i = threadIdx.x + t * NT, nn = i >> 2, j = i & 3;
    w2r[t] = W2[min(nn, F - 1) * 3 + min(j, 2)];
  }
  const float b2r = args.params[max(o_aux1, 0) + min((int)threadIdx.x & 3, 2)];

  // ---- register-resident weights of this wave's 32 hidden columns ----
  float wreg[SPLIT ? 1 : KH];
  SplitW wsp[SPLIT ? 6 : 1];
  // SPLIT: weight-side exponents per hidden unit n (pow2_scale): W1 column n enters the forward
  // MFMAs scaled by s1 (its max |w| in [2^13, 2^14)), Z1 comes out as acc * inv1, inv1 = 1 / (C s1);
  // dZ1 column n enters the dW1 MFMAs scaled by s2 (from max_j |W2[n][j]|, its only per-column
  // factor: s2 max |W2[n]| in [2^2, 2^3)), dW1 leaves as acc / (C s2)
  float inv1 = 1.f, s2 = 1.f;
  bool wbad = false;  // PRE: a W1 fragment of this lane's column is not finite (the weight side of the guard)
  if constexpr (SPLIT) {
    f32x8 v[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = half * KH + 8 * s + j;
        v[s][j] = 8 * s + j < KH ? W1[(size_t)min(k, Cin - 1) * F + nc] : 0.f;
      }
    }
    // every prologue load issued above this point (the scheduler otherwise sinks W2[n], b1 and the
    // W2 table loads to their uses, each behind its own vmcnt wait)
    __builtin_amdgcn_sched_barrier(0);
    float mx = 0.f;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = half * KH + 8 * s + j;
        v[s][j] = (k < Cin && nok) ? v[s][j] : 0.f;
        mx = fmaxf(mx, fabsf(v[s][j]));
      }
    }
    mx = fmaxf(mx, PRE ? xor32_now(mx, lane_now()) : __shfl_xor(mx, 32, 64));
    const float s1 = pow2_scale(mx, 13);
    inv1 = SPLIT_INV_C / s1;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      const f32x8 vs = v[s] * s1;
      wsp[s] = split_w8(vs);
      // the scaled value, per value (fmaxf drops a NaN from mx): its hi half fp16(w s1) is infinite
      // from 65520 on — an infinite or NaN entry (s1 = 1), or a finite column maximum from about
      // 2^102 on, past pow2_scale's exponent clamp (s1 stays at 2^-86); below that every fragment
      // is finite (|lo| <= 2^10 x half an fp16 ulp)
      if (PRE) {
#pragma unroll
        for (int j = 0; j < 8; ++j) wbad |= !(fabsf(vs[j]) < 65520.f);
      }
    }
    s2 = pow2_scale(nok ? fmaxf(fmaxf(fabsf(w2a), fabsf(w2b)), fabsf(w2c)) : 0.f, 2);
  } else {
#pragma unroll
    for (int m = 0; m < KH; ++m) {
      const int k = half * KH + m;
      const float wv = W1[(size_t)min(k, Cin - 1) * F + nc];
      wreg[m] = (k < Cin && nok) ? wv : 0.f;
    }
  }
  // PRE: the forward side of the overflow guard is checked where the values are already in hand and
  // off the tile loop's critical path — the data by presplit_tile (every tile passes through it once:
  // prologue or head shadow), W1 above: a non-finite fragment makes the accumulator
  // of every tile non-finite (inf x, or 0 x inf = NaN), so it flags the launch as soon as the
  // workgroup has a tile.  With finite fragments on both sides the fp32 accumulator stays finite
  bool bad = PRE && wbad && blockIdx.x < ntiles;
  {
    // the per-unit scalars live in LDS across the tile loop, not in 3 loop-carried VGPRs (the
    // 12-wave variant sits at the 168-VGPR budget; in registers they pushed a W1 fragment to scratch)
    const float b1 = (nok && o_bias >= 0) ? b1r : 0.f;
    // EXPK: the pre-split kernel with tanh compiled in keeps the pair pre-multiplied by fast_tanh5's
    // 2 log2(e), so the forward takes e^{2z} = exp2(fma(acc, inv1 k, b1 k)) without a multiply per
    // value (inv1 is a power of two: inv1 k is exact; b1 k rounds once, the argument moves by about
    // one ulp of itself, inside fast_tanh5's 2^-22 absolute bar)
    const float ck = EXPK ? 2.8853900817779268f : 1.f;
    if (half == 0) *(f32x4*)(colt + n * 4) = f32x4{inv1 * ck, b1 * ck, s2, 0.f};
  }
  // small tables in LDS rather than loop-carried VGPRs (the 12-wave variant is at its budget)
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int i = threadIdx.x + t * NT, nn = i >> 2, j = i & 3;
    if (i < NCB * 128) w2t[i] = (nn < F && j < 3) ? w2r[t] : 0.f;
  }
  if (threadIdx.x < 4) b2t[threadIdx.x] = (threadIdx.x < 3 && o_aux1 >= 0) ? b2r : 0.f;
  for (int i = threadIdx.x; i < NT * HS; i += NT) hacc[i] = 0.f;

  f32x16 dw[NKB];
#pragma unroll
  for (int s = 0; s < NKB; ++s) dw[s] = f32x16{};
  float dw2[3] = {0.f, 0.f, 0.f};
  float db1 = 0.f;

  // head phase: thread it handles (row, output) items it, it + NT3, ... with NT3 a multiple of 3,
  // so its output index j (and its db2 accumulator) is the same in every tile
  const int NT3 = (NT / 3) * 3;

  // pad columns [C_in, 96) of both X buffers: never written by the staging, read by the forward
  // MFMA against zero weights -> must hold zeros, not stale LDS (the DMA above writes [0, C_in))
  for (int i = threadIdx.x; i < NXB * 32 * 16; i += NT) {
    const int r = i >> 4, c = Cin + (i & 15);
    if (c < 96) xbuf[r * MLP2_XS + c] = 0.f;
  }
  // the partial rows of the absent waves [NCB, NPR): zero for the whole launch
  for (int i = NCB * T * 4 + threadIdx.x; i < NPR * T * 4; i += NT) part[i] = 0.f;
  __syncthreads();
  if constexpr (PRE) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bar_lds();
    // (a workgroup without a tile splits whatever its LDS holds: not data, so not checked)
    const bool xbad = presplit_tile<KH>(xbuf, xfb, threadIdx.x, NT);
    bad |= xbad && blockIdx.x < ntiles;
  }
  int buf = 0;
#ifdef MLP2_STAMPS
  uint32_t ph[9] = {};
  uint64_t tprev = __builtin_amdgcn_s_memtime();
  const uint64_t rt1 = __builtin_amdgcn_s_memrealtime();
#define STAMP(i) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); ph[i] += (uint32_t)(t_ - tprev); tprev = t_; } while (0)
#else
#define STAMP(i) do {} while (0)
#endif
  for (int tile = blockIdx.x; tile < (int)ntiles; tile += gridDim.x, buf ^= 1, ti.advance(dq, dr)) {
    // PRE: the lane's coordinates recomputed per tile (lane_now: a few VALU ops) — hoisted to kernel
    // entry they and the LDS addresses derived from them stay live across the whole loop, at the
    // register budget the price was a W1 fragment in scratch, reloaded per tile behind a vmcnt(0)
    // that waits for the next tile's LDS-DMA
    const int tlane = PRE ? lane_now() : lane, thalf = tlane >> 5, tl32 = tlane & 31;
    const int tcol = wave * 32 + tl32;
    const bool tok = tcol < F;
    // ... and the thread id of the head phase with them: threadIdx.x, the LDS addresses and the
    // cold-path terms (output pointer, dropout hash) derived from it are otherwise carried around
    // the loop, in scratch at this budget
    // (threadIdx.x itself, unsigned as ever, in the other kernels: their code stays as it was)
    using tid_t = typename std::conditional<PRE, int, unsigned>::type;
    const tid_t ttid = PRE ? (tid_t)(wave * 64 + tlane) : (tid_t)threadIdx.x;
    const int64_t row0 = (int64_t)tile * T;
    const float* xs = xbuf + (PRE ? 0 : buf) * MLP2_XF;
    const float* lab = lbuf + buf * MLP2_LAB;
    // tile `tile` landed (own pieces) -> barrier: every wave's pieces landed, and every wave is
    // done with tile - gridDim.x, whose buffer the prefetch below overwrites (PRE: the tile was
    // split before this barrier, the raw buffer is free)
    if constexpr (!PRE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(0);
    // PRE: every LDS hazard this barrier guards is already ordered by the previous tile's two
    // barriers (the one before the head, B2, and the one after it, B3) — the raw tile was split (and
    // the next raw tile's landing waited for) before B3, the partials / this parity's labels were last
    // read before it, the A1 park and the loss accumulators are per wave / per thread.  The fp16 image
    // has two parities: tile t's forward (before B2(t)) and backward (after B3(t)) read parity p; tile
    // t + 1 is split into parity p ^ 1 between B2(t) and B3(t), after that parity's last reader (tile
    // t - 1's backward, which every wave left before B2(t)) and before its next (tile t + 1's forward,
    // after B3(t)); the writer of parity p for tile t + 2 runs after B2(t + 1), which every wave
    // reaches only past tile t's backward, the last reader of parity p.  So after the first tile
    // (whose pre-split is ordered only by this barrier) the tile loop runs on two barriers
    if (!(MLP2_BAR1_SKIP && PRE && tile != (int)blockIdx.x)) bar_lds();
    STAMP(1);
    if (tile + gridDim.x < ntiles) {
      TileImg tn = ti;
      tn.advance(dq, dr);
      if constexpr (CONTIG) {
        stage_contig(args, xbuf, lbuf + (buf ^ 1) * MLP2_LAB, xnext, (int64_t)(tile + gridDim.x) * T, tn,
                     wave, NCB, Cin, labels);
        xnext += xstep;
      } else {
        stage_tile<PRE && MLP2_BIG_OBJ>(args, xbuf + (PRE ? 0 : (buf ^ 1)) * MLP2_XF, lbuf + (buf ^ 1) * MLP2_LAB,
                   (int64_t)(tile + gridDim.x) * T, tn, wave, NCB, tlane, Cin, labels);
      }
    }

    STAMP(2);
    // ---- forward: Z1 = X.W1 (+b1, act, dropout) and the head partials ----
    uint32_t dmask = 0;  // layer-1 dropout keep bits of this lane's 16 rows (reused by backward)
    {
      const float* ap = xs + tl32 * MLP2_XS + thalf * KH;
      f32x16 acc = {};
      if constexpr (PRE) {
        const _Float16* fp = xfb + buf * MLP2_IMG + img_row(tl32) * MLP2_FS + 48 * thalf;
        // two-deep fragment buffer: the three reads of K-step s + 1 are issued before K-step s's
        // MFMAs, so an MFMA waits for reads a whole K-step old, not for its own fragment's round trip
        auto frag = [&](int s) {
          return SplitD{*(const h8*)(fp + 8 * s), *(const h8*)(fp + 32 * MLP2_FS + 8 * s),
                        *(const h8*)(fp + 64 * MLP2_FS + 8 * s)};
        };
        SplitD xd = frag(0);
#pragma unroll
        for (int s = 0; s < 6; ++s) {
          SplitD xn = xd;
          if (s + 1 < 6) xn = frag(s + 1);
          __builtin_amdgcn_sched_barrier(0);
          acc = mfma3_dw(xd, wsp[s], acc);
          xd = xn;
        }
        // (no accumulator check here: presplit_tile and the prologue's W1 check flag the same launches)
        STAMP(3);
      } else if constexpr (SPLIT) {
#pragma unroll
        for (int s = 0; s < 6; ++s) {
          const f32x4 a0 = *(const f32x4*)(ap + 8 * s), a1 = *(const f32x4*)(ap + 8 * s + 4);
          acc = mfma3_dw(split_d8(f32x8{a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}), wsp[s], acc);
          __builtin_amdgcn_sched_barrier(0);
        }
        bad |= !(fabsf(sum16(acc)) <= 3.0e38f);
      } else {
        f32x4 an = *(const f32x4*)(ap);
#pragma unroll
        for (int m = 0; m < KH; m += 4) {
          const f32x4 a = an;
          if (m + 4 < KH) an = *(const f32x4*)(ap + m + 4);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, wreg[m + 0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, wreg[m + 1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, wreg[m + 2], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, wreg[m + 3], acc, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (DROP) {
        if (CONTIG || P >= 32) {  // two images at most: two hashes per lane per tile
          const bool k0 = drop_hash(args.seed, e1.drop, (uint64_t)(ti.img0 + args.img_off), tcol) >= e1.thr;
          const bool k1 = drop_hash(args.seed, e1.drop, (uint64_t)(ti.img0 + 1 + args.img_off), tcol) >= e1.thr;
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            const int r = (g & 3) + 8 * (g >> 2) + 4 * thalf;
            dmask |= (ti.rem0 + r >= P ? k1 : k0) ? (1u << g) : 0u;
          }
        } else {
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            const int r = (g & 3) + 8 * (g >> 2) + 4 * thalf;
            dmask |= drop_hash(args.seed, e1.drop, (uint64_t)(ti.of(r) + args.img_off), tcol) >= e1.thr
                         ? (1u << g) : 0u;
          }
        }
      }
      const f32x4 cs = *(const f32x4*)(colt + tcol * 4);  // (inv1, b1, s2, -); EXPK: both x 2 log2(e)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        float z;
        if constexpr (EXPK) {  // fast_tanh5 with its argument already scaled
          const float e = __builtin_amdgcn_exp2f(fmaf(acc[g], cs.x, cs.y));
          z = fmaf(-2.f, __builtin_amdgcn_rcpf(1.f + e), 1.f);
        } else {
          z = act1_f<ACT1, SPLIT>(e1.act, SPLIT ? fmaf(acc[g], cs.x, cs.y) : acc[g] + cs.y);
        }
        if (DROP) z = (dmask >> g) & 1u ? z * inv_keep1 : 0.f;
        // LEAN: a pad column (n >= F) has a zero W1 column, b1 = 0 and zero W2 rows, and the
        // compiled-in activations map 0 to 0: its z is already exactly 0 without a select
        acc[g] = LEAN || tok ? z : 0.f;
      }
      // park A1 in LDS across the head phase (16 VGPRs fewer live through the loss epilogue)
#pragma unroll
      for (int g = 0; g < 16; ++g) a1s[wave * A1S + (PAD1 ? a1_row(g) : 64 * g) + tlane] = acc[g];
      // head partials from the parked A1 (a row-on-lane read of this wave's own LDS region, no
      // cross-lane shuffles): lane (row r = l32, half h) dots A1[r][16 h .. 16 h + 16) with the
      // matching W2 rows, the two halves are combined with one xor-32 exchange
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      {
        const int r = tl32, hh = (r >> 2) & 1, gr = (r & 3) + 4 * (r >> 3);
        const float* ar = a1s + wave * A1S + (PAD1 ? a1_row(gr) : 64 * gr) + hh * 32 + 16 * thalf;
        const float* wr = w2t + (wave * 32 + 16 * thalf) * 4;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        if constexpr (BCH) {
          // the half's sixteen W2 rows one per lane (lane 16 q + u of the wave: unit 16 (q >> 1) + u),
          // handed to the FMAs by row broadcast: one table read where sixteen broadcast reads stood
          f32x4 av[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) av[i] = *(const f32x4*)(ar + 4 * i);
          const f32x4 wq = *(const f32x4*)(wr + (tlane & 15) * 4);
          float wx = wq.x, wy = wq.y, wz = wq.z;
          dpp_settle3(wx, wy, wz);
          fmac3x4_bcast<0>(s0, s1, s2, wx, wy, wz, av[0]);
          fmac3x4_bcast<4>(s0, s1, s2, wx, wy, wz, av[1]);
          fmac3x4_bcast<8>(s0, s1, s2, wx, wy, wz, av[2]);
          fmac3x4_bcast<12>(s0, s1, s2, wx, wy, wz, av[3]);
        } else {
#pragma unroll
        for (int i = 0; i < 16; i += 4) {
          const f32x4 av = *(const f32x4*)(ar + i);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const f32x4 w = *(const f32x4*)(wr + (i + e) * 4);
            s0 = fmaf(av[e], w.x, s0);
            s1 = fmaf(av[e], w.y, s1);
            s2 = fmaf(av[e], w.z, s2);
          }
        }
        }
        if constexpr (PRE) {
          s0 += xor32_now(s0, tlane);
          s1 += xor32_now(s1, tlane);
          s2 += xor32_now(s2, tlane);
        } else {
          s0 += __shfl_xor(s0, 32, 64);
          s1 += __shfl_xor(s1, 32, 64);
          s2 += __shfl_xor(s2, 32, 64);
        }
        if (thalf == 0) *(f32x4*)(part + (wave * T + r) * 4) = f32x4{s0, s1, s2, 0.f};
      }
    }
    STAMP(4);
    // PRE (NCB >= 5: pick_d sends narrower layers to the 4-wave kernel): the next tile's pre-split
    // runs on waves 2.. during the head (waves 0-1), into the image's other parity, so its pieces
    // must have landed by this barrier instead of the next one
    if constexpr (PRE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bar_lds();
    STAMP(5);
    if constexpr (PRE) {
      if (wave >= 2 && tile + gridDim.x < ntiles)
        bad |= presplit_tile<KH>(xbuf, xfb + (buf ^ 1) * MLP2_IMG, ttid - 128, NT - 128);
    }

    // ---- head: sum partials (fixed wave order) + b2, epilogue, loss / output ----
    auto head_item = [&](int it) {
      const int r = it / 3, j = it - r * 3;
      const int64_t R = row0 + r;
      float z = b2t[j];
      float pv[MLP2_MAXW];  // all partial loads in flight, summed in fixed wave order
#pragma unroll
      for (int w = 0; w < MLP2_MAXW; ++w) pv[w] = NWM == MLP2_MAXW || w < NCB ? part[(w * T + r) * 4 + j] : 0.f;
      // the label and this thread's loss accumulators read with the partials (one LDS round trip;
      // read-modify-written one by one behind the dz2 store they were three more on the head's path)
      float lv = 0.f, ha0 = 0.f, ha1 = 0.f, ha2 = 0.f;
      if (mode != MODE_FWD) {
        lv = lab[r * 4 + j];
        ha0 = hacc[ttid * HS + 0];
        ha1 = hacc[ttid * HS + 1];
        ha2 = hacc[ttid * HS + 2];
      }
#pragma unroll
      for (int w = 0; w < MLP2_MAXW; ++w) z += pv[w];
      // ACT1 >= 0 kernels are only picked for a linear head (the create_model family); the row's
      // image and the output dropout's keep bit only when that dropout is on (uniform branch: the
      // no-dropout head computes neither)
      const bool d2 = ACT1 < 0 || __builtin_expect(e2.drop >= 0, 0);
      int64_t img = 0;
      bool k2 = true;
      if (d2) {
        img = ti.of<CONTIG>(r) + args.img_off;
        if (ACT1 >= 0) k2 = drop_hash(args.seed, e2.drop, (uint64_t)img, j) >= e2.thr;
      }
      const float p = ACT1 >= 0 ? (d2 ? (k2 ? z / e2.keep : 0.f) : z) : e_fwd(e2, args.seed, img, j, z);
      if (mode == MODE_FWD) {
        if (R < nrows) args.y[R * 3 + j] = p;
      } else {
        float g = 0.f;
        if (R < nrows) {
          const float err = p - lv;
          ha0 = fmaf(err, err, ha0);
          ha1 += fabsf(err);
          g = SPLIT ? 2.f * err : 2.f * err * args.inv_count;
        }
        if (train) {
          g = ACT1 >= 0 ? (d2 ? (k2 ? g / e2.keep : 0.f) : g) : e_bwd(e2, args.seed, img, j, g, p);
          dz2[r * DZS + j] = g;
          ha2 += g;
        }
        hacc[ttid * HS + 0] = ha0;
        hacc[ttid * HS + 1] = ha1;
        hacc[ttid * HS + 2] = ha2;
      }
    };
    if constexpr (NWM == MLP2_MAXW) {
      // at least 320 threads for the 96 items: one item per thread
      if (ttid < T * 3) head_item(ttid);
    } else {
      for (int it = threadIdx.x; it < T * 3 && threadIdx.x < NT3; it += NT3) head_item(it);
    }
    STAMP(6);
    if constexpr (PRE) {
      // the head is done and the next tile is split (by waves 2.. during the head: splitting it here,
      // after the barrier, measured slower, 3.235 -> 3.128 ms on configs[3], A/B x3)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      bar_lds();
      STAMP(7);
      if (!train) continue;
    } else {
      if (!train) continue;  // the next tile's first barrier orders part / lab reuse
      bar_lds();
    }

    STAMP(8);
    // ---- backward: dA1 = dZ2.W2^T, dZ1, dW2, db1 in registers; dW1 += X^T.dZ1 on MFMA ----
    {
      const f32x4 w2r = *(const f32x4*)(w2t + tcol * 4);
      const float s2 = colt[tcol * 4 + 2];
      // PRE: the dW1 operand's power-of-two scale s2 rides on the three W2 values of dA1 (3 multiplies
      // instead of 16 on dZ1; exact, so dZ1 s2 has the same bits either way) and db1 accumulates
      // scaled, unscaled once at the flush
      const f32x4 w2v = PRE ? f32x4{w2r.x * s2, w2r.y * s2, w2r.z * s2, 0.f} : w2r;
      // dZ1 of accumulator register g (row (g & 3) + 8 (g >> 2) + 4 h), dW2 / db1 on the way
      // (dx, dy, dz): the row's dZ2
      auto dz_row = [&](int g, float dx, float dy, float dz) {
        const float a = a1s[wave * A1S + (PAD1 ? a1_row(g) : 64 * g) + tlane];
        // PRE: the fused form this sum compiles to, spelled out — with the scale folded into w2v the
        // bits stay the same only in that form, in every instantiation
        const float da = PRE ? fmaf(dz, w2v.z, fmaf(dx, w2v.x, dy * w2v.y))
                             : dx * w2v.x + dy * w2v.y + dz * w2v.z;
        float gz, av = a;
        if (DROP) {
          gz = (dmask >> g) & 1u ? da * inv_keep1 : 0.f;
          av = a * e1.keep;
        } else {
          gz = da;
        }
        // LEAN: a pad column's W2 row is zero, so its dA1, and with it dZ1, is already 0 — or NaN under
        // a non-finite dZ2, which stays inside the pad column: its dW1 / db1 / dW2 are never stored
        // and the flush keeps it out of the overflow check
        // (db1 sums the rounded dZ1 the MFMAs see: without the select between them the product and
        // the sum would contract to one fma)
        {
#pragma clang fp contract(off)
          gz = LEAN || tok ? gz * act1_g<ACT1>(e1.act, av) : 0.f;
          db1 += gz;
        }
        dw2[0] = fmaf(a, dx, dw2[0]);
        dw2[1] = fmaf(a, dy, dw2[1]);
        dw2[2] = fmaf(a, dz, dw2[2]);
        return gz;
      };
      // the padded table: one broadcast b128 per row
      auto dz_of = [&](int g) {
        const int r = (g & 3) + 8 * (g >> 2) + 4 * thalf;
        const f32x4 d = *(const f32x4*)(dz2 + r * 4);
        return dz_row(g, d.x, d.y, d.z);
      };
      // DZ2P: K-step s's eight dZ1 (accumulator registers 8 s .. 8 s + 7) from the packed table: the four
      // rows 8 k + 4 h .. + 3 of k = 2 s, 2 s + 1 are twelve floats each, three b128; row q's dZ2 at 3 q
      auto dz_step = [&](int s) {
        f32x8 dv;
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          const float* dp = dz2 + (8 * (2 * s + k2) + 4 * thalf) * 3;
          const f32x4 t0 = *(const f32x4*)(dp), t1 = *(const f32x4*)(dp + 4), t2 = *(const f32x4*)(dp + 8);
          const float t[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) dv[4 * k2 + q] = dz_row(8 * s + 4 * k2 + q, t[3 * q], t[3 * q + 1], t[3 * q + 2]);
        }
        return dv;
      };
      if constexpr (PRE) {
        // dZ1 of K-step 0 -> split -> its 9 MFMAs, with the VALU of K-step 1's dZ1 free to issue
        // under them (no scheduling fences between the two), then K-step 1's MFMAs
        // The A operand X^T by transposed reads of this tile's image (tr_read8): K-step s, lane half
        // h, element j <-> tile row 16 s + 8 (j >> 2) + 4 h + (j & 3), so R0 = 16 s + 4 h; lane
        // 16 g + 4 q + p of the half addresses tile row R0 + q = image row 16 s + 4 q + h (img_row),
        // channels 32 kb + 16 g + 4 p .. + 3.  One lane term recomputed per tile; K-step, block (at
        // KH = 48) and fragment are immediate offsets
        const int tc = (tl32 & 16) + 4 * (tl32 & 3);
        const _Float16* th = xfb + buf * MLP2_IMG + img_row(4 * thalf + ((tl32 >> 2) & 3)) * MLP2_FS;
        auto xt_of = [&](int s, int kb) {
          const _Float16* q = th + 16 * s * MLP2_FS + img_pos<KH>(32 * kb + tc);
          return SplitD{tr_read8(q), tr_read8(q + 32 * MLP2_FS), tr_read8(q + 64 * MLP2_FS)};
        };
        f32x8 dv0, dv1;
        if constexpr (DZ2P) dv0 = dz_step(0);
        else {
#pragma unroll
          for (int j = 0; j < 8; ++j) dv0[j] = dz_of(j);
        }
        const SplitW d0 = split_w8_mix(dv0);
        __builtin_amdgcn_sched_barrier(0);
        // (no fence between the blocks: all 18 reads of the K-step may be in flight at once.  Their 36
        // VGPRs fit since the head phase's thread id and the shuffles' lane id are recomputed per tile
        // (ttid, xor32_now) instead of carried around the loop; a fence after block 0, which the
        // tighter budget needed before, measured 1.2 % slower on the Model-96 step, A/B x3)
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) dw[kb] = mfma3_dw(xt_of(0, kb), d0, dw[kb]);
        if constexpr (DZ2P) dv1 = dz_step(1);
        else {
#pragma unroll
          for (int j = 0; j < 8; ++j) dv1[j] = dz_of(8 + j);
        }
        __builtin_amdgcn_sched_barrier(0);
        const SplitW d1 = split_w8_mix(dv1);
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) dw[kb] = mfma3_dw(xt_of(1, kb), d1, dw[kb]);
      } else if constexpr (SPLIT) {
        // K-step s (rows 16 s + 8 (j >> 2) + 4 h + (j & 3)): dZ1 registers 8 s .. 8 s + 7 as the B
        // operand, the matching X^T rows as A; one K-step at a time keeps the live set small
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          f32x8 dv;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            dv[j] = dz_of(8 * s + j);
            if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
          }
          const SplitW dsp = split_w8(dv * s2);
#pragma unroll
          for (int kb = 0; kb < NKB; ++kb) {
            const float* xp = xs + (4 * thalf) * MLP2_XS + kb * 32 + tl32;
            f32x8 xv;
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[j] = xp[(16 * s + 8 * (j >> 2) + (j & 3)) * MLP2_XS];
            dw[kb] = mfma3_dw(split_d8(xv), dsp, dw[kb]);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      } else {
        float dz1[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          dz1[g] = dz_of(g);
          if ((g & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // bound the dZ2 reads in flight
        }
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
          // X^T block: lane reads X[r(g)][k = 32 kb + l32]
          const float* xp = xs + (4 * thalf) * MLP2_XS + kb * 32 + tl32;
          f32x16 acc = dw[kb];
          auto xat = [&](int g) { return xp[((g & 3) + 8 * (g >> 2)) * MLP2_XS]; };
          float x0 = xat(0), x1 = xat(1);
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            const float xv = x0;
            x0 = x1;
            if (g + 2 < 16) x1 = xat(g + 2);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, dz1[g], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
          }
          dw[kb] = acc;
        }
      }
    }
  }

#ifdef MLP2_STAMPS
  const uint64_t rt2 = __builtin_amdgcn_s_memrealtime();
  uint64_t rtA = 0, rtB = 0;
  if (PRE && blockIdx.x == 0 && lane == 0 && (wave == 0 || wave == 5))
    printf("STAMP w%d bwd+tail %u bar1 %u stage %u fwdmfma %u act+part %u bar2 %u head %u bar3 %u presplit %u\n", wave,
           ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], ph[6], ph[7], ph[8]);
#endif
  // (the lane's coordinates again: not kept live across the tile loop in the pre-split kernels)
  const int flane = PRE ? lane_now() : lane, fhalf = flane >> 5;
  const int fcol = wave * 32 + (flane & 31);
  const bool fok = fcol < F;
  if (mode == MODE_FWD) {
    if (SPLIT && bad) __hip_atomic_store(args.guard, args.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  // ---- flush this workgroup's partial gradients + loss sums ----
  const int slab = prog[H_SLAB];
  const int npt = prog[H_NPARAMS_TRAIN];
  float* ws = args.ws + (size_t)blockIdx.x * slab;
  const float sc = SPLIT ? args.inv_count : 1.f;  // the split path carries unnormalised gradients
  // slab offsets in registers: read through `o` at each store, the compiler reloads them behind a
  // vmcnt(0) per store (ws may alias the program) — 48 serial round trips, 17 us of a one-tile launch
  const int oW = __builtin_amdgcn_readfirstlane(o[O_W]), oB = __builtin_amdgcn_readfirstlane(o[O_BIAS]);
  const int oA0 = __builtin_amdgcn_readfirstlane(o[O_AUX0]), oA1 = __builtin_amdgcn_readfirstlane(o[O_AUX1]);
  __syncthreads();
  const float s2f = colt[fcol * 4 + 2];
  if (train) {
    const float scw = SPLIT ? sc * (SPLIT_INV_C / s2f) : sc;
    float chk = 0.f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      if (SPLIT) chk += sum16(dw[kb]);
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int k = kb * 32 + (g & 3) + 8 * (g >> 2) + 4 * fhalf;
        if (k < Cin && fok) ws[oW + (size_t)k * F + fcol] = dw[kb][g] * scw;
      }
    }
    // (a LEAN pad column's accumulators are zero, or hold the NaN of a non-finite dZ2 that the
    // select-free dZ1 lets through: never stored, and not part of the check)
    if (SPLIT) bad |= (!LEAN || fok) && !(fabsf(chk) <= 3.0e38f);
    // PRE: db1 was accumulated at the dW1 operand's scale s2 (a power of two: exact to undo)
    const float tb = (db1 + __shfl_xor(db1, 32, 64)) * (PRE ? 1.f / s2f : 1.f);
    float t2[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) t2[j] = dw2[j] + __shfl_xor(dw2[j], 32, 64);
    if (fhalf == 0 && fok) {
      if (oB >= 0) ws[oB + fcol] = tb * sc;
#pragma unroll
      for (int j = 0; j < 3; ++j) ws[oA0 + fcol * 3 + j] = t2[j] * sc;
    }
#ifdef MLP2_STAMPS
    rtA = __builtin_amdgcn_s_memrealtime();
#endif
    // db2: output j's per-thread accumulators (threads i = j mod 3 below NT3), fixed order: lane q
    // sums i = j + 3 q, j + 3 (q + 64), ..., then one wave sum (was one thread's serial pass over
    // NT3 / 3 LDS reads: 10 us of a one-tile launch)
    if (oA1 >= 0) {
      for (int j = wave; j < 3; j += NT >> 6) {
        float s = 0.f;
        for (int i = j + 3 * flane; i < NT3; i += 192) s += hacc[i * HS + 2];
        s = wave_sum(s);
        if (flane == 0) ws[oA1 + j] = s * sc;
      }
    }
#ifdef MLP2_STAMPS
    rtB = __builtin_amdgcn_s_memrealtime();
#endif
    __syncthreads();
  }
#ifdef MLP2_STAMPS
  const uint64_t rtC = __builtin_amdgcn_s_memrealtime();
#endif
  if (SPLIT && bad) __hip_atomic_store(args.guard, args.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float a = wave_sum(hacc[threadIdx.x * HS + 0]), b = wave_sum(hacc[threadIdx.x * HS + 1]);
  if (flane == 0) { red[wave] = a; red[MLP2_MAXW + wave] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s0 = 0.f, s1 = 0.f;
    const int nw = NT >> 6;
    for (int w = 0; w < nw; ++w) { s0 += red[w]; s1 += red[MLP2_MAXW + w]; }
    ws[npt] = s0;
    ws[npt + 1] = s1;
  }
#ifdef MLP2_STAMPS
  if (PRE && threadIdx.x == 0) {
    const uint64_t rt3 = __builtin_amdgcn_s_memrealtime();
    printf("RT wg %d t0 %llu pro %llu loop %llu flush %llu wstore %llu db2 %llu sync %llu tail %llu\n", (int)blockIdx.x, (unsigned long long)rt0,
           (unsigned long long)(rt1 - rt0), (unsigned long long)(rt2 - rt1), (unsigned long long)(rt3 - rt2),
           (unsigned long long)(rtA - rt2), (unsigned long long)(rtB - rtA), (unsigned long long)(rtC - rtB), (unsigned long long)(rt3 - rtC));
  }
#endif
}

#ifdef MLP2_BIG
// ------------------------------------------------------------------------------------------------
// mlp2r_kernel: the large-launch training kernel for NARROW hidden layers (F <= 64: Model-88's
// create_model, 88 -> 64 softsign -> 3, train_88.py:66-140), one WAVE per workgroup and every wave
// a whole worker over its own 32-row tiles.  mlp2_kernel gives such a layer two waves per tile:
// both split the same X tile (the data-side split is most of their VALU work), they meet at three
// barriers per tile and run two waves per SIMD at the 256-VGPR budget.  Here one wave owns all 64
// hidden units (two 32-unit blocks: W1 as hi / lo fp16 B fragments, 96 VGPRs, and the dW1
// accumulators, 96), so
//   * each X tile is split once per layout and feeds both unit blocks' MFMAs;
//   * the 3-wide head is reduced inside the wave (A1 parked in the wave's LDS, row-on-lane reads,
//     one xor-32 exchange);
//   * no workgroup barrier: LDS order inside one wave, and the next tile's LDS-DMA in flight over
//     the whole compute of the current one;
//   * one wave per SIMD (up to 512 VGPRs), four workgroups per CU (~37 KB of LDS each).
// Same arithmetic per product as mlp2_kernel's SPLIT path (exponent-shifted 3-product fp16 split,
// fp32 accumulation), another summation order (per wave over its tiles; the reduce kernel sums the
// per-workgroup slabs in fixed order): deterministic, within the split's error bound.  The exact
// twin (mlp2_kernel<KH, ACT1, DROP, 4, false>, same grid and slabs) recomputes a flagged launch.
// ------------------------------------------------------------------------------------------------
#define MLP2R_NU 2  // 32-unit blocks per wave (F <= 64)
#define MLP2R_LDS_FLOATS (2 * MLP2_XF + 2 * MLP2_LAB + MLP2R_NU * MLP2_A1W + 32 * 4 + MLP2R_NU * 128 + 4)

template <int KH, int ACT1, bool DROP>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) mlp2r_kernel(Args args) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int NU = MLP2R_NU;
  constexpr int NKB = (2 * KH + 31) / 32;
  constexpr int T = 32;
  // Cin = 88: X tiles packed at the row stride 88 (11264 B = 11 full 64-lane LDS-DMA pieces per
  // tile instead of 32 one-row pieces: the piece issue cost was a fifth of the tile's cycles);
  // the forward's b128 reads take 2-way bank conflicts there.  Cin = 96 keeps the padded stride.
  constexpr int XS = KH == 44 ? 88 : MLP2_XS;
  const int* prog = args.prog;
  const int* o = prog + prog[H_OPS_OFF];
  const int Cin = o[O_K], F = o[O_N];
  const int lane = threadIdx.x, half = lane >> 5, l32 = lane & 31;
  float* xbuf = lds;                  // [2][MLP2_XF]: X tiles [32][XS] (double-buffered LDS-DMA)
  float* lbuf = xbuf + 2 * MLP2_XF;   // [2][32][4] labels
  float* a1p = lbuf + 2 * MLP2_LAB;   // [NU][MLP2_A1W] A1 park (a1_row slots)
  float* dz2 = a1p + NU * MLP2_A1W;   // [32][4] output gradients of the tile
  float* w2t = dz2 + 32 * 4;          // [NU * 32][4] W2 rows (zero past F)
  float* b2t = w2t + NU * 128;        // [4]
  const E2 e1 = {o[O_EACT], o[O_EDROP], (uint32_t)o[O_ETHR], __int_as_float(o[O_EKEEP])};
  const E2 e2 = {o[O_AUX2], o[O_TBASE], (uint32_t)o[O_TCOUNT], __int_as_float(o[O_F0])};
  const float inv_keep1 = 1.f / e1.keep, inv_keep2 = 1.f / e2.keep;
  const float* W1 = args.params + o[O_W];
  const float* W2 = args.params + o[O_AUX0];
  const int o_bias = __builtin_amdgcn_readfirstlane(o[O_BIAS]), o_aux1 = __builtin_amdgcn_readfirstlane(o[O_AUX1]);

  const int64_t nrows = args.nrows;
  const int64_t ntiles = (nrows + T - 1) / T;
  const int P = args.P;
  const int S = gridDim.x * T, dq = S / P, dr = S - dq * P;
  TileImg ti;
  ti.P = P;
  ti.img0 = (int)(blockIdx.x * T / P);
  ti.rem0 = (int)(blockIdx.x * T - ti.img0 * P);
  auto stage = [&](float* xd, float* ld, int64_t r0, const TileImg& t) {
    if (XS == 88 && !args.idx && P >= 32 && r0 + T <= nrows && Cin == 88) {
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) {
        const int slot = pc * 64 + lane;
        glds4(args.ytrue + (int64_t)t.of(slot >> 2) * 3 + min(slot & 3, 2), lds_addr(ld + pc * 64));
      }
#pragma unroll
      for (int i = 0; i < 11; ++i) glds16(args.x + r0 * 88 + 256 * i + 4 * lane, lds_addr(xd + 256 * i));
    } else {
      stage_tile(args, xd, ld, r0, t, 0, 1, lane, Cin, true, XS);
    }
  };
  if (blockIdx.x < ntiles) stage(xbuf, lbuf, (int64_t)blockIdx.x * T, ti);

  // ---- this wave's hidden units n = 32 u + l32: W1 columns split in registers, per-unit scalars ----
  SplitW wsp[NU][6];
  float inv1[NU], b1v[NU], s2[NU], nm[NU];  // nm: 1 for a unit below F, 0 past it (branch-free masks)
  f32x4 w2v[NU];
  bool nok[NU];
  {
    f32x8 v[NU][6];
    float w2r[NU][3], b1r[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int n = 32 * u + l32, nc = min(n, F - 1);
      nok[u] = n < F;
      nm[u] = nok[u] ? 1.f : 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j) w2r[u][j] = W2[nc * 3 + j];
      b1r[u] = args.params[max(o_bias, 0) + nc];
#pragma unroll
      for (int s = 0; s < 6; ++s) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = half * KH + 8 * s + j;
          v[u][s][j] = 8 * s + j < KH ? W1[(size_t)min(k, Cin - 1) * F + nc] : 0.f;
        }
      }
    }
    const float b2r = args.params[max(o_aux1, 0) + min(lane & 3, 2)];
    __builtin_amdgcn_sched_barrier(0);  // every prologue load in flight before the first use
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      float mx = 0.f;
#pragma unroll
      for (int s = 0; s < 6; ++s) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = half * KH + 8 * s + j;
          v[u][s][j] = (k < Cin && nok[u]) ? v[u][s][j] : 0.f;
          mx = fmaxf(mx, fabsf(v[u][s][j]));
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float s1 = pow2_scale(mx, 13);
      inv1[u] = SPLIT_INV_C / s1;
#pragma unroll
      for (int s = 0; s < 6; ++s) wsp[u][s] = split_w8(v[u][s] * s1);
      w2v[u] = nok[u] ? f32x4{w2r[u][0], w2r[u][1], w2r[u][2], 0.f} : f32x4{0.f, 0.f, 0.f, 0.f};
      s2[u] = pow2_scale(nok[u] ? fmaxf(fmaxf(fabsf(w2r[u][0]), fabsf(w2r[u][1])), fabsf(w2r[u][2])) : 0.f, 2);
      b1v[u] = (nok[u] && o_bias >= 0) ? b1r[u] : 0.f;
      if (half == 0) *(f32x4*)(w2t + (32 * u + l32) * 4) = w2v[u];
    }
    if (lane < 4) b2t[lane] = (lane < 3 && o_aux1 >= 0) ? b2r : 0.f;
  }
  // pad columns [C_in, 96) of both X buffers: read by the forward (against zero weights) and by the
  // dW1 blocks past C_in (never flushed) -> zeros, not stale LDS (the DMA writes [0, C_in))
  if (XS == 88) {
    // packed rows: the reads past channel 88 land in the next row (finite, against zero weights /
    // unflushed dW1 rows) and, for the last row, in the tile buffer's tail: zeros
    for (int i = lane; i < 2 * (MLP2_XF - 32 * 88); i += 64)
      xbuf[(i >= MLP2_XF - 32 * 88 ? MLP2_XF : 0) + 32 * 88 + i % (MLP2_XF - 32 * 88)] = 0.f;
  } else {
    for (int i = lane; i < 2 * 32 * 16; i += 64) {
      const int r = i >> 4, c = Cin + (i & 15);
      if (c < 96) xbuf[r * MLP2_XS + c] = 0.f;
    }
  }

  f32x16 dw[NU][NKB];
#pragma unroll
  for (int u = 0; u < NU; ++u)
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) dw[u][kb] = f32x16{};
  float dw2[NU][3], db1[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) { dw2[u][0] = dw2[u][1] = dw2[u][2] = 0.f; db1[u] = 0.f; }
  float sse = 0.f, sae = 0.f, db2[3] = {0.f, 0.f, 0.f};
  bool bad = false;

  int buf = 0;
#ifdef MLP2R_STAMPS
  uint32_t ph[7] = {};
  uint64_t tprev = __builtin_amdgcn_s_memtime();
#define RSTAMP(i) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); ph[i] += (uint32_t)(t_ - tprev); tprev = t_; } while (0)
#else
#define RSTAMP(i) do {} while (0)
#endif
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, buf ^= 1, ti.advance(dq, dr)) {
    const int64_t row0 = tile * T;
    RSTAMP(0);
    // tile `tile` landed; nothing else in flight -> the other buffer (read by the previous tile, all
    // of whose reads have returned) takes the next tile's LDS-DMA
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tile + gridDim.x < ntiles) {
      TileImg tn = ti;
      tn.advance(dq, dr);
      stage(xbuf + (buf ^ 1) * MLP2_XF, lbuf + (buf ^ 1) * MLP2_LAB, (tile + gridDim.x) * T, tn);
    }
    const float* xs = xbuf + buf * MLP2_XF;
    const float* lab = lbuf + buf * MLP2_LAB;
    RSTAMP(1);

    // ---- forward: Z1 = X.W1 for both unit blocks off one split of each X K-step ----
    f32x16 acc[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) acc[u] = f32x16{};
    {
      // one wave per SIMD: nothing hides a load's latency but the wave's own other work, so every
      // read of a phase is issued before its first use (here: the tile's 12 X reads, then split +
      // MFMA per K-step as they land)
      const float* ap = xs + l32 * XS + half * KH;
      f32x4 xa[12];
#pragma unroll
      for (int s = 0; s < 12; ++s) xa[s] = *(const f32x4*)(ap + 4 * s);
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        const f32x4 a0 = xa[2 * s], a1 = xa[2 * s + 1];
        const SplitD xd = split_d8(f32x8{a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w});
#pragma unroll
        for (int u = 0; u < NU; ++u) acc[u] = mfma3_dw(xd, wsp[u][s], acc[u]);
      }
    }
    RSTAMP(2);
    uint32_t dmask[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      bad |= !(fabsf(sum16(acc[u])) <= 3.0e38f);
      const int n = 32 * u + l32;
      dmask[u] = 0u;
      if (DROP) {
        if (P >= 32) {
          const bool k0 = drop_hash(args.seed, e1.drop, (uint64_t)(ti.img0 + args.img_off), n) >= e1.thr;
          const bool k1 = drop_hash(args.seed, e1.drop, (uint64_t)(ti.img0 + 1 + args.img_off), n) >= e1.thr;
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            const int r = (g & 3) + 8 * (g >> 2) + 4 * half;
            dmask[u] |= (ti.rem0 + r >= P ? k1 : k0) ? (1u << g) : 0u;
          }
        } else {
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            const int r = (g & 3) + 8 * (g >> 2) + 4 * half;
            dmask[u] |= drop_hash(args.seed, e1.drop, (uint64_t)(ti.of(r) + args.img_off), n) >= e1.thr ? (1u << g) : 0u;
          }
        }
      }
      // multiplies by 0 / 1 / inv_keep instead of selects: the compiler turns value selects over
      // several instructions into per-element branches, each behind its own LDS wait
      // A1 stays in acc for the backward; the park is for the head's row-on-lane reads
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const float km = DROP ? ((dmask[u] >> g) & 1u ? inv_keep1 : 0.f) : 1.f;
        acc[u][g] = act1_f<ACT1>(e1.act, fmaf(acc[u][g], inv1[u], b1v[u])) * km * nm[u];
        a1p[u * MLP2_A1W + a1_row(g) + lane] = acc[u][g];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    RSTAMP(3);
    // ---- head in the wave: lane (row r, half h) dots A1[r][32 u + 16 h ..] with the W2 rows ----
    {
      const int r = l32, hh = (r >> 2) & 1, gr = (r & 3) + 4 * (r >> 3);
      const f32x4 lv = *(const f32x4*)(lab + r * 4);
      float h0 = 0.f, h1 = 0.f, h2 = 0.f;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const float* ar = a1p + u * MLP2_A1W + a1_row(gr) + hh * 32 + 16 * half;
        const float* wr = w2t + (32 * u + 16 * half) * 4;
        f32x4 av[4], wv[16];  // the block's 20 reads in flight together
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = *(const f32x4*)(ar + 4 * i);
#pragma unroll
        for (int i = 0; i < 16; ++i) wv[i] = *(const f32x4*)(wr + 4 * i);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          h0 = fmaf(av[i >> 2][i & 3], wv[i].x, h0);
          h1 = fmaf(av[i >> 2][i & 3], wv[i].y, h1);
          h2 = fmaf(av[i >> 2][i & 3], wv[i].z, h2);
        }
      }
      h0 += __shfl_xor(h0, 32, 64);
      h1 += __shfl_xor(h1, 32, 64);
      h2 += __shfl_xor(h2, 32, 64);
      if (half == 0) {
        const bool valid = row0 + r < nrows;
        const bool d2 = __builtin_expect(e2.drop >= 0, 0);
        const int64_t img = d2 ? ti.of(r) + args.img_off : 0;
        const float zs[3] = {b2t[0] + h0, b2t[1] + h1, b2t[2] + h2};
        float gs[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const bool k2 = d2 ? drop_hash(args.seed, e2.drop, (uint64_t)img, j) >= e2.thr : true;
          const float kk = d2 ? (k2 ? inv_keep2 : 0.f) : 1.f;
          const float p = zs[j] * kk;
          float g = 0.f;
          if (valid) {
            const float err = p - lv[j];
            sse = fmaf(err, err, sse);
            sae += fabsf(err);
            g = 2.f * err;
          }
          g *= kk;
          db2[j] += g;
          gs[j] = g;
        }
        *(f32x4*)(dz2 + r * 4) = f32x4{gs[0], gs[1], gs[2], 0.f};
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    RSTAMP(4);
    // ---- backward: dZ1 per unit block (registers), dW2 / db1, dW1 += X^T.dZ1 off one X^T split ----
    // the 16 rows' dZ2 of this lane's half and the tile's X^T reads (both K-steps), all in flight
    f32x4 dzr[16];
#pragma unroll
    for (int g = 0; g < 16; ++g) dzr[g] = *(const f32x4*)(dz2 + ((g & 3) + 8 * (g >> 2) + 4 * half) * 4);
    f32x8 xtr[2][NKB];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          xtr[s][kb][j] = xs[(4 * half + 16 * s + 8 * (j >> 2) + (j & 3)) * XS + kb * 32 + l32];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      f32x8 dv[NU];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int g = 8 * s + j;
        const f32x4 d = dzr[g];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const float a = acc[u][g];
          const float da = d.x * w2v[u].x + d.y * w2v[u].y + d.z * w2v[u].z;
          const float km = DROP ? ((dmask[u] >> g) & 1u ? inv_keep1 : 0.f) : 1.f;
          const float gz = da * km * act1_g<ACT1>(e1.act, DROP ? a * e1.keep : a) * nm[u];
          dw2[u][0] = fmaf(a, d.x, dw2[u][0]);
          dw2[u][1] = fmaf(a, d.y, dw2[u][1]);
          dw2[u][2] = fmaf(a, d.z, dw2[u][2]);
          db1[u] += gz;
          dv[u][j] = gz;
        }
      }
      SplitW dsp[NU];
#pragma unroll
      for (int u = 0; u < NU; ++u) dsp[u] = split_w8(dv[u] * s2[u]);
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        const SplitD xd = split_d8(xtr[s][kb]);
#pragma unroll
        for (int u = 0; u < NU; ++u) dw[u][kb] = mfma3_dw(xd, dsp[u], dw[u][kb]);
      }
      if (s == 0) RSTAMP(5);
    }
    RSTAMP(6);
  }
#ifdef MLP2R_STAMPS
  if (blockIdx.x < 2 && lane == 0)
    printf("RSTAMP wg %d top %u stage %u fwd %u act %u head %u bwd0 %u bwd1 %u\n", (int)blockIdx.x, ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], ph[6]);
#endif

  // ---- flush this workgroup's partial gradients + loss sums (mlp2_kernel's slab layout) ----
  const int slab = prog[H_SLAB];
  const int npt = prog[H_NPARAMS_TRAIN];
  float* ws = args.ws + (size_t)blockIdx.x * slab;
  const float sc = args.inv_count;
  const int oW = __builtin_amdgcn_readfirstlane(o[O_W]), oA0 = __builtin_amdgcn_readfirstlane(o[O_AUX0]);
  float chk = 0.f;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int n = 32 * u + l32;
    const float scw = sc * (SPLIT_INV_C / s2[u]);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      chk += sum16(dw[u][kb]);
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int k = kb * 32 + (g & 3) + 8 * (g >> 2) + 4 * half;
        if (k < Cin && nok[u]) ws[oW + (size_t)k * F + n] = dw[u][kb][g] * scw;
      }
    }
    const float tb = db1[u] + __shfl_xor(db1[u], 32, 64);
    float t2[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) t2[j] = dw2[u][j] + __shfl_xor(dw2[u][j], 32, 64);
    if (half == 0 && nok[u]) {
      if (o_bias >= 0) ws[o_bias + n] = tb * sc;
#pragma unroll
      for (int j = 0; j < 3; ++j) ws[oA0 + n * 3 + j] = t2[j] * sc;
    }
  }
  bad |= !(fabsf(chk) <= 3.0e38f);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float t = wave_sum(db2[j]);
    if (lane == 0 && o_aux1 >= 0) ws[o_aux1 + j] = t * sc;
  }
  if (bad) __hip_atomic_store(args.guard, args.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float ta = wave_sum(sse), tb = wave_sum(sae);
  if (lane == 0) {
    ws[npt] = ta;
    ws[npt + 1] = tb;
  }
}
#endif

// ---- host-side dispatch ---------------------------------------------------------------------
typedef void (*mlp2_fn)(Args);

template <int KH, bool DROP, int NWM, bool SPLIT, bool CONTIG = false>
static mlp2_fn pick_act(int act, int act2) {
  if (act2 != ACT_LINEAR) return mlp2_kernel<KH, -1, DROP, NWM, SPLIT, CONTIG>;
  if (act == ACT_TANH) return mlp2_kernel<KH, ACT_TANH, DROP, NWM, SPLIT, CONTIG>;
  if (act == ACT_SOFTSIGN) return mlp2_kernel<KH, ACT_SOFTSIGN, DROP, NWM, SPLIT, CONTIG>;
  return mlp2_kernel<KH, -1, DROP, NWM, SPLIT, CONTIG>;
}

// contig: the contiguous-rows instantiation of the 12-wave split kernel (ignored by the others)
template <bool DROP, bool SPLIT>
static mlp2_fn pick_d(int kh, int act, int act2, int ncb, bool contig) {
  if (ncb <= 4) {
    if (kh == 44) return pick_act<44, DROP, 4, SPLIT>(act, act2);  // 88-channel BlazeFace tap (Model-88)
    if (kh == 48) return pick_act<48, DROP, 4, SPLIT>(act, act2);  // 96-channel tap (Model-96)
  }
  if constexpr (SPLIT) {
    if (contig && kh == 44) return pick_act<44, DROP, MLP2_MAXW, SPLIT, true>(act, act2);
    if (contig && kh == 48) return pick_act<48, DROP, MLP2_MAXW, SPLIT, true>(act, act2);
  }
  if (kh == 44) return pick_act<44, DROP, MLP2_MAXW, SPLIT>(act, act2);
  if (kh == 48) return pick_act<48, DROP, MLP2_MAXW, SPLIT>(act, act2);
  return nullptr;
}

static mlp2_fn pick(const int* w, bool split = false, bool contig = false) {
  const int* o = w + w[H_OPS_OFF];
  const int kh = ((o[O_K] + 7) & ~7) / 2, act = o[O_EACT], act2 = o[O_AUX2];
  if (split)
    return o[O_EDROP] >= 0 ? pick_d<true, true>(kh, act, act2, o[O_MODE], contig) : pick_d<false, true>(kh, act, act2, o[O_MODE], contig);
  return o[O_EDROP] >= 0 ? pick_d<true, false>(kh, act, act2, o[O_MODE], false) : pick_d<false, false>(kh, act, act2, o[O_MODE], false);
}

static void geom(const int* w, int& kh, int& rbw, int& ncb, int& lds_bytes, int& act, int& drop) {
  const int* o = w + w[H_OPS_OFF];
  act = o[O_EACT];
  drop = o[O_EDROP];
  const int cin = o[O_K];
  const int cp = (cin + 7) & ~7;
  kh = cp / 2;
  rbw = o[O_FLAGS];
  ncb = o[O_MODE];
  const int T = 32;
  const int npr = ncb > 4 ? MLP2_MAXW : ncb;  // head partial rows (the 12-wave kernels keep all twelve)
  const int rest = 2 * MLP2_LAB + npr * T * 4 + T * 4 + ncb * MLP2_A1W + ncb * 128 + 4 + ncb * 64 * (ncb > 4 ? 4 : 3) + MLP2_RED + ncb * 128;
  lds_bytes = (2 * MLP2_XF + rest) * 4;
  // the 12-wave variant's split kernel (PRE): one raw tile buffer + the two parities of the fp16 image
  const int pre = (MLP2_XF + rest) * 4 + MLP2_PRE_HALVES * 2;
  if (ncb > 4 && pre > lds_bytes) lds_bytes = pre;
}

// LDS of the split instantiation pick(w, true) launches
static int lds_split(const int* w) {
  int kh, rbw, ncb, lds, act, drop;
  geom(w, kh, rbw, ncb, lds, act, drop);
  return lds;
}

static int launch_k(mlp2_fn k, int nw, int lds, const Args& a, int grid, hipStream_t s) {
  hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(k, dim3(grid), dim3(nw * 64), lds, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// HPE_SPLIT_ONLY=1 (race screens): no exact twin behind a split launch, so a launch whose guard
// fired keeps the split kernel's own (non-finite or perturbed) result
static bool split_only() {
  const char* e = getenv("HPE_SPLIT_ONLY");
  return e && e[0] == '1';
}

#ifdef MLP2_BIG
// the row-parallel split kernel for this training program, or null: F <= 64, linear head, layer-1
// activation compiled in; HPE_MLP2_ROWS=0 keeps mlp2_kernel (A/B, tests)
template <int KH>
static mlp2_fn pick_r_act(int act, bool drop) {
  if (act == ACT_TANH) return drop ? mlp2r_kernel<KH, ACT_TANH, true> : mlp2r_kernel<KH, ACT_TANH, false>;
  if (act == ACT_SOFTSIGN) return drop ? mlp2r_kernel<KH, ACT_SOFTSIGN, true> : mlp2r_kernel<KH, ACT_SOFTSIGN, false>;
  return nullptr;
}
static mlp2_fn pick_r(const int* w) {
  const char* e = getenv("HPE_MLP2_ROWS");
  if ((e && e[0] == '0') || w[H_MODE] != MODE_TRAIN) return nullptr;
  const int* o = w + w[H_OPS_OFF];
  if (o[O_MODE] > MLP2R_NU || o[O_N] > 32 * MLP2R_NU || o[O_AUX2] != ACT_LINEAR) return nullptr;
  const int kh = ((o[O_K] + 7) & ~7) / 2;
  if (kh == 44 && o[O_K] == 88) return pick_r_act<44>(o[O_EACT], o[O_EDROP] >= 0);  // packed 88-float rows
  if (kh == 48) return pick_r_act<48>(o[O_EACT], o[O_EDROP] >= 0);
  return nullptr;
}
#else
static mlp2_fn pick_r(const int*) { return nullptr; }
#define MLP2R_LDS_FLOATS 0
#endif

// split instantiation, then the exact one, which exits at once unless the split launch flagged a
// non-finite value (guard == epoch); hpe_set_exact_fp32(1): the exact kernel alone
static int launch_pair(const int* w, const Args& a, int grid, hipStream_t s) {
  int kh, rbw, ncb, lds, act, drop;
  geom(w, kh, rbw, ncb, lds, act, drop);
  if (hpe_exact_fp32() || !a.guard) {
    Args e = a;
    e.guard = nullptr;
    const int tv = hpe_tev_begin(s);
    const int rc = launch_k(pick(w), ncb, lds, e, grid, s);
    hpe_tev_end(s, tv);
    return rc;
  }
  const mlp2_fn kr = pick_r(w);
  const int tv = hpe_tev_begin(s);
  // contiguous rows, at most two images per tile: the 12-wave split kernel's CONTIG instantiation
  const bool contig = a.idx == nullptr && a.P >= 32;
  const int rc = kr ? launch_k(kr, 1, MLP2R_LDS_FLOATS * 4, a, grid, s) : launch_k(pick(w, true, contig), ncb, lds_split(w), a, grid, s);
  hpe_tev_end(s, tv);
  if (rc) return rc;
  if (split_only()) return 0;
  // inputs the caller bounds below the data-side range: the guard cannot fire (finite weights are
  // scaled into range), so the exact twin's early-exit launch is not queued
  if (a.x_bound > 0.f && a.x_bound < SPLIT_DATA_RANGE) return 0;
  return launch_k(pick(w), ncb, lds, a, grid, s);
}

static int per_cu_of(mlp2_fn k, int ncb, int lds) {
  hipFuncAttributes attr;
  int per_cu = 1;
  if (hipFuncGetAttributes(&attr, (const void*)k) == hipSuccess) {
    const int vg = ((attr.numRegs + 7) / 8) * 8;
    const int waves_simd = vg > 0 ? (512 / vg > 8 ? 8 : 512 / vg) : 8;
    per_cu = (4 * waves_simd) / ncb;
  }
  const int by_lds = (160 * 1024) / lds;
  if (per_cu > by_lds) per_cu = by_lds;
  return per_cu < 1 ? 1 : per_cu;
}

// resident workgroups per CU of this object's kernels for program w: the smallest of the exact, the
// split (general and contiguous-rows) and the row-parallel instantiations
static int cap_per_cu(const int* w) {
  int kh, rbw, ncb, lds, act, drop;
  geom(w, kh, rbw, ncb, lds, act, drop);
  int cap = per_cu_of(pick(w), ncb, lds);
  const int b = per_cu_of(pick(w, true), ncb, lds_split(w)), bc = per_cu_of(pick(w, true, true), ncb, lds_split(w));
  cap = b < cap ? b : cap;
  cap = bc < cap ? bc : cap;
  const mlp2_fn kr = pick_r(w);
  if (kr) {
    const int c = per_cu_of(kr, 1, MLP2R_LDS_FLOATS * 4);
    cap = c < cap ? c : cap;
  }
  return cap;
}
}  // namespace MLP2_NS

#ifdef MLP2_BIG
int mlp2_launch_big(const int* w, const Args& a, int grid, hipStream_t s) {
  return MLP2_NS::launch_pair(w, a, grid, s);
}
int mlp2_per_cu_big(const int* w) { return MLP2_NS::cap_per_cu(w); }
#else
using namespace MLP2_NS;
int mlp2_launch_big(const int* w, const Args& a, int grid, hipStream_t s);
int mlp2_per_cu_big(const int* w);

int mlp2_supported(const int* w) {
  int kh, rbw, ncb, lds, act, drop;
  geom(w, kh, rbw, ncb, lds, act, drop);
  const int* o = w + w[H_OPS_OFF];
  return pick(w) != nullptr && rbw == 1 && ncb >= 1 && ncb <= MLP2_MAXW &&
         o[O_AUX3] == 3 && (o[O_K] & 3) == 0 && o[O_K] <= 96 && lds <= 160 * 1024;
}

// one grid for both instantiations and both objects (the exact one recomputes a flagged split
// launch into the same per-workgroup slabs; launches of >= MLP2_BIG_ROWS rows run the MLP2_BIG
// object, whose register counts differ): the smallest of their occupancies
int mlp2_grid_cap(const int* w, int n_cu) {
  const int a = MLP2_NS::cap_per_cu(w), b = mlp2_per_cu_big(w);
  return n_cu * (a < b ? a : b);
}

int mlp2_launch(const int* w, const Args& a, int grid, hipStream_t s) {
  if (a.nrows >= MLP2_BIG_ROWS) return mlp2_launch_big(w, a, grid, s);
  return launch_pair(w, a, grid, s);
}
#endif
