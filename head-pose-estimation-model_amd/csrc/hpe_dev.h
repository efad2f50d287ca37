// hpe_dev.h — device helpers shared by the fused regressor kernels (hpe_mlp2.hip, hpe_fit.hip):
// LDS-DMA staging, an LDS-only workgroup barrier, and the layer-1 activations of the hot loops.
#pragma once
#include <type_traits>
#include <utility>

#include "hpe_common.h"

// LDS-DMA (global_load_lds) in inline asm: hipcc's waitcnt pass cannot tell the two X buffers
// apart and would put vmcnt(0) before every ds_read of the tile in use, draining the prefetch of
// the next one; hidden from it, the prefetch completes only at the explicit vmcnt(0) before the
// barrier that opens its tile.  M0 is written in the same statement (compiler-reserved).
// the low 32 bits of a flat (generic) pointer into LDS are the LDS byte address (the high half is
// the shared aperture); no generic -> local addrspacecast (its null check miscompiles on constants)
__device__ __forceinline__ uint32_t lds_addr(const float* p) {
  return __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)p);
}
// HPE_GLDS_NT: the X stream's pieces non-temporal (read once per launch)
#ifdef HPE_GLDS_NT
#define HPE_GLDS16_OP "global_load_lds_dwordx4 %1, off nt"
#else
#define HPE_GLDS16_OP "global_load_lds_dwordx4 %1, off"
#endif
__device__ __forceinline__ void glds16(const float* gsrc, uint32_t lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t" HPE_GLDS16_OP "\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void glds4(const float* gsrc, uint32_t lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// raw workgroup barrier that waits for LDS traffic only: an in-flight global_load_lds prefetch of
// the next tile survives it (__syncthreads() would drain it with vmcnt(0))
__device__ __forceinline__ void bar_lds() {
  asm volatile("" ::: "memory");       // no LDS access moves across it
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// DPP row broadcast folded into the consuming VALU op (VOP2 DPP, row_newbcast:N): every lane of a
// 16-lane row takes lane N of its own row as the op's first source — a table that a lane half shares
// sits one entry per lane in a VGPR and costs neither an LDS read nor a separate move per use (hipcc
// emits a v_mov_b32_dpp per use from __builtin_amdgcn_update_dpp, hence the asm).  tests/
// test_gpu_bcast_probe.py holds the instruction's meaning through hpe_bcast_probe.  Rules of use:
//   * EXEC all ones (a disabled source lane reads as zero);
//   * a VALU write of the table register followed by its DPP read needs two wait states, which hipcc
//     does not pad around an asm statement: dpp_settle3 between the table's definition and its uses
//     (an LDS read's s_waitcnt does not cover a register copy the allocator may put behind it)
__device__ __forceinline__ void dpp_settle3(float& a, float& b, float& c) {
  asm volatile("s_nop 1" : "+v"(a), "+v"(b), "+v"(c));
}
// one instruction: d = fma(bcast_n(t), x, d) / d = bcast_n(t) * x, operands by asm operand number
#define HPE_DPP_CTRL(n) " row_newbcast:%c" #n " row_mask:0xf bank_mask:0xf\n\t"
#define HPE_FMAC_BCAST(d, t, x, n) "v_fmac_f32_dpp %" #d ", %" #t ", %" #x HPE_DPP_CTRL(n)
#define HPE_MUL_BCAST(d, t, x, n) "v_mul_f32_dpp %" #d ", %" #t ", %" #x HPE_DPP_CTRL(n)
template <int N>
__device__ __forceinline__ float fmac_bcast(float acc, float t, float x) {
  asm(HPE_FMAC_BCAST(0, 1, 2, 3) : "+v"(acc) : "v"(t), "v"(x), "i"(N));
  return acc;
}
template <int N>
__device__ __forceinline__ float mul_bcast(float t, float x) {
  float r;
  asm(HPE_MUL_BCAST(0, 1, 2, 3) : "=v"(r) : "v"(t), "v"(x), "i"(N));
  return r;
}
// the same instructions in the groups the fused kernel issues (one statement per group: hipcc pads
// every asm statement whose result the next one reads with an s_nop of its own)
// s_j = fma(bcast_{K + e}(t_j), a[e], s_j) for e = 0 .. 3, j = 0 .. 2 (e outer)
template <int K>
__device__ __forceinline__ void fmac3x4_bcast(float& s0, float& s1, float& s2, float t0, float t1, float t2, f32x4 a) {
  asm(HPE_FMAC_BCAST(0, 3, 6, 10) HPE_FMAC_BCAST(1, 4, 6, 10) HPE_FMAC_BCAST(2, 5, 6, 10)
      HPE_FMAC_BCAST(0, 3, 7, 11) HPE_FMAC_BCAST(1, 4, 7, 11) HPE_FMAC_BCAST(2, 5, 7, 11)
      HPE_FMAC_BCAST(0, 3, 8, 12) HPE_FMAC_BCAST(1, 4, 8, 12) HPE_FMAC_BCAST(2, 5, 8, 12)
      HPE_FMAC_BCAST(0, 3, 9, 13) HPE_FMAC_BCAST(1, 4, 9, 13) HPE_FMAC_BCAST(2, 5, 9, 13)
      : "+v"(s0), "+v"(s1), "+v"(s2)
      : "v"(t0), "v"(t1), "v"(t2), "v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "i"(K), "i"(K + 1), "i"(K + 2), "i"(K + 3));
}
// f(integral_constant<int, I>) for I = B .. B + N - 1, in order (the DPP lane is an immediate)
template <int B, int... I, class Fn>
__device__ __forceinline__ void static_for_seq(std::integer_sequence<int, I...>, Fn&& f) {
  (f(std::integral_constant<int, B + I>{}), ...);
}
template <int B, int N, class Fn>
__device__ __forceinline__ void static_for(Fn&& f) {
  static_for_seq<B>(std::make_integer_sequence<int, N>{}, f);
}

// activation of layer 1 fixed at compile time (tanh: Model-96, softsign: Model-88); ACT1 = -1 is
// the runtime-dispatched variant for the other activations the checkpoints use
// tanh in 5 VALU ops for the fp16-split hot loops, 1 - 2 / (1 + e^{2z}) (e^{2z} -> inf gives 1,
// -> 0 gives -1).  Its error is ABSOLUTE: |fast_tanh5(z) - tanh(z)| <= 2^-22 (2.4e-7) over all z
// (tests/test_gpu_activations.py measures it against float64 through hpe_act_probe), so for
// |z| << 1 the relative error grows (~1e-3 at |z| = 1e-4) where tanhf is relatively accurate.
// The exact-fp32 kernels (the split kernels' overflow twins, HPE_EXACT_FP32=1, the residual-stack
// kernels) use tanhf (FAST = false), so the split-vs-exact error bars are anchored to fp32 tanh.
// Derivative 1 - a^2 as in Keras' TanhGrad.
__device__ __forceinline__ float fast_tanh5(float z) {
  const float e = __builtin_amdgcn_exp2f(z * 2.8853900817779268f);  // 2 log2(e)
  return fmaf(-2.f, __builtin_amdgcn_rcpf(1.f + e), 1.f);
}
template <int ACT1, bool FAST = true>
__device__ __forceinline__ float act1_f(int act, float z) {
  if (ACT1 == ACT_TANH) return FAST ? fast_tanh5(z) : tanhf(z);
  if (ACT1 == ACT_SOFTSIGN) return z * __builtin_amdgcn_rcpf(1.f + fabsf(z));
  return act_f(ACT1 >= 0 ? ACT1 : act, z);
}
template <int ACT1>
__device__ __forceinline__ float act1_g(int act, float a) {
  const int k = ACT1 >= 0 ? ACT1 : act;
  return k == ACT_LINEAR ? 1.f : act_grad(k, a, 0.f);
}

