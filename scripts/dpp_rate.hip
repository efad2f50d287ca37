// DPP-operand issue-rate probe (gfx950): cycles per instruction of v_fmac_f32_dpp row_newbcast (the
// row broadcast folded into the FMA, csrc/hpe_dev.h) against plain v_fmac_f32 —
//   * a stream of 16 independent accumulators from one wave per SIMD (256 threads),
//   * the same from three waves per SIMD (768 threads: mlp2_kernel's occupancy),
//   * both with one v_mfma_f32_32x32x16_f16 (4 independent accumulators) after every 8 FMAs.
// Prints cycles per FMA as one wave sees them and per SIMD (the wave's cycles / waves per SIMD).
//   hipcc --offload-arch=gfx950 -O3 scripts/dpp_rate.hip -o scripts/dpp_rate
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CTRL " row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
#define F1(OP, SFX, d) OP " %" #d ", %8, %9" SFX
#define F8(OP, SFX) F1(OP, SFX, 0) F1(OP, SFX, 1) F1(OP, SFX, 2) F1(OP, SFX, 3) F1(OP, SFX, 4) F1(OP, SFX, 5) F1(OP, SFX, 6) F1(OP, SFX, 7)
#define ACC8(a) "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7])

template <bool DPP>
__device__ __forceinline__ void fma8(float (&a)[8], float t, float x) {
  if (DPP) asm volatile(F8("v_fmac_f32_dpp", CTRL) : ACC8(a) : "v"(t), "v"(x));
  else asm volatile(F8("v_fmac_f32_e32", "\n\t") : ACC8(a) : "v"(t), "v"(x));
}

template <bool DPP, bool MFMA>
__global__ void __launch_bounds__(768) probe(float* out, unsigned long long* cyc, int n) {
  const int l = threadIdx.x & 63;
  float a[8], b[8];
  for (int j = 0; j < 8; ++j) a[j] = b[j] = 0.f;
  float t = 1.f + l * 1e-3f, x = 1e-3f;
  asm volatile("s_nop 1" : "+v"(t), "+v"(x));
  const h8 hv = {(_Float16)(l * 0.01f), (_Float16)1.f, (_Float16)0.5f, (_Float16)0.25f,
                 (_Float16)0.125f, (_Float16)1.f, (_Float16)0.5f, (_Float16)0.25f};
  f32x16 c0 = {}, c1 = {}, c2 = {}, c3 = {};
  __builtin_amdgcn_s_barrier();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int i = 0; i < n; ++i) {
    fma8<DPP>(a, t, x);
    __builtin_amdgcn_sched_barrier(0);
    if (MFMA) c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(hv, hv, c0, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    fma8<DPP>(b, t, x);
    __builtin_amdgcn_sched_barrier(0);
    if (MFMA) c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(hv, hv, c1, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    fma8<DPP>(a, t, x);
    __builtin_amdgcn_sched_barrier(0);
    if (MFMA) c2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(hv, hv, c2, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    fma8<DPP>(b, t, x);
    __builtin_amdgcn_sched_barrier(0);
    if (MFMA) c3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(hv, hv, c3, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  float s = 0.f;
  for (int j = 0; j < 16; ++j) s += a[j & 7] + b[j & 7] + c0[j] + c1[j] + c2[j] + c3[j];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
  if (l == 0) cyc[threadIdx.x >> 6] = t1 - t0;
}

template <bool DPP, bool MFMA>
static void run(const char* name, float* out, unsigned long long* cyc, int n) {
  for (int waves = 4; waves <= 12; waves += 8) {
    for (int rep = 0; rep < 2; ++rep) {
      hipLaunchKernelGGL((probe<DPP, MFMA>), dim3(1), dim3(64 * waves), 0, 0, out, cyc, n);
      if (hipDeviceSynchronize() != hipSuccess) { printf("%s: launch failed\n", name); return; }
    }
    unsigned long long h[12];
    hipMemcpy(h, cyc, sizeof(unsigned long long) * waves, hipMemcpyDeviceToHost);
    unsigned long long mx = 0;
    for (int w = 0; w < waves; ++w) mx = h[w] > mx ? h[w] : mx;
    const double per = (double)mx / (32.0 * n);
    printf("%-22s %2d waves (%d per SIMD): %.2f cycles per FMA per wave, %.2f per SIMD%s\n", name, waves, waves / 4,
           per, per / (waves / 4), MFMA ? " (one 8-pass MFMA per 8 FMAs)" : "");
  }
}

int main() {
  float* out;
  unsigned long long* cyc;
  if (hipMalloc(&out, 768 * 4) != hipSuccess || hipMalloc(&cyc, 12 * 8) != hipSuccess) return 1;
  const int n = 2000;
  run<false, false>("v_fmac_f32", out, cyc, n);
  run<true, false>("v_fmac_f32_dpp", out, cyc, n);
  run<false, true>("v_fmac_f32 + mfma", out, cyc, n);
  run<true, true>("v_fmac_f32_dpp + mfma", out, cyc, n);
  return 0;
}
