// Float64 arithmetic that the compiler may not contract, for the kernels that are held bit for bit against a numpy
// restatement (tests/*_ref.py).
// hipcc fuses a multiply and an add into v_fma_f64 / v_fmac_f64 by default, even through __dmul_rn / __dadd_rn (the
// HIP headers define those before an including file's first line, so no pragma there reaches them).  Products and sums
// therefore go through mul / add / sub, plain operators under the pragma.  The only fused instructions left are inside
// the correctly rounded __ddiv_rn / __dsqrt_rn expansions (tests/test_*_asm.py).
// A .hip that includes this header still opens with the pragma as its own first code line: its kernels must not depend
// on where an #include stands.  Only helpers whose operation order is the same for every user live here; a file whose
// dot product or cross product takes other operands keeps its own.
#pragma once
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <math.h>

__device__ __forceinline__ double mul(double x, double y) { return x * y; }
__device__ __forceinline__ double add(double x, double y) { return x + y; }
__device__ __forceinline__ double sub(double x, double y) { return x - y; }

// (x x + y y) + z z
__device__ __forceinline__ double dot3(double x, double y, double z) {
  return add(add(mul(x, x), mul(y, y)), mul(z, z));
}

__host__ __device__ __forceinline__ bool is_finite(double x) { return fabs(x) < HUGE_VAL; }     // false for NaN
__host__ __device__ __forceinline__ bool positive_finite(double x) { return x > 0.0 && x < HUGE_VAL; }

struct V3 {
  double x, y, z;
};

__device__ __forceinline__ V3 vload(const double* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ V3 vsub(const V3& a, const V3& b) { return {sub(a.x, b.x), sub(a.y, b.y), sub(a.z, b.z)}; }
__device__ __forceinline__ double vdot(const V3& a, const V3& b) {
  return add(add(mul(a.x, b.x), mul(a.y, b.y)), mul(a.z, b.z));
}
__device__ __forceinline__ V3 vcross(const V3& a, const V3& b) {          // np.cross order
  return {sub(mul(a.y, b.z), mul(a.z, b.y)), sub(mul(a.z, b.x), mul(a.x, b.z)), sub(mul(a.x, b.y), mul(a.y, b.x))};
}
