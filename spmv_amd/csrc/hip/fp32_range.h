// The range rule of the fp32 value stream of the multicolour sweeps
// (SgsOptions::values = fp32), plain C++ shared by the device kernels that
// narrow (spmv_mcgs.hip, spmv_ilu0.hip) and the host (spmvh_fp32_range_count).
//
// A stored value is the fp64 value rounded to nearest-even.  A finite non-zero
// value whose rounding is +-Inf, zero or an fp32 subnormal is OUT OF RANGE: the
// plan must not depend on the denormal mode of whoever converts, and a factor
// entry that silently becomes 0 or Inf is another preconditioner.  +-0, +-Inf
// and NaN convert as IEEE says and are in range.
//
// The rule is stated on the magnitude of the double, so that it does not
// depend on how a conversion treats subnormals either:
//   |v| >= 2^128 - 2^103        rounds to Inf (FLT_MAX + half an ulp; the tie
//                               goes to the even neighbour, which is 2^128)
//   |v| <  2^-126 - 2^-150      rounds below FLT_MIN (the tie between the
//                               largest subnormal and 2^-126 goes to 2^-126)
#pragma once

#if defined(__HIPCC__)
#define SPMV_FP32_RANGE_FN __host__ __device__ inline
#else
#define SPMV_FP32_RANGE_FN inline
#endif

SPMV_FP32_RANGE_FN bool spmv_fp32_out_of_range(double v)
{
  const double a = v < 0.0 ? -v : v;
  constexpr double kInf = __builtin_huge_val();
  constexpr double kRoundsToInf = 0x1p128 - 0x1p103;
  constexpr double kRoundsToNormal = 0x1p-126 - 0x1p-150;
  return a > 0.0 && a < kInf && (a >= kRoundsToInf || a < kRoundsToNormal);
}
