// The per-element arithmetic of the Chebyshev steps (blas1_cheb.hip) and of the
// AMG cycle (spmv_amg.hip), one definition for the streaming kernels and for the
// fused tail kernel, so that both give the same bits.  Built with
// -ffp-contract=off: every product, sum and difference is a rounding of its own.
#pragma once

#include <cstdint>

// dinv*v, or v itself without a preconditioner diagonal
template <bool PRE>
__device__ __forceinline__ double scaled(double dv, double v)
{
  return PRE ? dv * v : v;
}

// step 0 from z = 0: d = b0 * (dinv*r)
template <bool PRE>
__device__ __forceinline__ double cheb_first(double b0, double dv, double r)
{
  return b0 * scaled<PRE>(dv, r);
}

// the correction of a later step: b * (dinv*(r - w)); with b = b_0 it is step 0
// of an iteration continued from the current z (amg_post0)
template <bool PRE>
__device__ __forceinline__ double cheb_corr(double b, double dv, double r,
                                            double w)
{
  return b * scaled<PRE>(dv, r - w);
}

// d = a*d + t
__device__ __forceinline__ double cheb_next(double a, double d, double t)
{
  const double ad = a * d;
  return ad + t;
}

// z[i] + scale * e[agg(i)]
__device__ __forceinline__ double amg_prolong_elem(double z, double scale,
                                                   double e)
{
  const double t = scale * e;
  return z + t;
}

// the two operations of amg_restrict_sum, for the block kernels
// (spmv_amg_block.hip), which keep one sum per column and walk the members once
__device__ __forceinline__ double amg_restrict_term(double r, double w)
{
  return r - w;
}
__device__ __forceinline__ double amg_restrict_add(double acc, double t)
{
  return acc + t;
}

// rc[I] = (t_0 + t_1) + ..., t_m = r[i_m] - w[i_m] over member[m0 .. m1)
__device__ __forceinline__ double amg_restrict_sum(int32_t m0, int32_t m1,
                                                   const int32_t* member,
                                                   const double* r,
                                                   const double* w)
{
  double acc = 0.0; // (an aggregate has a member)
  if (m0 < m1) {
    const int32_t i = member[m0];
    acc = r[i] - w[i];
  }
  for (int32_t m = m0 + 1; m < m1; ++m) {
    const int32_t i = member[m];
    const double t = r[i] - w[i];
    acc = acc + t;
  }
  return acc;
}
