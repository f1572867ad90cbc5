/*
 * vs_ac_corr.h -- the correlation core the period kernel (vs_acoustic.hip) and the candidate kernel of the pitch track
 * (vs_pitch.hip) share.  Device code only.
 *
 * A window of W samples lies in LDS as doubles, with tmax + 1 samples behind it and zeros behind those
 * (vs_ac_xs_doubles).  The lags tlo .. tlo + nl - 1 are dealt four adjacent lags to a thread, the k range cut into as
 * many segments as the threads left over allow.  A thread walks its k segment with a window of seven samples in
 * registers: sixteen fp64 FMAs for eight LDS reads (four of them the same address for every lane).  Products of int16
 * samples are below 2^30 and every partial sum below 2^53, so the sums are EXACT integers and their order does not
 * matter: any caller, any grouping, the same bits.
 */
#ifndef VS_AC_CORR_H
#define VS_AC_CORR_H

#include <hip/hip_runtime.h>

#define VS_AC_A_THREADS 256

/* r(t) = sum_{k<W} xs[k] * xs[k + t] into rp[t - tlo], t - tlo in [0, nl).  rp holds vs_ac_rp_doubles doubles.  Every
 * thread of the workgroup (VS_AC_A_THREADS) calls it, behind a barrier after xs was written; it returns behind one. */
__device__ __forceinline__ void vs_ac_lag_sums(const double *xs, double *rp, int tlo, int nl, int W, int tid)
{
  const int G = (nl + 3) / 4;                 /* groups of four adjacent lags */
  const int S = G >= VS_AC_A_THREADS ? 1 : VS_AC_A_THREADS / G; /* k segments */
  const int seglen = (W + S - 1) / S;
  for (int it = tid; it < G * S; it += VS_AC_A_THREADS) {
    const int g = it % G, sg = it / G;
    const int t0 = tlo + 4 * g;
    const int k0 = sg * seglen, k1 = min(W, k0 + seglen);
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    int k = k0;
    if (k + 4 <= k1) {
      const double *v = xs + t0;
      double v4 = v[k], v5 = v[k + 1], v6 = v[k + 2];
      for (; k + 4 <= k1; k += 4) {
        const double v0 = v4, v1 = v5, v2 = v6, v3 = v[k + 3];
        v4 = v[k + 4];
        v5 = v[k + 5];
        v6 = v[k + 6];
        const double a0 = xs[k], a1 = xs[k + 1], a2 = xs[k + 2], a3 = xs[k + 3];
        c0 = fma(a0, v0, c0); c1 = fma(a0, v1, c1); c2 = fma(a0, v2, c2); c3 = fma(a0, v3, c3);
        c0 = fma(a1, v1, c0); c1 = fma(a1, v2, c1); c2 = fma(a1, v3, c2); c3 = fma(a1, v4, c3);
        c0 = fma(a2, v2, c0); c1 = fma(a2, v3, c1); c2 = fma(a2, v4, c2); c3 = fma(a2, v5, c3);
        c0 = fma(a3, v3, c0); c1 = fma(a3, v4, c1); c2 = fma(a3, v5, c2); c3 = fma(a3, v6, c3);
      }
    }
    for (; k < k1; k++) {
      const double a0 = xs[k];
      c0 = fma(a0, xs[k + t0], c0);
      c1 = fma(a0, xs[k + t0 + 1], c1);
      c2 = fma(a0, xs[k + t0 + 2], c2);
      c3 = fma(a0, xs[k + t0 + 3], c3);
    }
    double *p = rp + sg * 4 * G + 4 * g;
    p[0] = c0;
    p[1] = c1;
    p[2] = c2;
    p[3] = c3;
  }
  __syncthreads();
  if (S > 1) {
    for (int i = tid; i < nl; i += VS_AC_A_THREADS) {
      double v = rp[i];
      for (int q = 1; q < S; q++) v += rp[q * 4 * G + i];
      rp[i] = v; /* (only thread i touches column i) */
    }
    __syncthreads();
  }
}

__device__ __forceinline__ double vs_ac_wave_sum(double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

#endif
