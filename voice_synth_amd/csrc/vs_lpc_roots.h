/*
 * vs_lpc_roots.h -- the root phase of the LPC analysis (include/voice_synth.h, "LPC analysis", Formants), shared by the
 * kernels that end in a set A(z) per frame in LDS: vs_lpc.hip, vs_iaif.hip and vs_cplpc.hip.  Device code only.
 *
 * One lane per root: P2 = the power of two >= order lanes per frame, 256 / P2 frames at a time.  Aberth-Ehrlich from
 * fixed points on a circle of radius 0.9 (every root lies inside the unit circle); the other roots of the frame come
 * through __shfl, the coefficients from LDS (one address per frame: broadcast); the sum over the other roots uses
 * v_rcp_f64 (near a root N*S is small: the step is N/(1 - N*S) ~ N).  A frame is done when all its corrections
 * |w| <= 1e-12 (the wave iterates until all its frames are, at most VS_LPC_MAX_ITER times), then one Newton step per
 * root.  Formants are ranked by f through __shfl.
 */
#ifndef VS_LPC_ROOTS_H
#define VS_LPC_ROOTS_H

#include <hip/hip_runtime.h>

#include "../../include/voice_synth.h"

#define VS_LPC_PI 3.14159265358979323846

/* N = P(z) / P'(z), P(z) = z^p + a_1 z^(p-1) + ... + a_p with a_t at A[t * FB] */
__device__ __forceinline__ void lpc_newton(const double *A, int FB, int p, double zr, double zi, double &nr,
                                           double &ni)
{
  double br = 1.0, bi = 0.0, dr = 0.0, di = 0.0;
  for (int t = 1; t <= p; t++) {
    const double ndr = dr * zr - di * zi + br, ndi = dr * zi + di * zr + bi;
    const double nbr = br * zr - bi * zi + A[t * FB], nbi = br * zi + bi * zr;
    dr = ndr;
    di = ndi;
    br = nbr;
    bi = nbi;
  }
  const double den = dr * dr + di * di;
  nr = (br * dr + bi * di) / den;
  ni = (bi * dr - br * di) / den;
}

/* The roots and formants of the nf frames of a workgroup of `threads` threads (a multiple of 64): a_t of frame f at
 * Aa[t * FB + f]; f_out[f]: the frame's record index, f_fs[f] its rate; f_status[f] non-zero: no roots wanted.  Writes
 * the (f, bw) pairs and the NaN slots of formants (NULL: none), f_nf[f], and VS_LPC_NO_ROOTS into f_status[f].  The
 * caller has f_nf[f] = 0 and a barrier behind it, and puts one in front of reading f_nf / f_status again. */
__device__ __forceinline__ void vs_lpc_roots(const double *Aa, int FB, int p, int nf, int nmax, double f_lo,
                                             double *formants, const long *f_out, const int *f_fs, int *f_status,
                                             int *f_nf, int tid, int threads)
{
  const double nan = __builtin_nan("");
  const int lane = tid & 63;
  int P2 = 1;
  while (P2 < p) P2 <<= 1;
  const int per = threads / P2, seg = tid / P2, q = tid % P2, base = lane & ~(P2 - 1);
  const unsigned long long smask = (P2 == 64 ? ~0ull : ((1ull << P2) - 1)) << base;
  for (int fb = 0; fb < nf; fb += per) {
    const int f = fb + seg, fc = min(f, nf - 1);
    const bool live = f < nf && f_status[fc] == 0;
    const bool on = live && q < p;
    const double *A = Aa + fc;
    const double ang = 2.0 * VS_LPC_PI * ((double)q + 0.25) / (double)p;
    double zr = 0.9 * cos(ang), zi = 0.9 * sin(ang);
    bool done = !live;
    for (int it = 0; it < VS_LPC_MAX_ITER && __any(!done); it++) {
      double nr, ni;
      lpc_newton(A, FB, p, zr, zi, nr, ni);
      double sr = 0.0, si = 0.0; /* sum over the other roots of 1 / (z - z_j) */
      for (int j = 0; j < p; j++) {
        const double ozr = __shfl(zr, base + j, 64), ozi = __shfl(zi, base + j, 64);
        if (j != q) { /* an approximate reciprocal: near a root N*S is small, so S need not be exact */
          const double dr = zr - ozr, di = zi - ozi, inv = __builtin_amdgcn_rcp(dr * dr + di * di);
          sr += dr * inv;
          si -= di * inv;
        }
      }
      /* w = N / (1 - N*S) */
      const double ur = 1.0 - (nr * sr - ni * si), ui = -(nr * si + ni * sr), uden = ur * ur + ui * ui;
      const double wr = (nr * ur + ni * ui) / uden, wi = (ni * ur - nr * ui) / uden;
      const bool conv = !on || wr * wr + wi * wi <= 1e-24;
      const bool seg_conv = (__ballot(!conv) & smask) == 0;
      if (!done) {
        zr -= wr;
        zi -= wi;
        if (seg_conv) done = true;
      }
    }
    const bool ok = live && done;
    if (on && ok) { /* one Newton step */
      double nr, ni;
      lpc_newton(A, FB, p, zr, zi, nr, ni);
      zr -= nr;
      zi -= ni;
    }
    double fhz = 0.0, bw = 0.0;
    bool valid = false;
    if (on && ok && zi > 0.0) {
      const double fsd = (double)f_fs[fc];
      fhz = fsd * atan2(zi, zr) / (2.0 * VS_LPC_PI);
      bw = -fsd * (0.5 * log(zr * zr + zi * zi)) / VS_LPC_PI;
      valid = fhz >= f_lo && fhz <= 0.5 * fsd - f_lo;
    }
    int rank = 0;
    for (int j = 0; j < P2; j++) {
      const double of = __shfl(fhz, base + j, 64);
      const int ov = __shfl((int)valid, base + j, 64);
      if (ov && (of < fhz || (of == fhz && j < q))) rank++;
    }
    const int cnt = __popcll(__ballot(valid) & smask), nw = min(cnt, nmax);
    if (f < nf) {
      if (formants) {
        double *out = formants + f_out[f] * 2 * nmax;
        if (valid && rank < nmax) {
          out[2 * rank] = fhz;
          out[2 * rank + 1] = bw;
        }
        for (int sl = nw + q; sl < nmax; sl += P2) {
          out[2 * sl] = nan;
          out[2 * sl + 1] = nan;
        }
      }
      if (q == 0) {
        f_nf[f] = nw;
        if (live && !done) f_status[f] = VS_LPC_NO_ROOTS;
      }
    }
  }
}

#endif
