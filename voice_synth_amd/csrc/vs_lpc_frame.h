/*
 * vs_lpc_frame.h -- what the kernels that write vs_lpc_frame records share around their own analysis: vs_lpc.hip,
 * vs_iaif.hip and vs_cplpc.hip.  Device code only, next to vs_lpc_roots.h (the root phase).
 *
 * Here: the row of a frame, Levinson-Durbin over the [lag][frame] LDS layout, the store of a workgroup's sets, the
 * frame record, a double out of another lane.  Not here, because they differ for a reason: the autocorrelation and
 * covariance cores (vs_lpc's exact int64 blocks, vs_iaif's look-back FMA chains, vs_cplpc's chunks and corrections) and
 * vs_cplpc's LDL^T solve.
 */
#ifndef VS_LPC_FRAME_H
#define VS_LPC_FRAME_H

#include <hip/hip_runtime.h>

#include "../../include/voice_synth.h"
#include "vs_lpc.h"

/* the row of frame g of the call: the last row whose first frame is <= g */
__device__ __forceinline__ long vs_frame_row(const VsLpcRow *rows, long n_lanes, long g)
{
  long lo = 0, hi = n_lanes - 1;
  while (lo < hi) {
    const long mid = (lo + hi + 1) >> 1;
    if (rows[mid].first <= g) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

/* Levinson-Durbin at order q for frame f, in the header's order of operations (the device equals the host restatement
 * bit for bit): r(t) at Rr[t * FB + f], a_t into Aa[t * FB + f], t = 1..q, updated in place, in pairs (a[j], a[i-j]):
 * the values of a' = a + k*reverse(a).  Returns the status; r0 = r(0), err = the prediction error.  A frame that fails
 * gets NaN taps and a NaN error. */
__device__ __forceinline__ int vs_frame_levinson(const double *Rr, double *Aa, int FB, int f, int q, double &r0,
                                                 double &err)
{
  const double r = Rr[f];
  int status = r == 0.0 ? VS_LPC_SILENT : 0;
  double e = r;
  for (int i = 1; i <= q && status == 0; i++) {
    double acc = Rr[i * FB + f];
    for (int j = 1; j < i; j++) acc = acc + Aa[j * FB + f] * Rr[(i - j) * FB + f];
    const double k = -acc / e;
    if (!(fabs(k) < 1.0)) {
      status = VS_LPC_UNSTABLE;
      break;
    }
    for (int j = 1; 2 * j <= i && j < i; j++) {
      const double aj = Aa[j * FB + f], aij = Aa[(i - j) * FB + f];
      if (2 * j == i) {
        Aa[j * FB + f] = aj + k * aj;
      } else {
        Aa[j * FB + f] = aj + k * aij;
        Aa[(i - j) * FB + f] = aij + k * aj;
      }
    }
    Aa[i * FB + f] = k;
    e = e * (1.0 - k * k);
    if (!(e > 0.0)) status = VS_LPC_UNSTABLE;
  }
  if (status != 0) {
    const double nan = __builtin_nan("");
    for (int t = 1; t <= q; t++) Aa[t * FB + f] = nan;
    e = nan;
  }
  r0 = r;
  err = e;
  return status;
}

/* the sets (1, a_1 .. a_q) of the workgroup's nf frames into sets[f_out[f]][0..q].  Consecutive frames of a row are
 * consecutive records: the stores of a wave are contiguous */
__device__ __forceinline__ void vs_frame_store_sets(double *sets, const double *Aa, int FB, int q, int nf,
                                                    const long *f_out, int tid, int threads)
{
  const int nc = q + 1;
  for (int idx = tid; idx < nf * nc; idx += threads) {
    const int f = idx / nc, t = idx - f * nc;
    sets[f_out[f] * nc + t] = t == 0 ? 1.0 : Aa[t * FB + f];
  }
}

/* the record of a frame.  By reference: what lies in LDS is read where it is stored, as the kernels did it themselves */
__device__ __forceinline__ void vs_frame_record(vs_lpc_frame *o, const double &r0, const double &err, const int &start,
                                                const int &n_formants, const int &status)
{
  o->r0 = r0;
  o->err = err;
  o->start = start;
  o->n_formants = n_formants;
  o->status = status;
  o->reserved_ = 0;
}

/* lane l's v for every lane (l uniform) */
__device__ __forceinline__ double vs_readlane_f64(double v, int l)
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

#endif
