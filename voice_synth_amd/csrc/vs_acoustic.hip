/*
 * vs_acoustic.hip -- gfx950 kernels of the acoustic measurement (include/voice_synth.h, "acoustic measurement"):
 * F0, jitter, shimmer and HNR of int16 rows, already on the device.
 *
 * Two kernels on the context's stream, one behind the other:
 *
 *   vs_ac_period_kernel (stage A): ONE WORKGROUP (256 threads) PER ROW.  The row's 3*tmax + 2-sample window goes into
 *       LDS as doubles; the lags tmin-1..tmax+1 go through the correlation core of vs_ac_corr.h (shared with the pitch
 *       track's candidate kernel): exact fp64 sums, whose order does not matter.  P0 and rmax come out of wave
 *       reductions; r(0) and e out of a block reduction.
 *
 *   vs_ac_marks_kernel (stage B/C): ONE LANE PER ROW, 64 rows per workgroup (one wavefront), like the synthesis kernels.
 *       [64 rows x VS_AC_TILE] int16 tiles stream through LDS (each load instruction covers 256 contiguous bytes of one
 *       row; the next tile is in registers while this one is walked); each lane walks its own row forward with O(1)
 *       state (window, running argmax, running minimum, the last four periods and amplitudes, int64 sums) and writes
 *       its marks as it goes.  A window that begins at or before the sample just walked (periods that jump by a quarter
 *       or more) is resolved by walking the already-streamed stretch again from the row in HBM: the same step, so the
 *       result is that of the one forward pass the header defines.
 *
 * Per-row status goes into the record; there is no device trap and nothing stops a wavefront but its own row.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_ac_corr.h"
#include "vs_acoustic.h"

#ifndef VS_AC_TILE
#define VS_AC_TILE 128  /* samples per row per tile of the marks kernel */
#endif
#define VS_AC_PAD 2      /* LDS row stride VS_AC_TILE + 2 int16 = an odd number of dwords: the lanes' reads hit 64 banks */

/* ---------------------------------------------------------------------------------------------------------------- */
/* stage A                                                                                                           */

__device__ __forceinline__ double ac_wave_max(double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int ac_wave_min_int(int v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ void ac_record_empty(vs_acoustic *o, int status)
{
  const double nan = __builtin_nan("");
  o->f0_hz = nan;
  o->jitter_local = nan;
  o->jitter_abs_s = nan;
  o->jitter_rap = nan;
  o->jitter_ppq5 = nan;
  o->shimmer_local = nan;
  o->shimmer_db = nan;
  o->shimmer_apq3 = nan;
  o->shimmer_apq5 = nan;
  o->hnr_db = nan;
  o->p0 = 0;
  o->n_periods = 0;
  o->first_mark = -1;
  o->status = status;
}

__global__ __launch_bounds__(VS_AC_A_THREADS) void vs_ac_period_kernel(VsAcArgs a)
{
  extern __shared__ double ac_lds[];
  const long row = blockIdx.x;
  const VsAcRow R = a.rows[row];
  const int tid = threadIdx.x;
  vs_acoustic *o = a.out + row;
  if (R.len < 3 * R.tmax + 2) {
    if (tid == 0) ac_record_empty(o, VS_AC_TOO_SHORT);
    return;
  }
  const int W = 2 * R.tmax;
  const int s = (R.len - W - R.tmax - 1) / 2;
  const int nwin = W + R.tmax + 1;            /* samples s .. s + W + tmax */
  const int tlo = R.tmin - 1, nl = R.tmax + 3 - R.tmin; /* lags tlo .. tmax + 1 */
  double *xs = ac_lds;                        /* [nwin + pad]: lags of the last group reach 3 past tmax + 1 */
  double *rp = ac_lds + vs_ac_xs_doubles(R.tmax);   /* [S][4G] partial sums, then r(t) in rp[t - tlo] */
  double *red = rp + vs_ac_rp_doubles(R.tmin, R.tmax); /* [2][4] block reduction */

  const int16_t *x = a.pcm + row * a.pitch + s;
  for (int i = tid; i < nwin; i += VS_AC_A_THREADS) xs[i] = (double)(a.polarity * (int)x[i]);
  for (int i = nwin + tid; i < vs_ac_xs_doubles(R.tmax); i += VS_AC_A_THREADS) xs[i] = 0.0;
  __syncthreads();

  vs_ac_lag_sums(xs, rp, tlo, nl, W, tid);

  /* rmax and P0 in the first wavefront: r(t) = rp[t - tlo], t in [tmin, tmax] = indices 1 .. nl - 2 */
  const int lane = tid & 63, wave = tid >> 6;
  __shared__ int ac_p0;
  if (wave == 0) {
    double m = -1.0e300;
    for (int i = 1 + lane; i <= nl - 2; i += 64) m = fmax(m, rp[i]);
    const double rmax = ac_wave_max(m);
    if (rmax <= 0.0) {
      if (lane == 0) ac_p0 = 0;
    } else {
      int best = 0x7FFFFFFF, first = 0x7FFFFFFF;
      for (int i = 1 + lane; i <= nl - 2; i += 64) {
        const double r = rp[i];
        if (r > rp[i - 1] && r >= rp[i + 1] && 10.0 * r >= 9.0 * rmax) best = min(best, i);  /* exact: below 2^47 */
        if (r == rmax) first = min(first, i);
      }
      best = ac_wave_min_int(best);
      first = ac_wave_min_int(first);
      if (lane == 0) ac_p0 = tlo + (best != 0x7FFFFFFF ? best : first);
    }
  }
  __syncthreads();
  const int p0 = ac_p0;
  if (p0 == 0) {
    if (tid == 0) ac_record_empty(o, VS_AC_UNVOICED);
    return;
  }
  double r0 = 0.0, e = 0.0;
  for (int k = tid; k < W; k += VS_AC_A_THREADS) {
    r0 = fma(xs[k], xs[k], r0);
    e = fma(xs[k + p0], xs[k + p0], e);
  }
  r0 = vs_ac_wave_sum(r0);
  e = vs_ac_wave_sum(e);
  if (lane == 0) {
    red[wave] = r0;
    red[4 + wave] = e;
  }
  __syncthreads();
  if (tid == 0) {
    r0 = (red[0] + red[1]) + (red[2] + red[3]);
    e = (red[4] + red[5]) + (red[6] + red[7]);
    double rho = rp[p0 - tlo] / sqrt(r0 * e);
    rho = fmin(fmax(rho, 1e-10), 1.0 - 1e-10);
    ac_record_empty(o, 0);
    o->p0 = p0;
    o->hnr_db = 10.0 * log10(rho / (1.0 - rho));
  }
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* stage B/C                                                                                                         */

struct AcWalk {
  int m;          /* last mark (-1: looking for m_0) */
  int wlo, whi;   /* window of the next mark */
  int best, bpos; /* running argmax over the window (first index on ties) */
  int amin;       /* min y over [m, bpos) */
  int msince;     /* min y over [bpos, current sample] */
  int runmin;     /* min y over [m, current sample) */
  int lo1, hi1, d;
  int done;
  int m0;         /* first mark */
  int K, nm;      /* periods, marks written */
  int T1, T2, T3, T4, A1, A2, A3, A4; /* the last four periods and amplitudes (1 = latest) */
  long long sT, sdT, s3T, s5T, sA, sdA, s3A, s5A;
  double sdb;
  int zero_amp;
};

__device__ __forceinline__ int ac_abs(int v) { return v < 0 ? -v : v; }

/* one sample j (value v) of the walk; true when the next window begins at or before j (walk again from the new mark) */
__device__ __forceinline__ bool ac_step(AcWalk &w, const VsAcArgs &a, const VsAcRow &R, long row, int j, int v)
{
  if (j >= w.wlo) {
    if (v > w.best) {
      w.best = v;
      w.bpos = j;
      w.amin = w.runmin;
      w.msince = v;
    } else {
      w.msince = min(w.msince, v);
    }
  }
  w.runmin = min(w.runmin, v);
  if (j != w.whi) return false;
  const int mn = w.bpos;
  int lo, hi;
  if (w.m < 0) {
    w.m0 = mn;
    lo = w.lo1;
    hi = w.hi1;
  } else {
    const int T = mn - w.m, A = w.best - w.amin;
    w.K++;
    w.sT += T;
    w.sA += A;
    if (A <= 0) w.zero_amp = 1;
    if (w.K >= 2) {
      w.sdT += ac_abs(T - w.T1);
      w.sdA += ac_abs(A - w.A1);
      if (A > 0 && w.A1 > 0) w.sdb += fabs(20.0 * log10((double)A / (double)w.A1));
    }
    if (w.K >= 3) {
      w.s3T += ac_abs(3 * w.T1 - (w.T2 + w.T1 + T));
      w.s3A += ac_abs(3 * w.A1 - (w.A2 + w.A1 + A));
    }
    if (w.K >= 5) {
      w.s5T += ac_abs(5 * w.T2 - (w.T4 + w.T3 + w.T2 + w.T1 + T));
      w.s5A += ac_abs(5 * w.A2 - (w.A4 + w.A3 + w.A2 + w.A1 + A));
    }
    w.T4 = w.T3; w.T3 = w.T2; w.T2 = w.T1; w.T1 = T;
    w.A4 = w.A3; w.A3 = w.A2; w.A2 = w.A1; w.A1 = A;
    lo = max(w.lo1, T - w.d);
    hi = min(w.hi1, T + w.d);
  }
  if (a.marks && w.nm < a.marks_pitch) a.marks[row * a.marks_pitch + w.nm] = mn;
  w.nm++;
  w.m = mn;
  w.wlo = mn + lo;
  w.whi = mn + hi;
  w.best = -0x7FFFFFFF - 1;
  if (w.whi >= R.len) {
    w.done = 1;
    return false;
  }
  if (w.wlo <= j) {
    w.runmin = 0x7FFFFFFF;
    return true;
  }
  w.runmin = w.msince;
  return false;
}

__global__ __launch_bounds__(64) void vs_ac_marks_kernel(VsAcArgs a)
{
  __shared__ uint32_t tile[64 * (VS_AC_TILE + VS_AC_PAD) / 2];
  const int lane = threadIdx.x;
  const long row0 = (long)blockIdx.x * 64, row = row0 + lane;
  const bool live = row < a.n_lanes;
  VsAcRow R = {0, 1, 2, 3};
  int p0 = 0, status = VS_AC_TOO_SHORT;
  if (live) {
    R = a.rows[row];
    p0 = a.out[row].p0;
    status = a.out[row].status;
  }
  AcWalk w = {};
  w.m = -1;
  w.wlo = 0;
  w.whi = R.tmax - 1;
  w.best = -0x7FFFFFFF - 1;
  w.runmin = 0x7FFFFFFF;
  w.lo1 = max(R.tmin, (2 * p0 + 2) / 3);
  w.hi1 = min(R.tmax, (3 * p0) / 2);
  w.d = (p0 + 3) / 4;
  w.done = (status != 0);
  int need = w.done ? 0 : R.len;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) need = max(need, __shfl_xor(need, o, 64));

  const int rows_here = (int)min((long)64, a.n_lanes - row0);
  const int16_t *base = a.pcm + row0 * a.pitch;
  const int16_t *mine = a.pcm + row * a.pitch;
  int pf[VS_AC_TILE / 64][64]; /* the next tile: [column block][row of the workgroup] */
  auto fetch = [&](int t0) {
#pragma unroll
    for (int cb = 0; cb < VS_AC_TILE / 64; cb++) {
      const long col = (long)t0 + cb * 64 + lane;
#pragma unroll
      for (int r = 0; r < 64; r++)
        pf[cb][r] = (r < rows_here && col < (long)a.n_samples) ? (int)base[r * a.pitch + col] : 0;
    }
  };
  if (need > 0) fetch(0);
  for (int t0 = 0; t0 < need; t0 += VS_AC_TILE) {
    __syncthreads();
    uint16_t *t16 = (uint16_t *)tile;
#pragma unroll
    for (int cb = 0; cb < VS_AC_TILE / 64; cb++)
#pragma unroll
      for (int r = 0; r < 64; r++) t16[r * (VS_AC_TILE + VS_AC_PAD) + cb * 64 + lane] = (uint16_t)pf[cb][r];
    __syncthreads();
    if (t0 + VS_AC_TILE < need) fetch(t0 + VS_AC_TILE);
    if (w.done) continue;
    const uint32_t *my = tile + lane * ((VS_AC_TILE + VS_AC_PAD) / 2);
    const int cend = min(VS_AC_TILE, R.len - t0);
    for (int c = 0; c < cend && !w.done; c += 2) {
      const uint32_t pair = my[c / 2];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int j = t0 + c + h;
        if (w.done || j >= R.len) break;
        const int v = a.polarity * (int)(int16_t)(h ? (pair >> 16) : (pair & 0xFFFFu));
        if (ac_step(w, a, R, row, j, v)) {
          int q = w.m; /* walk [m, j] again from HBM */
          while (q <= j && !w.done) q = ac_step(w, a, R, row, q, a.polarity * (int)mine[q]) ? w.m : q + 1;
        }
      }
    }
  }
  if (!live || status != 0) return;

  vs_acoustic *o = a.out + row;
  const double nan = __builtin_nan("");
  const int K = w.K;
  double f0 = nan, jl = nan, jabs = nan, rap = nan, ppq = nan, sl = nan, sdb = nan, apq3 = nan, apq5 = nan;
  if (K >= 1) {
    const double Tm = (double)w.sT / (double)K;
    f0 = (double)R.fs / Tm;
    if (K >= 2) {
      jl = ((double)w.sdT / (double)(K - 1)) / Tm;
      jabs = ((double)w.sdT / (double)(K - 1)) / (double)R.fs;
    }
    if (K >= 3) rap = ((double)w.s3T / (3.0 * (double)(K - 2))) / Tm;
    if (K >= 5) ppq = ((double)w.s5T / (5.0 * (double)(K - 4))) / Tm;
    if (!w.zero_amp) {
      const double Am = (double)w.sA / (double)K;
      if (K >= 2) {
        sl = ((double)w.sdA / (double)(K - 1)) / Am;
        sdb = w.sdb / (double)(K - 1);
      }
      if (K >= 3) apq3 = ((double)w.s3A / (3.0 * (double)(K - 2))) / Am;
      if (K >= 5) apq5 = ((double)w.s5A / (5.0 * (double)(K - 4))) / Am;
    }
  }
  o->f0_hz = f0;
  o->jitter_local = jl;
  o->jitter_abs_s = jabs;
  o->jitter_rap = rap;
  o->jitter_ppq5 = ppq;
  o->shimmer_local = sl;
  o->shimmer_db = sdb;
  o->shimmer_apq3 = apq3;
  o->shimmer_apq5 = apq5;
  o->n_periods = K;
  o->first_mark = w.nm > 0 ? w.m0 : -1;
  o->status = (K < 2 ? VS_AC_FEW_PERIODS : 0) | (K >= 1 && w.zero_amp ? VS_AC_ZERO_AMPLITUDE : 0);
}

extern "C" hipError_t vs_launch_measure(const VsAcArgs *args, int lds_doubles, hipStream_t stream)
{
  if (args->n_lanes <= 0 || args->n_lanes > 0x7FFFFFFFL) return hipErrorInvalidValue;
  const size_t lds = (size_t)lds_doubles * sizeof(double);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)vs_ac_period_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(vs_ac_period_kernel, dim3((unsigned)args->n_lanes), dim3(VS_AC_A_THREADS), lds, stream, *args);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vs_ac_marks_kernel, dim3((unsigned)((args->n_lanes + 63) / 64)), dim3(64), 0, stream, *args);
  return hipGetLastError();
}
