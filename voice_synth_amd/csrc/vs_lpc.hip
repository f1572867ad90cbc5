/*
 * vs_lpc.hip -- gfx950 kernel of the LPC analysis (include/voice_synth.h, "LPC analysis"): A(z), the prediction error
 * and the formants of every frame of int16 rows, already on the device.
 *
 * ONE fused kernel, 256 threads per workgroup, FB = min(64, 256 / G) consecutive frames of the call per workgroup
 * (frames of all rows numbered in a row; G = groups of four lags, 6 at order 22, so FB = 42):
 *
 *   1. Autocorrelation.  Thread (frame f = tid % FB, lag group g = tid / FB) owns lags 4g..4g+3 of frame f.  The frames'
 *      windowed samples v[n] = w[n] * d[s+n] go through LDS as doubles in chunks of VS_LPC_CHUNK (each frame's row of an
 *      odd number of doubles: the 32 lanes of a b64 read hit distinct banks); each thread walks its chunk with a window
 *      of seven values in registers, sixteen fp64 FMAs for eight LDS reads.  |v| < 2^24, so a block of 32 products per
 *      accumulator is an exact fp64 integer below 2^53; the blocks are added in int64.  The sum is exact, in any order.
 *   2. Levinson-Durbin (vs_lpc_frame.h, shared with vs_iaif.hip), one lane per frame (wave 0), r and a in LDS
 *      ([lag][frame]: the lanes read consecutive doubles), in the header's order: the device equals the host
 *      restatement bit for bit.
 *   3. Roots (opts.n_formants > 0; vs_lpc_roots.h, shared with vs_iaif.hip and vs_cplpc.hip), one lane per root: P2 = the power of two
 *      >= order lanes per frame, 256 / P2 frames at a time.  Aberth-Ehrlich from fixed points on a circle of radius 0.9 (every root lies inside the unit circle);
 *      the other roots of the frame come through __shfl, the coefficients from LDS (one address per frame: broadcast);
 *      the sum over the other roots uses v_rcp_f64 (near a root N*S is small: the step is N/(1 - N*S) ~ N).
 *      A frame is done when all its corrections |w| <= 1e-12 (the wave iterates until all its frames are, at most
 *      VS_LPC_MAX_ITER times), then one Newton step per root.  Formants are ranked by f through __shfl.
 *
 * Fused rather than two kernels: the coefficients are in LDS when the roots need them; a second kernel would read them
 * from a buffer of 8*(order+1) bytes per frame (1.2 GB for config 3's 6.4 M frames) that the caller may not want.
 * Per-frame status goes into the record; there is no device trap.  The row of a frame, the store of the sets and the
 * record are vs_lpc_frame.h's, shared with vs_iaif.hip and vs_cplpc.hip.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_lpc.h"
#include "vs_lpc_frame.h"
#include "vs_lpc_roots.h"

__global__ __launch_bounds__(VS_LPC_THREADS) void vs_lpc_kernel(VsLpcArgs a)
{
  extern __shared__ double lpc_lds[];
  __shared__ long f_base[64], f_out[64]; /* row*pitch + s; row*frames_pitch + j */
  __shared__ int f_L[64], f_woff[64], f_start[64], f_fs[64], f_status[64], f_nf[64];
  __shared__ double f_r0[64], f_err[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = a.order, G = vs_lpc_groups(p), FB = vs_lpc_fb(p), SD = vs_lpc_stride(p);
  const long g0 = (long)blockIdx.x * FB;
  const int nf = (int)min((long)FB, a.total_frames - g0);

  if (tid < nf) {
    const long g = g0 + tid, lo = vs_frame_row(a.rows, a.n_lanes, g);
    const VsLpcRow R = a.rows[lo];
    const int j = (int)(g - R.first);
    const int s = R.s0 + j * R.H;
    f_base[tid] = lo * a.pitch + s;
    f_out[tid] = lo * a.frames_pitch + j;
    f_L[tid] = R.L;
    f_woff[tid] = R.woff;
    f_start[tid] = s;
    f_fs[tid] = R.fs;
  }
  __syncthreads();
  int Lmax = 0;
  for (int f = 0; f < nf; f++) Lmax = max(Lmax, f_L[f]);

  /* 1. autocorrelation */
  const int fi = tid % FB, gi = tid / FB, t0 = 4 * gi;
  const bool mine = gi < G && fi < nf;
  const int W = VS_LPC_CHUNK + 4 * G - 1; /* values of a chunk row: lags reach 4G - 1 past the chunk */
  long long s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  for (int n0 = 0; n0 < Lmax; n0 += VS_LPC_CHUNK) {
    __syncthreads();
    for (int f = wave; f < nf; f += VS_LPC_THREADS / 64) {
      const int L = f_L[f];
      const int16_t *x = a.pcm + f_base[f];
      const int32_t *w = a.windows + f_woff[f];
      double *row = lpc_lds + f * SD;
      for (int c = lane; c < W; c += 64) {
        const int n = n0 + c;
        double v = 0.0;
        if (n < L) {
          int d = x[n];
          if (a.pre) d -= x[n - 1];   /* s >= 1 with pre-emphasis */
          v = (double)(w[n] * d);     /* |v| <= 256 * 65535 < 2^24 */
        }
        row[c] = v;
      }
    }
    __syncthreads();
    if (mine) {
      const double *xs = lpc_lds + fi * SD, *v = xs + t0;
#pragma unroll
      for (int kb = 0; kb < VS_LPC_CHUNK; kb += 32) {
        double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
        double v4 = v[kb], v5 = v[kb + 1], v6 = v[kb + 2];
#pragma unroll 2
        for (int k = kb; k < kb + 32; k += 4) {
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
        s0 += (long long)c0; /* 32 products: an exact integer below 2^53 */
        s1 += (long long)c1;
        s2 += (long long)c2;
        s3 += (long long)c3;
      }
    }
  }
  __syncthreads();
  double *Rr = lpc_lds;                /* r(t) of frame f at Rr[t * FB + f] */
  double *Aa = lpc_lds + (p + 1) * FB; /* a_t at Aa[t * FB + f], t = 1..p */
  if (mine) {
    if (t0 <= p) Rr[t0 * FB + fi] = (double)s0;
    if (t0 + 1 <= p) Rr[(t0 + 1) * FB + fi] = (double)s1;
    if (t0 + 2 <= p) Rr[(t0 + 2) * FB + fi] = (double)s2;
    if (t0 + 3 <= p) Rr[(t0 + 3) * FB + fi] = (double)s3;
  }
  __syncthreads();

  /* 2. Levinson-Durbin */
  if (tid < nf) {
    f_status[tid] = vs_frame_levinson(Rr, Aa, FB, tid, p, f_r0[tid], f_err[tid]);
    f_nf[tid] = 0;
  }
  __syncthreads();

  if (a.coefs) vs_frame_store_sets(a.coefs, Aa, FB, p, nf, f_out, tid, VS_LPC_THREADS);

  /* 3. roots and formants */
  if (a.n_formants > 0)
    vs_lpc_roots(Aa, FB, p, nf, a.n_formants, a.f_lo, a.formants, f_out, f_fs, f_status, f_nf, tid, VS_LPC_THREADS);
  __syncthreads();

  if (tid < nf)
    vs_frame_record(a.frames + f_out[tid], f_r0[tid], f_err[tid], f_start[tid], f_nf[tid], f_status[tid]);
}

extern "C" hipError_t vs_launch_lpc(const VsLpcArgs *args, hipStream_t stream)
{
  if (args->total_frames <= 0) return hipSuccess;
  if (args->order < 1 || args->order > VS_MAX_ORDER) return hipErrorInvalidValue;
  const long fb = vs_lpc_fb(args->order);
  const long blocks = (args->total_frames + fb - 1) / fb;
  if (blocks > 0x7FFFFFFFL) return hipErrorInvalidValue;
  const size_t lds = (size_t)vs_lpc_lds_doubles(args->order) * sizeof(double);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)vs_lpc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(vs_lpc_kernel, dim3((unsigned)blocks), dim3(VS_LPC_THREADS), lds, stream, *args);
  return hipGetLastError();
}
