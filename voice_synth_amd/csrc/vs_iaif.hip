/*
 * vs_iaif.hip -- gfx950 kernel of the IAIF analysis (include/voice_synth.h, "IAIF"): per frame of int16 rows, already on
 * the device, the vocal-tract set V2 that four rounds of linear prediction leave once the glottal contribution c2 has been
 * taken out of the speech, with r0, err and the formants of V2.
 *
 * ONE fused kernel in the shape of vs_lpc_kernel: 256 threads per workgroup, FB = vs_lpc_fb(p) consecutive frames of the
 * call per workgroup, the same frame -> row records.  The four stages run one after the other over the frame, each in
 * chunks of VS_LPC_CHUNK samples m0 .. m0 + 63 through LDS:
 *
 *   a. E: the int16 input of every frame, the stage's n taps of history before the chunk and the chunk, zeros where the
 *      header has zeros (before -M, before the row, behind the window); a wave per frame, a lane per sample.
 *   b. FIR: a wave per frame, a lane per sample: acc = e[m]; acc = fma(c_j, e[m-j], acc), j ascending.  Lane j holds tap
 *      c_(j+1) of the frame; the loop takes it with v_readlane, so a tap costs one LDS read (the int16 sample), one
 *      conversion and one fp64 FMA.  The windowed value v = w[m] * y goes into the frame's V row behind the H = 4G - 1
 *      values the previous chunk ended with (they move there through registers: read while the autocorrelation reads,
 *      written behind the barrier).
 *   c. Stage 3 only: INT, the one recurrence, one lane per frame, one FMA per sample, its state in a register from chunk
 *      to chunk; it starts one chunk early (m0 = -64: the FIR of samples -M .. -1 feeds it, zeros before).
 *   d. Autocorrelation: thread (frame, lag group) as in vs_lpc with the register window of seven values, looking BACK
 *      from the chunk: lag k pairs v[m-k] with v[m] for m ascending, which are the header's products in the header's
 *      order (a zero product leaves the chain as it is).  One fp64 FMA chain per (frame, lag): no int64 blocks.
 *
 * Between the stages Levinson-Durbin runs as in vs_lpc (one lane per frame, r and a over the V rows), and the new taps go
 * into T.  A frame whose stage fails keeps its status, r0 of that stage and NaN taps; the later stages run on it with
 * NaN taps and their results are dropped.  The root phase is vs_lpc's (vs_lpc_roots.h); the recursion, the store of
 * the sets, the record and the lane read are vs_lpc_frame.h's, shared with vs_lpc.hip and vs_cplpc.hip.  No device trap.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_iaif.h"
#include "vs_lpc_frame.h"
#include "vs_lpc_roots.h"

__global__ __launch_bounds__(VS_LPC_THREADS) void vs_iaif_kernel(VsIaifArgs ia)
{
  extern __shared__ double iaif_lds[];
  __shared__ long f_base[64], f_out[64]; /* row*pitch + s; row*frames_pitch + j */
  __shared__ int f_L[64], f_woff[64], f_start[64], f_fs[64], f_status[64], f_nf[64], f_low[64];
  __shared__ double f_r0[64], f_err[64];
  const VsLpcArgs &a = ia.lpc;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = a.order, g = ia.glottal_order, G = vs_lpc_groups(p), FB = vs_lpc_fb(p), SD = vs_lpc_stride(p);
  const int H = 4 * G - 1, SE = vs_iaif_estride(p), TP = vs_iaif_tstride(p);
  const double rho = ia.leak, nan = __builtin_nan("");
  double *V = iaif_lds;                                                 /* [FB][SD] */
  int16_t *E = (int16_t *)(iaif_lds + vs_lpc_lds_doubles(p));           /* [FB][SE] */
  double *T = iaif_lds + vs_lpc_lds_doubles(p) + vs_iaif_e_doubles(p);  /* [FB][TP] */
  double *Rr = iaif_lds;                /* r(t) of frame f at Rr[t * FB + f] */
  double *Aa = iaif_lds + (p + 1) * FB; /* a_t at Aa[t * FB + f], t = 1..p */
  const long g0 = (long)blockIdx.x * FB;
  const int nf = (int)min((long)FB, a.total_frames - g0);

  if (tid < nf) { /* the frame's row: the last row whose first frame is <= g.  vs_frame_row's search, written out: through
                     the function the compiler schedules the LDS reads of the autocorrelation loop (d.) differently, and
                     the launch takes 0.8 % longer (profiles/frame_scaffold_refactor.txt) */
    const long gf = g0 + tid;
    long lo = 0, hi = a.n_lanes - 1;
    while (lo < hi) {
      const long mid = (lo + hi + 1) >> 1;
      if (a.rows[mid].first <= gf) lo = mid;
      else hi = mid - 1;
    }
    const VsLpcRow R = a.rows[lo];
    const int j = (int)(gf - R.first);
    const int s = R.s0 + j * R.H;
    f_base[tid] = lo * a.pitch + s;
    f_out[tid] = lo * a.frames_pitch + j;
    f_L[tid] = R.L;
    f_woff[tid] = R.woff;
    f_start[tid] = s;
    f_fs[tid] = R.fs;
    f_low[tid] = -min(s, p + 1); /* e[n] = 0 for n < -M and before the row */
    f_status[tid] = 0;
    f_nf[tid] = 0;
    f_r0[tid] = 0.0;
    f_err[tid] = nan;
  }
  __syncthreads();
  int Lmax = 0;
  for (int f = 0; f < nf; f++) Lmax = max(Lmax, f_L[f]);

  const int fi = tid % FB, gi = tid / FB, t0 = 4 * gi;
  /* the values a chunk hands to the next: item tid + 256 r is value ti of frame tf's H */
  int toff[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int idx = tid + VS_LPC_THREADS * r;
    const int tf = idx / H;
    toff[r] = idx < nf * H ? tf * SD + (idx - tf * H) : -1;
  }

#pragma unroll 1
  for (int stage = 1; stage <= 4; stage++) {
    const int ntap = stage == 1 ? 0 : stage == 2 ? 1 : stage == 3 ? p : g; /* taps of the stage's FIR */
    const int q = stage == 1 ? 1 : stage == 3 ? g : p;                     /* order of its predictor */
    const bool mine = fi < nf && gi < G && t0 <= q;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0, integ = 0.0;
    double tl[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m0 = stage == 3 ? -VS_LPC_CHUNK : 0; m0 < Lmax; m0 += VS_LPC_CHUNK) {
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; r++)
        if (toff[r] >= 0) V[toff[r]] = tl[r];
      for (int f = wave; f < nf; f += VS_LPC_THREADS / 64) { /* a. */
        const int16_t *x = a.pcm + f_base[f];
        const int low = f_low[f], L = f_L[f];
        for (int i = lane; i < VS_LPC_CHUNK + ntap; i += 64) {
          const int n = m0 - ntap + i;
          E[f * SE + i] = n >= low && n < L ? x[n] : (int16_t)0;
        }
      }
      __syncthreads();
      for (int f = wave; f < nf; f += VS_LPC_THREADS / 64) { /* b. */
        const double tap = lane < ntap ? T[f * TP + lane] : 0.0;
        const int16_t *er = E + f * SE + ntap + lane;
        double acc = (double)er[0];
        for (int j = 1; j <= ntap; j++) acc = fma(vs_readlane_f64(tap, j - 1), (double)er[-j], acc);
        const int m = m0 + lane;
        if (stage != 3) acc = m >= 0 && m < f_L[f] ? (double)a.windows[f_woff[f] + m] * acc : 0.0;
        V[f * SD + H + lane] = acc;
      }
      __syncthreads();
      if (stage == 3) { /* c. */
        if (tid < nf) {
          double *row = V + tid * SD + H;
          const int32_t *w = a.windows + f_woff[tid];
          const int L = f_L[tid];
          for (int c = 0; c < VS_LPC_CHUNK; c++) {
            const int m = m0 + c;
            integ = fma(rho, integ, row[c]);
            row[c] = m >= 0 && m < L ? (double)w[m] * integ : 0.0;
          }
        }
        __syncthreads();
      }
#pragma unroll
      for (int r = 0; r < 4; r++)
        if (toff[r] >= 0) tl[r] = V[toff[r] + VS_LPC_CHUNK];
      if (mine && m0 >= 0) { /* d. */
        const double *xs = V + fi * SD + H, *u = xs - t0 - 3;
        double w4 = u[0], w5 = u[1], w6 = u[2];
#pragma unroll 2
        for (int k = 0; k < VS_LPC_CHUNK; k += 4) {
          const double w0 = w4, w1 = w5, w2 = w6, w3 = u[k + 3];
          w4 = u[k + 4];
          w5 = u[k + 5];
          w6 = u[k + 6];
          const double a0 = xs[k], a1 = xs[k + 1], a2 = xs[k + 2], a3 = xs[k + 3];
          c0 = fma(w3, a0, c0); c1 = fma(w2, a0, c1); c2 = fma(w1, a0, c2); c3 = fma(w0, a0, c3);
          c0 = fma(w4, a1, c0); c1 = fma(w3, a1, c1); c2 = fma(w2, a1, c2); c3 = fma(w1, a1, c3);
          c0 = fma(w5, a2, c0); c1 = fma(w4, a2, c1); c2 = fma(w3, a2, c2); c3 = fma(w2, a2, c3);
          c0 = fma(w6, a3, c0); c1 = fma(w5, a3, c1); c2 = fma(w4, a3, c2); c3 = fma(w3, a3, c3);
        }
      }
    }
    __syncthreads();
    if (mine) {
      Rr[t0 * FB + fi] = c0;
      if (t0 + 1 <= q) Rr[(t0 + 1) * FB + fi] = c1;
      if (t0 + 2 <= q) Rr[(t0 + 2) * FB + fi] = c2;
      if (t0 + 3 <= q) Rr[(t0 + 3) * FB + fi] = c3;
    }
    __syncthreads();

    /* Levinson-Durbin at order q; a frame that failed an earlier stage keeps what that stage left, and NaN taps */
    if (tid < nf) {
      if (f_status[tid] == 0) f_status[tid] = vs_frame_levinson(Rr, Aa, FB, tid, q, f_r0[tid], f_err[tid]);
      else
        for (int t = 1; t <= q; t++) Aa[t * FB + tid] = nan;
    }
    __syncthreads();

    if (stage < 4) { /* the next stage's taps */
      for (int f = wave; f < nf; f += VS_LPC_THREADS / 64)
        if (lane < q) T[f * TP + lane] = Aa[(lane + 1) * FB + f];
      if (stage == 3 && ia.glottal) vs_frame_store_sets(ia.glottal, Aa, FB, g, nf, f_out, tid, VS_LPC_THREADS);
    }
  }

  /* what only the end needs is read from the kernel's argument block here, not held in SGPRs through the stages */
  const VsLpcArgs &z = ((const VsIaifArgs *)__builtin_amdgcn_kernarg_segment_ptr())->lpc;
  if (z.coefs) vs_frame_store_sets(z.coefs, Aa, FB, p, nf, f_out, tid, VS_LPC_THREADS);
  if (z.n_formants > 0)
    vs_lpc_roots(Aa, FB, p, nf, z.n_formants, z.f_lo, z.formants, f_out, f_fs, f_status, f_nf, tid, VS_LPC_THREADS);
  __syncthreads();

  if (tid < nf)
    vs_frame_record(z.frames + f_out[tid], f_r0[tid], f_err[tid], f_start[tid], f_nf[tid], f_status[tid]);
}

extern "C" hipError_t vs_launch_iaif(const VsIaifArgs *args, hipStream_t stream)
{
  const int p = args->lpc.order;
  if (args->lpc.total_frames <= 0) return hipSuccess;
  if (p < 1 || p > VS_MAX_ORDER || args->glottal_order < 1 || args->glottal_order > p) return hipErrorInvalidValue;
  const long fb = vs_lpc_fb(p);
  const long blocks = (args->lpc.total_frames + fb - 1) / fb;
  if (blocks > 0x7FFFFFFFL) return hipErrorInvalidValue;
  const size_t lds = (size_t)vs_iaif_lds_doubles(p) * sizeof(double);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)vs_iaif_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(vs_iaif_kernel, dim3((unsigned)blocks), dim3(VS_LPC_THREADS), lds, stream, *args);
  return hipGetLastError();
}
