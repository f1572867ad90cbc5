/*
 * vs_cplpc.hip -- gfx950 kernel of the closed-phase covariance LPC (include/voice_synth.h, "closed-phase covariance
 * LPC"): per frame the covariance of the samples inside the closed-phase spans of the row's cycles, its LDL^T solve, the
 * step-down and the formants.
 *
 * ONE kernel, one wavefront (64 threads) per frame; with window_s == 0 that is one per row.  Several workgroups share a
 * CU (LDS below), which is what hides the latency of the divisions and of the dependent chains of the solve.
 *
 *   1. Spans.  The row's cycle records are read 64 at a time, one per lane, and each lane decides its span [b, e) and
 *      whether it lies in the frame, in 64-bit integers; the frame lies in [0, len), so a span that lies in the frame
 *      reads nothing outside the row, whatever the records hold.  The spans that pass are then taken one by one, in the
 *      order of their slots.
 *   2. Covariance.  Only the first row phi(0,k) is summed over the equations: lane k owns lag k, the samples go through
 *      LDS in chunks of VS_CPLPC_CHUNK equations with the p samples in front of them, counted from the span's first
 *      equation, so a long span is a sequence of chunks like any other and no chunk boundary is a case of its own.  The
 *      rest follows from phi(i+1,k+1) = phi(i,k) + x[b+p-1-i]*x[b+p-1-k] - x[e-1-i]*x[e-1-k]: the p(p+1)/2 corrections
 *      of a span come from its first and last chunk, at most VS_CPLPC_CORR per lane, each summed in LDS where its phi will
 *      stand.  Everything is int64
 *      (32x32 -> 64 multiply-adds), so the sums are exact in any order.  The clamp test of a span of one chunk is made on
 *      the staged chunk before anything is added; longer spans are scanned once before their first chunk.
 *   3. The triangle c_ik, i <= k, as doubles at M[i * S + k] (S odd: a row and a column are both read without a bank
 *      conflict): lane d walks diagonal d, adding the corrections.
 *   4. The solve in the header's order.  Lane i owns row i of L, which overwrites the triangle (l_ik at M[k * S + i]);
 *      lane k keeps d_k and u_k = l_jk * d_k, and the chain of lane i takes u_k from lane k's register (v_readlane).  The
 *      forward substitution runs over the columns, the back substitution is the serial chain the header writes, with a_k
 *      in lane k's register.  The step-down has lane j own tap j.
 *   5. Roots (vs_lpc_roots.h, shared with vs_lpc.hip and vs_iaif.hip) for frames with status 0.
 *
 * LDS: the triangle, (p + 1) * S doubles of dynamic LDS (vs_cplpc_lds_bytes: 4600 bytes at order 22, 14104 at order 40),
 * and VS_CPLPC_LDS_STATIC bytes of static LDS: the chunk, the taps for the root phase, the frame's words.  Per-frame
 * status goes into the record; there is no device trap.  The row of a frame, the record and the lane read are
 * vs_lpc_frame.h's, shared with vs_lpc.hip and vs_iaif.hip.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_cplpc.h"
#include "vs_lpc_frame.h"
#include "vs_lpc_roots.h"

#define VS_CPLPC_CORR 13 /* corrections per lane: ceil(p/2) * (p + 1) <= 64 * 13 up to order 40 */
static_assert(((VS_MAX_ORDER + 1) / 2) * (VS_MAX_ORDER + 1) <= 64 * VS_CPLPC_CORR, "corrections per lane");
static_assert(VS_MAX_ORDER < 64, "one lane per row of L");

__device__ __forceinline__ bool cp_clamped(int v) { return v >= 32767 || v <= -32767; }

__global__ __launch_bounds__(VS_CPLPC_THREADS, 4) void vs_cplpc_kernel(VsCplpcArgs a)
{
  extern __shared__ double cp_M[];
  __shared__ int cp_xs[VS_CPLPC_CHUNK + VS_MAX_ORDER];
  __shared__ double cp_a[VS_CPLPC_THREADS];
  __shared__ long f_out[1];
  __shared__ void *f_ptr[4]; /* the frame's outputs, kept here across the analysis: record, coefs, counts, formants */
  __shared__ int f_fs[1], f_status[1], f_nf[1];
  const int lane = threadIdx.x;
  const int p = a.lpc.order, S = vs_cplpc_stride(p);
  double *M = cp_M;

  const long g = blockIdx.x, lo = vs_frame_row(a.lpc.rows, a.lpc.n_lanes, g);
  const VsLpcRow R = a.lpc.rows[lo];
  const int fj = (int)(g - R.first);
  const long long fs0 = (long long)R.s0 + (long long)fj * R.H, fe = fs0 + R.L; /* 0 <= fs0, fe <= len */
  const int16_t *x = a.lpc.pcm + lo * a.lpc.pitch;
  const long out = lo * a.lpc.frames_pitch + fj;
  if (lane == 0) {
    f_out[0] = out;
    f_fs[0] = R.fs;
    f_ptr[0] = a.lpc.frames + out;
    f_ptr[1] = a.lpc.coefs ? a.lpc.coefs + out * (p + 1) : nullptr;
    f_ptr[2] = a.counts ? a.counts + out * 2 : nullptr;
    f_ptr[3] = a.lpc.formants;
  }

  const vs_glottal_rec *G = a.glottal + lo;
  long long C = (long long)G->n_cycles + (long long)G->n_rejected;
  if (C < 0 || (G->status & (VS_GL_NO_CYCLES | VS_GL_BAD_MARKS))) C = 0;
  if (C > a.cycles_pitch) C = a.cycles_pitch;
  const vs_glottal_cycle *cyc = a.cycles + lo * a.cycles_pitch;

  for (int idx = lane; idx < (p + 1) * S; idx += VS_CPLPC_THREADS) M[idx] = 0.0;

  /* 1. and 2.: the spans and their sums */
  long long racc = 0, n_eq = 0; /* phi(0, lane) */
  int spans = 0;
  bool full = false;
  for (long long c0 = 0; c0 < C && !full; c0 += 64) {
    const long long c = c0 + lane;
    long long b = 0, e = 0;
    bool cand = false;
    if (c < C) {
      const vs_glottal_cycle *cy = cyc + c;
      const int st = cy->status, per = cy->period;
      const int anc = a.anchor == VS_CP_ANCHOR_GCI ? cy->gci : a.anchor == VS_CP_ANCHOR_PEAK ? cy->peak : cy->close;
      if (st == 0 && per > 0) {
        b = (long long)anc + (long long)a.delay;
        e = b + ((long long)a.span_q * (long long)per) / 256;
        cand = b >= fs0 && e <= fe && e - b >= (long long)p + 1;
      }
    }
    unsigned long long mask = __ballot(cand);
    while (mask) {
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const long long sb = __shfl(b, src, 64), se = __shfl(e, src, 64);
      const long long neq = se - sb - p;
      if (n_eq + neq >= 2147483648LL) { /* the cut is at the first ACCEPTED span that crosses it: the clamp test first */
        bool bad = false;
        for (long long n = sb + lane; n < se; n += 64) bad |= cp_clamped(x[n]);
        if (__any(bad)) continue;
        full = true;
        break;
      }
      if (neq > VS_CPLPC_CHUNK) { /* more than one chunk: the clamp test before the first */
        bool bad = false;
        for (long long n = sb + lane; n < se; n += 64) bad |= cp_clamped(x[n]);
        if (__any(bad)) continue;
      }
      bool dropped = false;
      for (long long n0 = sb + p; n0 < se; n0 += VS_CPLPC_CHUNK) {
        const int m = (int)min((long long)VS_CPLPC_CHUNK, se - n0);
        __syncthreads();
        bool bad = false;
        for (int k = lane; k < p + m; k += 64) { /* x[n0 - p .. n0 + m) within [sb, se) */
          const int v = x[n0 - p + k];
          bad |= cp_clamped(v);
          cp_xs[k] = v;
        }
        __syncthreads();
        if (__any(bad)) { /* only a span of one chunk gets here with a clamped sample */
          dropped = true;
          break;
        }
        if (lane <= p) {
          const int *q = cp_xs + p;
          long long s = 0;
          for (int t = 0; t < m; t++) s += (long long)q[t] * (long long)q[t - lane];
          racc += s;
        }
        /* the corrections (i, d), summed as int64 where phi(i+1, i+1+d) will stand.  Rows i and p - 1 - i of their
         * triangle side by side are p + 1 of them: entry t = lane + 64 r is column c of pair rr */
        const bool head = n0 == sb + p, tail = n0 + m == se;
        if (head || tail) {
          int rr = 0, c = lane;
          for (int r = 0; r < VS_CPLPC_CORR; r++, c += 64) {
            while (c >= p + 1) {
              c -= p + 1;
              rr++;
            }
            int i = rr, d = c;
            bool ok = rr < (p + 1) / 2;
            if (c >= p - rr) {
              i = p - 1 - rr;
              d = c - (p - rr);
              ok = ok && i != rr;
            }
            if (ok) {
              const int pos = (i + 1) * S + i + 1 + d;
              long long v = __double_as_longlong(M[pos]);
              if (head) v += (long long)cp_xs[p - 1 - i] * (long long)cp_xs[p - 1 - i - d];
              if (tail) v -= (long long)cp_xs[p + m - 1 - i] * (long long)cp_xs[p + m - 1 - i - d];
              M[pos] = __longlong_as_double(v);
            }
          }
        }
      }
      if (dropped) continue;
      spans++;
      n_eq += neq;
    }
  }

  /* 3. the triangle */
  __syncthreads();
  if (lane <= p) {
    long long acc = racc;
    M[lane] = (double)acc;
    for (int i = 0; i < p - lane; i++) {
      const int pos = (i + 1) * S + i + 1 + lane;
      acc += __double_as_longlong(M[pos]);
      M[pos] = (double)acc;
    }
  }
  __syncthreads();

  /* 4. the solve */
  const double nan = __builtin_nan("");
  const double c00 = M[0];
  const int min_eq = a.min_equations ? a.min_equations : 2 * p;
  int status = n_eq < (long long)min_eq ? VS_CP_FEW_EQUATIONS : c00 == 0.0 ? VS_LPC_SILENT : 0;
  const bool row = lane >= 1 && lane <= p;
  double dreg = 1.0, areg = nan, err = nan;
  if (status == 0) {
    for (int j = 1; j <= p; j++) {
      double ureg = 0.0;
      if (row && lane < j) ureg = M[lane * S + j] * dreg; /* u_k = l_jk * d_k */
      double t = 0.0;
      if (row && lane >= j) t = M[j * S + lane]; /* c_ij; lane j: c_jj */
      for (int k = 1; k < j; k++) {
        const double uk = vs_readlane_f64(ureg, k);
        if (row && lane >= j) t = fma(-M[k * S + lane], uk, t);
      }
      const double dj = vs_readlane_f64(t, j);
      if (!(dj > 0.0 && dj <= 1.7976931348623157e308)) {
        status = VS_CP_SINGULAR;
        break;
      }
      if (lane == j) dreg = dj;
      __syncthreads();
      if (row && lane > j) M[j * S + lane] = t / dj;
      __syncthreads();
    }
  }
  if (status == 0) {
    double z = row ? -M[lane] : 0.0;
    for (int k = 1; k < p; k++) {
      const double zk = vs_readlane_f64(z, k);
      if (row && lane > k) z = fma(-M[k * S + lane], zk, z);
    }
    const double y = z / dreg;
    areg = y;
    for (int i = p - 1; i >= 1; i--) { /* a_p = y_p */
      double ai = vs_readlane_f64(y, i);
      for (int k = i + 1; k <= p; k++) ai = fma(-M[i * S + k], vs_readlane_f64(areg, k), ai);
      if (lane == i) areg = ai;
    }
    err = c00;
    for (int i = 1; i <= p; i++) err = fma(vs_readlane_f64(areg, i), M[i], err);
    /* the step-down of the coefficient tracks */
    double w = row ? areg : 0.0;
    for (int i = p; i >= 1; i--) {
      const double k = vs_readlane_f64(w, i);
      if (!(fabs(k) < 1.0)) {
        status = VS_CP_NOT_MINIMUM_PHASE;
        break;
      }
      if (i > 1) {
        const double d = 1.0 - k * k;
        const double rev = __shfl(w, (i - lane) & 63, 64);
        if (lane >= 1 && lane < i) w = (w - k * rev) / d;
      }
    }
  }

  __syncthreads();
  cp_a[lane] = row ? areg : 0.0;
  if (lane == 0) {
    f_status[0] = status;
    f_nf[0] = 0;
  }
  double *coefs = (double *)f_ptr[1];
  if (coefs && lane <= p) coefs[lane] = lane == 0 ? 1.0 : areg;
  __syncthreads();

  /* 5. roots and formants */
  if (a.lpc.n_formants > 0)
    vs_lpc_roots(cp_a, 1, p, 1, a.lpc.n_formants, a.lpc.f_lo, (double *)f_ptr[3], f_out, f_fs, f_status, f_nf, lane,
                 VS_CPLPC_THREADS);
  __syncthreads();

  if (lane == 0) {
    int32_t *counts = (int32_t *)f_ptr[2];
    vs_frame_record((vs_lpc_frame *)f_ptr[0], c00, err, (int)fs0, f_nf[0], f_status[0]);
    if (counts) {
      counts[0] = spans;
      counts[1] = (int)n_eq;
    }
  }
}

extern "C" hipError_t vs_launch_cplpc(const VsCplpcArgs *args, hipStream_t stream)
{
  if (args->lpc.total_frames <= 0) return hipSuccess;
  if (args->lpc.order < 1 || args->lpc.order > VS_MAX_ORDER) return hipErrorInvalidValue;
  if (args->lpc.total_frames > 0x7FFFFFFFL) return hipErrorInvalidValue;
  const size_t lds = (size_t)vs_cplpc_lds_bytes(args->lpc.order);
  hipLaunchKernelGGL(vs_cplpc_kernel, dim3((unsigned)args->lpc.total_frames), dim3(VS_CPLPC_THREADS), lds, stream, *args);
  return hipGetLastError();
}
