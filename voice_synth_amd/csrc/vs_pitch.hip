/*
 * vs_pitch.hip -- gfx950 kernels of the pitch track (include/voice_synth.h, "pitch track"): candidates per frame and one
 * Viterbi path per row, of int16 rows already on the device.
 *
 * Two kernels on the context's stream, one behind the other:
 *
 *   vs_pt_cand_kernel: ONE WORKGROUP (256 threads) PER FRAME of the call.  The frame's 3*tmax + 1 samples go into LDS as
 *       doubles.  r0 and e(tmin-1) come out of a block reduction (a silent frame ends there); r(t) out of the correlation
 *       core of vs_ac_corr.h, which the period kernel of the acoustic measurement runs once per row; e(t) is the running
 *       sum e(t+1) = e(t) + y[s+t+W]^2 - y[s+t]^2, as a block scan.  All of them are exact integers in fp64.  q(t) is one
 *       int64 division per lag.  The first wavefront then takes the seven largest keys (q << 12 | 4095 - index: q
 *       descending, t ascending) of the local maxima by seven wave maxima, and lane c stores the c-th best at its rank by
 *       lag: the record holds the candidates in ascending lag.
 *
 *   vs_pt_path_kernel: ONE WAVEFRONT PER ROW.  The 64 lanes are the 8 x 8 pairs (i = lane & 7: state of the frame before,
 *       j = lane >> 3: state of this frame) of a transition; the maximum over i is three xor-shuffles within a group of
 *       eight, ties to the smaller i.  The next frame's candidates are loaded while this frame's are reduced.  back goes
 *       into the records; the way back takes 64 frames at a time: lane l loads back of frame hi - l, the chain of states
 *       runs through 64 readlanes, and every lane writes lag, q and status of its own frame.  The chain of a row is short
 *       and bound by latency, not by throughput.
 *
 * Per-frame status goes into the record; there is no device trap and no loop without a bound set by the host's records.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_ac_corr.h"
#include "vs_pitch.h"

/* the row of frame g of the call: the last row whose first frame is <= g */
__device__ __forceinline__ long pt_frame_row(const VsPtRow *rows, long n_lanes, long g)
{
  long lo = 0, hi = n_lanes - 1;
  while (lo < hi) {
    const long mid = (lo + hi + 1) >> 1;
    if (rows[mid].first <= g) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int pt_wave_max_int(int v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* candidates                                                                                                        */

__global__ __launch_bounds__(VS_AC_A_THREADS) void vs_pt_cand_kernel(VsPtArgs a)
{
  extern __shared__ double pt_lds[];
  const long g = blockIdx.x;
  const long row = pt_frame_row(a.rows, a.n_lanes, g);
  const VsPtRow R = a.rows[row];
  const int f = (int)(g - R.first);
  if (f < 0 || f >= R.n_frames) return; /* (cannot happen with the host's records) */
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = 2 * R.tmax;
  const int s = f * R.H;
  const int nwin = W + R.tmax + 1;            /* samples s .. s + W + tmax <= len - 2 */
  const int tlo = R.tmin - 1, nl = vs_pt_lags(R.tmin, R.tmax);
  double *xs = pt_lds;                                   /* [nwin + zeros] */
  double *rp = xs + vs_ac_xs_doubles(R.tmax);            /* partial sums, then r(t) in rp[t - tlo]; then the keys */
  double *es = rp + vs_ac_rp_doubles(R.tmin, R.tmax);    /* e(t) in es[t - tlo] */
  double *red = es + vs_pt_e_doubles(R.tmin, R.tmax);    /* [2][4] block reduction, [4] + [4] the scan's wave totals */
  int *qv = (int *)(red + 16);                           /* q(t) in qv[t - tlo] */
  int *keys = (int *)rp;
  vs_pitch_frame *o = a.frames + row * a.frames_pitch + f;

  const int16_t *x = a.pcm + row * a.pitch + s;
  for (int i = tid; i < nwin; i += VS_AC_A_THREADS) xs[i] = (double)(int)x[i];
  for (int i = nwin + tid; i < vs_ac_xs_doubles(R.tmax); i += VS_AC_A_THREADS) xs[i] = 0.0;
  __syncthreads();

  double r0 = 0.0, e0 = 0.0;
  for (int k = tid; k < W; k += VS_AC_A_THREADS) {
    r0 = fma(xs[k], xs[k], r0);
    e0 = fma(xs[k + tlo], xs[k + tlo], e0);
  }
  r0 = vs_ac_wave_sum(r0);
  e0 = vs_ac_wave_sum(e0);
  if (lane == 0) {
    red[wave] = r0;
    red[4 + wave] = e0;
  }
  __syncthreads();
  r0 = (red[0] + red[1]) + (red[2] + red[3]);
  e0 = (red[4] + red[5]) + (red[6] + red[7]);
  const long long r0i = (long long)r0;
  const bool silent = r0i < (long long)W * a.silence_rms * a.silence_rms;
  if (tid == 0) {
    o->r0 = r0i;
    o->start = s;
    o->lag = 0;
    o->q = 0;
    o->reserved_ = 0;
  }
  if (tid >= 8 && tid < 16) o->back[tid - 8] = 0;
  if (silent) {
    if (tid == 0) {
      o->status = VS_PT_SILENT;
      o->n_cand = 0;
    }
    if (tid < VS_PT_MAX_CAND) {
      o->cand_lag[tid] = 0;
      o->cand_q[tid] = 0;
    }
    return;
  }

  vs_ac_lag_sums(xs, rp, tlo, nl, W, tid);

  /* e(t): thread tid owns the lags [i0, i1); d(i) = e(t+1) - e(t) */
  {
    const int c = (nl + VS_AC_A_THREADS - 1) / VS_AC_A_THREADS;
    const int i0 = min(nl, tid * c), i1 = min(nl, i0 + c);
    double own = 0.0;
    for (int i = i0; i < i1; i++) {
      const double hi = xs[tlo + i + W], lo = xs[tlo + i];
      own = fma(hi, hi, own);
      own = fma(-lo, lo, own);
    }
    double inc = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) red[8 + wave] = inc;
    __syncthreads();
    double v = e0 + (inc - own);
    for (int w = 0; w < wave; w++) v += red[8 + w];
    for (int i = i0; i < i1; i++) {
      es[i] = v;
      const double hi = xs[tlo + i + W], lo = xs[tlo + i];
      v = fma(hi, hi, v);
      v = fma(-lo, lo, v);
    }
  }
  __syncthreads();

  for (int i = tid; i < nl; i += VS_AC_A_THREADS) {
    const long long r = (long long)rp[i], den = r0i + (long long)es[i];
    qv[i] = (r > 0 && den > 0) ? (int)((r << 16) / den) : 0;
  }
  __syncthreads(); /* r(t) is used up: the keys take its place */
  for (int i = 1 + tid; i <= nl - 2; i += VS_AC_A_THREADS) {
    const int q = qv[i];
    keys[i] = (q > 0 && q > qv[i - 1] && q >= qv[i + 1]) ? ((q << 12) | (4095 - i)) : 0;
  }
  __syncthreads();
  if (wave != 0) return;

  int sel[VS_PT_MAX_CAND];
  int below = 0x7FFFFFFF;
#pragma unroll
  for (int c = 0; c < VS_PT_MAX_CAND; c++) {
    int m = 0;
    for (int i = 1 + lane; i <= nl - 2; i += 64) {
      const int k = keys[i];
      if (k < below) m = max(m, k);
    }
    m = pt_wave_max_int(m);
    sel[c] = m;
    below = m; /* (0 once the maxima are used up: nothing is below it) */
  }
  int mine = 0, n_cand = 0;
#pragma unroll
  for (int c = 0; c < VS_PT_MAX_CAND; c++) {
    if (lane == c) mine = sel[c];
    n_cand += sel[c] != 0;
  }
  if (lane < VS_PT_MAX_CAND) {
    /* a larger key index part is a smaller lag: the rank by lag counts the chosen ones with a smaller lag */
    const int idx = 4095 - (mine & 4095);
    int rank = 0;
#pragma unroll
    for (int c = 0; c < VS_PT_MAX_CAND; c++) rank += sel[c] != 0 && (4095 - (sel[c] & 4095)) < idx;
    if (mine != 0) {
      o->cand_lag[rank] = tlo + idx;
      o->cand_q[rank] = mine >> 12;
    } else { /* the chosen ones fill the slots 0 .. n_cand - 1; lane >= n_cand here */
      o->cand_lag[lane] = 0;
      o->cand_q[lane] = 0;
    }
  }
  if (lane == 0) {
    o->status = n_cand == 0 ? VS_PT_NO_CANDIDATE : 0;
    o->n_cand = n_cand;
  }
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* path                                                                                                              */

struct PtStates { /* what a lane reads of a frame: the states j and i of its pair */
  int nc, tj, qj, ti;
};

__device__ __forceinline__ PtStates pt_states(const vs_pitch_frame *fr, int i, int j)
{
  PtStates s;
  s.nc = fr->n_cand;
  const int lj = fr->cand_lag[j > 0 ? j - 1 : 0], qj = fr->cand_q[j > 0 ? j - 1 : 0];
  const int li = fr->cand_lag[i > 0 ? i - 1 : 0];
  s.tj = (j > 0 && j <= s.nc) ? lj : 0;
  s.qj = (j > 0 && j <= s.nc) ? qj : 0;
  s.ti = (i > 0 && i <= s.nc) ? li : 0;
  return s;
}

__global__ __launch_bounds__(64) void vs_pt_path_kernel(VsPtArgs a)
{
  __shared__ int lg[VS_AC_MAX_LAG + 1];
  const long row = blockIdx.x;
  const int lane = threadIdx.x;
  const VsPtRow R = a.rows[row];
  const int F = R.n_frames;
  if (F <= 0) return;
  for (int t = lane; t <= R.tmax; t += 64) lg[t] = a.lg[t];
  __syncthreads();
  vs_pitch_frame *fr = a.frames + row * a.frames_pitch;
  const int i = lane & 7, j = lane >> 3;
  const long long NEG = -(1LL << 62);
  const int lgmax = lg[R.tmax];

  auto local = [&](const PtStates &s) -> long long {
    if (j == 0) return (long long)a.voicing_q;
    if (j > s.nc) return NEG;
    return (long long)s.qj + (((long long)a.octave_q * (long long)(lgmax - lg[s.tj])) >> 8);
  };

  PtStates cur = pt_states(fr, i, j);
  PtStates nxt = F > 1 ? pt_states(fr + 1, i, j) : cur;
  long long delta = local(cur);                    /* of state j: the same in the eight lanes of a group */
  for (int f = 1; f < F; f++) {
    const long long dprev = __shfl(delta, i * 8, 64); /* of state i of the frame before */
    const int pti = cur.ti;
    cur = nxt;
    if (f + 1 < F) nxt = pt_states(fr + f + 1, i, j); /* on its way while this frame is reduced */
    long long tr;
    if (pti == 0 && cur.tj == 0) tr = 0;
    else if (pti == 0 || cur.tj == 0) tr = a.vuv_q;
    else {
      const int d = lg[pti] - lg[cur.tj];
      tr = ((long long)a.jump_q * (long long)(d < 0 ? -d : d)) >> 8;
    }
    long long v = dprev - tr; /* (a state the frame before does not have: NEG less something, never the maximum) */
    int from = i;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
      const long long ov = __shfl_xor(v, o, 64);
      const int of = __shfl_xor(from, o, 64);
      if (ov > v || (ov == v && of < from)) {
        v = ov;
        from = of;
      }
    }
    const bool have = j <= cur.nc;
    delta = have ? local(cur) + v : NEG;
    if (i == 0) fr[f].back[j] = have ? (uint8_t)from : (uint8_t)0;
  }

  /* the last frame's state: the largest delta, ties to the smallest j */
  int state = j;
  {
    long long v = delta;
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
      const long long ov = __shfl_xor(v, o, 64);
      const int os = __shfl_xor(state, o, 64);
      if (ov > v || (ov == v && os < state)) {
        v = ov;
        state = os;
      }
    }
  }

  /* the way back, 64 frames at a time; the back words were stored by other lanes of this wavefront */
  __threadfence();
  for (int hi = F - 1; hi >= 0; hi -= 64) {
    const int fl = hi - lane;
    unsigned long long B = 0;
    if (fl >= 0)
      B = __hip_atomic_load((const unsigned long long *)fr[fl].back, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int mine = 0;
    const int n = min(64, hi + 1);
    for (int k = 0; k < n; k++) {
      if (lane == k) mine = state;
      const unsigned long long Bk = __shfl(B, k, 64);
      state = (int)(Bk >> (8 * state)) & 7; /* the state of frame hi - k - 1 */
    }
    if (fl >= 0) {
      vs_pitch_frame *o = fr + fl;
      if (mine == 0) {
        o->lag = 0;
        o->q = a.voicing_q;
        o->status = o->status | VS_PT_UNVOICED;
      } else {
        o->lag = o->cand_lag[mine - 1];
        o->q = o->cand_q[mine - 1];
      }
    }
  }
}

extern "C" hipError_t vs_launch_pitch(const VsPtArgs *args, int lds_doubles, hipStream_t stream)
{
  if (args->n_lanes <= 0 || args->n_lanes > 0x7FFFFFFFL || args->total_frames < 0 || args->total_frames > 0x7FFFFFFFL)
    return hipErrorInvalidValue;
  if (args->total_frames == 0) return hipSuccess;
  const size_t lds = (size_t)lds_doubles * sizeof(double);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)vs_pt_cand_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(vs_pt_cand_kernel, dim3((unsigned)args->total_frames), dim3(VS_AC_A_THREADS), lds, stream, *args);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vs_pt_path_kernel, dim3((unsigned)args->n_lanes), dim3(64), 0, stream, *args);
  return hipGetLastError();
}
