/*
 * vs_guided.hip -- gfx950 kernels of the guided marks (include/voice_synth.h, "guided marks"): the cycle walk of the
 * acoustic measurement, steered frame by frame by the pitch track, of int16 rows already on the device.
 *
 * Two kernels on the context's stream, one behind the other:
 *
 *   vs_mg_plan_kernel: ONE WAVEFRONT PER ROW.  Lane l takes frame 64c + l of chunk c (the records are 96 bytes apart:
 *       the lanes stride, and read lag and q only).  A forward pass gives every frame the first frame of its voiced
 *       stretch (a ballot, the highest unvoiced bit below the lane, a carry from the chunk before); a backward pass the
 *       last one (the lowest unvoiced bit above, a carry from the chunk behind), and with both the trim, min_frames and
 *       whether the frame is walked.  It writes the compact lag array (0 where nothing is walked) and the link array
 *       (the run's last frame; outside a run the next run's first), sums Q and nF, and for VS_MG_LONGEST keeps the best
 *       (frames, first) key and clears the other runs in a third pass.
 *
 *   vs_mg_walk_kernel: ONE LANE PER ROW, 64 rows per workgroup: the streaming scheme of vs_ac_marks_kernel
 *       (vs_acoustic.hip; its walk state and step are restated here, not shared: this step restarts at every run, reads
 *       one lag per mark and counts pairs, triples and quintuples per run).  [64 rows x VS_MG_TILE] int16 tiles stream
 *       through LDS, the next tile in registers; each lane walks its row forward with O(1) state.  A window that begins
 *       at or before the sample just walked is resolved by walking that stretch again from the row in HBM.
 *
 * Per-row status goes into the record; there is no device trap and nothing stops a wavefront but its own rows.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_guided.h"

#define MG_INT_MIN (-0x7FFFFFFF - 1)
#define MG_INT_MAX 0x7FFFFFFF

/* ---------------------------------------------------------------------------------------------------------------- */
/* plan                                                                                                              */

__device__ __forceinline__ unsigned long long mg_above(int lane) { return ~((2ull << lane) - 1ull); } /* lanes > lane */

__global__ __launch_bounds__(64) void vs_mg_plan_kernel(VsMgArgs a)
{
  const long row = blockIdx.x;
  const int lane = threadIdx.x;
  const VsMgRow R = a.rows[row];
  const int F = R.n_frames;
  VsMgHead *head = a.head + row;
  if (F <= 0) {
    if (lane == 0) {
      head->Q = 0;
      head->nF = 0;
      head->first = 0;
    }
    return;
  }
  const vs_pitch_frame *fr = a.frames + row * a.frames_pitch;
  int32_t *lag = a.lag + row * a.frames_pitch, *link = a.link + row * a.frames_pitch;
  const int chunks = (F + 63) / 64;
  const int edge = a.edge_frames;

  /* forward: the first frame of every frame's voiced stretch, into link[] for the pass behind */
  int carry = -1; /* the first frame of the stretch that reaches this chunk from the one before; -1: none */
  for (int c = 0; c < chunks; c++) {
    const int base = c * 64, f = base + lane;
    const int lg = f < F ? fr[f].lag : 0;
    const bool v = f < F && lg >= R.tmin && lg <= R.tmax;
    const unsigned long long M = __ballot(v);
    const unsigned long long below = ~M & ((1ull << lane) - 1ull);
    const int s = below ? base + 64 - __clzll((long long)below) : (carry >= 0 ? carry : base);
    if (f < F) link[f] = s;
    const int s63 = __shfl(s, 63, 64);
    carry = (M >> 63) ? s63 : -1;
  }

  /* backward: the last frame, the trim, what is walked */
  int ecarry = -1; /* the last frame of the stretch that reaches this chunk from the one behind; -1: none */
  int next = F;    /* the first frame of the first walked run behind this chunk */
  long long best = -1, Q = 0;
  int nF = 0;
  for (int c = chunks - 1; c >= 0; c--) {
    const int base = c * 64, f = base + lane;
    int lg = 0, q = 0, s = 0;
    if (f < F) {
      lg = fr[f].lag;
      q = fr[f].q;
      s = link[f];
    }
    const bool v = f < F && lg >= R.tmin && lg <= R.tmax;
    const unsigned long long M = __ballot(v);
    const unsigned long long above = ~M & mg_above(lane);
    const int e = above ? base + __ffsll((long long)above) - 2 : (ecarry >= 0 ? ecarry : base + 63);
    const int e0 = __shfl(e, 0, 64);
    ecarry = (M & 1ull) ? e0 : -1;
    const int fa = s + (s > 0 ? edge : 0), fb = e - (e < F - 1 ? edge : 0);
    const bool walked = v && fb - fa + 1 >= a.min_frames && f >= fa && f <= fb;
    const bool starts = walked && f == fa;
    if (starts) best = max(best, ((long long)(fb - fa + 1) << 32) | (long long)(MG_INT_MAX - fa));
    const unsigned long long S = __ballot(starts);
    const unsigned long long Sa = S & mg_above(lane);
    if (f < F) {
      lag[f] = walked ? lg : 0;
      link[f] = walked ? fb : (Sa ? base + __ffsll((long long)Sa) - 1 : next);
    }
    if (S) next = base + __ffsll((long long)S) - 1;
    if (walked) {
      Q += min(max(q, 0), 32768);
      nF++;
    }
  }

  if (a.segments == VS_MG_LONGEST) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
    const int bfa = best < 0 ? F : MG_INT_MAX - (int)(best & 0x7FFFFFFFLL);
    const int bfb = best < 0 ? F : bfa + (int)(best >> 32) - 1;
    Q = 0;
    nF = 0;
    for (int c = 0; c < chunks; c++) {
      const int f = c * 64 + lane;
      if (f >= F) continue;
      const int lg = lag[f];
      const bool walked = lg > 0 && f >= bfa && f <= bfb;
      lag[f] = walked ? lg : 0;
      link[f] = walked ? bfb : (f < bfa ? bfa : F);
      if (walked) {
        Q += min(max(fr[f].q, 0), 32768);
        nF++;
      }
    }
    next = bfa;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Q += __shfl_xor(Q, o, 64);
    nF += __shfl_xor(nF, o, 64);
  }
  if (lane == 0) {
    head->Q = Q;
    head->nF = nF;
    head->first = next;
  }
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* walk                                                                                                              */

struct MgWalk {
  int fb;         /* last frame of the run being walked */
  int b;          /* its samples end here */
  int m;          /* last mark of the run (-1: looking for its m_0) */
  int wlo, whi;   /* window of the next mark */
  int best, bpos; /* running argmax over the window (first index on ties) */
  int amin;       /* min y over [m, bpos) */
  int msince;     /* min y over [bpos, current sample] */
  int runmin;     /* min y over [m, current sample) */
  int done;
  int m0, p0;     /* the first mark of the first run, the lag of its frame */
  int kr;         /* periods of this run */
  int K, nm;      /* periods, marks of the row */
  int N2, N3, N5; /* adjacent pairs, triples, quintuples within runs */
  int nseg, seg_mark, seg_frame;
  int T1, T2, T3, T4, A1, A2, A3, A4; /* the last four periods and amplitudes of this run (1 = latest) */
  long long sT, sdT, s3T, s5T, sA, sdA, s3A, s5A;
  double sdb;
  int zero_amp;
};

/* where a row's scratch and outputs lie: only the lag pointer is kept per lane, the rest is computed when it is used */
struct MgRowPtrs {
  const int32_t *lag;
  long link_off; /* link = lag + link_off (the same for every row) */
  long row;
};

__device__ __forceinline__ int mg_abs(int v) { return v < 0 ? -v : v; }

__device__ __forceinline__ int mg_frame_of(const VsMgRow &R, int n)
{
  /* (unsigned: n - C + H/2 may pass 2^31 in a very long row) */
  return n <= R.C ? 0 : (int)min((unsigned)(R.n_frames - 1), ((unsigned)(n - R.C) + (unsigned)(R.H / 2)) / (unsigned)R.H);
}

/* the run that begins with frame fa: its samples [a, b), the window of its first mark */
__device__ __forceinline__ void mg_enter(MgWalk &w, const VsMgRow &R, const MgRowPtrs &P, int fa)
{
  const int fb = P.lag[P.link_off + fa];
  /* (the products stay below 2^31: the frames' centres lie inside the row) */
  const int a = fa == 0 ? 0 : R.C + fa * R.H - R.H / 2;
  const int b = fb == R.n_frames - 1 ? R.len : min(R.len, R.C + (fb + 1) * R.H - R.H / 2);
  w.fb = fb;
  w.b = b;
  w.m = -1;
  w.wlo = a;
  w.whi = min(a + P.lag[fa], b) - 1;
  w.best = MG_INT_MIN;
  w.runmin = MG_INT_MAX;
  w.kr = 0;
  w.seg_mark = w.nm;
  w.seg_frame = fa;
}

/* one sample j (value v) of the walk; true when the next window begins at or before j (walk again from the new mark) */
__device__ __forceinline__ bool mg_step(MgWalk &w, const VsMgArgs &a, const VsMgRow &R, const MgRowPtrs &P, int j, int v)
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
  const int lagf = P.lag[mg_frame_of(R, mn)];
  const int lo1 = max(R.tmin, (2 * lagf + 2) / 3), hi1 = min(R.tmax, (3 * lagf) / 2), d = (lagf + 3) / 4;
  int lo = lo1, hi = hi1;
  if (w.m < 0) {
    if (w.nm == 0) {
      w.m0 = mn;
      w.p0 = lagf;
    }
  } else {
    const int T = mn - w.m, A = w.best - w.amin;
    w.K++;
    w.kr++;
    w.sT += T;
    w.sA += A;
    if (A <= 0) w.zero_amp = 1;
    if (w.kr >= 2) {
      w.N2++;
      w.sdT += mg_abs(T - w.T1);
      w.sdA += mg_abs(A - w.A1);
      if (A > 0 && w.A1 > 0) w.sdb += fabs(20.0 * log10((double)A / (double)w.A1));
    }
    if (w.kr >= 3) {
      w.N3++;
      w.s3T += mg_abs(3 * w.T1 - (w.T2 + w.T1 + T));
      w.s3A += mg_abs(3 * w.A1 - (w.A2 + w.A1 + A));
    }
    if (w.kr >= 5) {
      w.N5++;
      w.s5T += mg_abs(5 * w.T2 - (w.T4 + w.T3 + w.T2 + w.T1 + T));
      w.s5A += mg_abs(5 * w.A2 - (w.A4 + w.A3 + w.A2 + w.A1 + A));
    }
    w.T4 = w.T3; w.T3 = w.T2; w.T2 = w.T1; w.T1 = T;
    w.A4 = w.A3; w.A3 = w.A2; w.A2 = w.A1; w.A1 = A;
    const int lo2 = max(lo1, T - d), hi2 = min(hi1, T + d);
    if (lo2 <= hi2) { /* else the track jumped: the window of a second mark */
      lo = lo2;
      hi = hi2;
    }
  }
  if (a.marks && w.nm < a.marks_pitch) a.marks[P.row * a.marks_pitch + w.nm] = mn;
  w.nm++;
  w.m = mn;
  w.wlo = mn + lo;
  w.whi = mn + hi;
  w.best = MG_INT_MIN;
  if (w.whi >= w.b) { /* the run ends: its record, then the next run or none */
    if (a.segs && w.nseg < a.seg_pitch) {
      vs_guided_seg *s = a.segs + P.row * a.seg_pitch + w.nseg;
      s->first_frame = w.seg_frame;
      s->n_frames = w.fb - w.seg_frame + 1;
      s->first_mark_index = w.seg_mark;
      s->n_marks = w.nm - w.seg_mark;
    }
    w.nseg++;
    const int nf = w.fb + 1 < R.n_frames ? P.lag[P.link_off + w.fb + 1] : R.n_frames;
    if (nf >= R.n_frames) {
      w.done = 1;
      return false;
    }
    mg_enter(w, R, P, nf); /* its first sample lies behind j */
    return false;
  }
  if (w.wlo <= j) {
    w.runmin = MG_INT_MAX;
    return true;
  }
  w.runmin = w.msince;
  return false;
}

__device__ __forceinline__ void mg_record_empty(vs_acoustic *o, vs_guided_rec *r, int status)
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
  r->n_segments = 0;
  r->n_marks = 0;
  r->n_frames_walked = 0;
  r->reserved_ = 0;
}

__global__ __launch_bounds__(64) void vs_mg_walk_kernel(VsMgArgs a)
{
  __shared__ uint32_t tile[64 * (VS_MG_TILE + VS_MG_PAD) / 2];
  const int lane = threadIdx.x;
  const long row0 = (long)blockIdx.x * 64, row = row0 + lane;
  const bool live = row < a.n_lanes;
  VsMgRow R = {0, 1, 2, 3, 1, 0, 4, 0};
  VsMgHead hd = {0, 0, 0};
  MgRowPtrs P = {};
  if (live) {
    R = a.rows[row];
    hd = a.head[row];
    P.lag = a.lag + row * a.frames_pitch;
    P.link_off = a.link - a.lag;
    P.row = row;
  }
  const int status = R.n_frames <= 0 ? VS_AC_TOO_SHORT : (hd.first >= R.n_frames ? VS_AC_UNVOICED : 0);
  MgWalk w = {};
  w.m0 = -1;
  w.done = (status != 0);
  if (!w.done) mg_enter(w, R, P, hd.first);
  int need = w.done ? 0 : R.len;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) need = max(need, __shfl_xor(need, o, 64));

  const int rows_here = (int)min((long)64, a.n_lanes - row0);
  const int16_t *base = a.pcm + row0 * a.pitch;
  const int16_t *mine = a.pcm + row * a.pitch;
  int pf[VS_MG_TILE / 64][64]; /* the next tile: [column block][row of the workgroup] */
  auto fetch = [&](int t0) {
#pragma unroll
    for (int cb = 0; cb < VS_MG_TILE / 64; cb++) {
      const long col = (long)t0 + cb * 64 + lane;
#pragma unroll
      for (int r = 0; r < 64; r++)
        pf[cb][r] = (r < rows_here && col < (long)a.n_samples) ? (int)base[r * a.pitch + col] : 0;
    }
  };
  if (need > 0) fetch(0);
  for (int t0 = 0; t0 < need; t0 += VS_MG_TILE) {
    __syncthreads();
    uint16_t *t16 = (uint16_t *)tile;
#pragma unroll
    for (int cb = 0; cb < VS_MG_TILE / 64; cb++)
#pragma unroll
      for (int r = 0; r < 64; r++) t16[r * (VS_MG_TILE + VS_MG_PAD) + cb * 64 + lane] = (uint16_t)pf[cb][r];
    __syncthreads();
    if (t0 + VS_MG_TILE < need) fetch(t0 + VS_MG_TILE);
    if (__ballot(!w.done) == 0) break; /* every row of the wavefront is through */
    if (w.done) continue;
    const uint32_t *my = tile + lane * ((VS_MG_TILE + VS_MG_PAD) / 2);
    const int cend = min(VS_MG_TILE, R.len - t0);
    for (int c = 0; c < cend && !w.done; c += 2) {
      const uint32_t pair = my[c / 2];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int j = t0 + c + h;
        if (w.done || j >= R.len) break;
        const int v = a.polarity * (int)(int16_t)(h ? (pair >> 16) : (pair & 0xFFFFu));
        if (mg_step(w, a, R, P, j, v)) {
          int q = w.m; /* walk [m, j] again from HBM */
          while (q <= j && !w.done) q = mg_step(w, a, R, P, q, a.polarity * (int)mine[q]) ? w.m : q + 1;
        }
      }
    }
  }
  if (!live) return;

  vs_acoustic *o = a.out + row;
  vs_guided_rec *g = a.rec + row;
  if (status != 0) {
    mg_record_empty(o, g, status);
    return;
  }
  const double nan = __builtin_nan("");
  const int K = w.K;
  double f0 = nan, jl = nan, jabs = nan, rap = nan, ppq = nan, sl = nan, sdb = nan, apq3 = nan, apq5 = nan;
  if (K >= 1) {
    const double Tm = (double)w.sT / (double)K;
    f0 = (double)R.fs / Tm;
    if (w.N2 >= 1) {
      jl = ((double)w.sdT / (double)w.N2) / Tm;
      jabs = ((double)w.sdT / (double)w.N2) / (double)R.fs;
    }
    if (w.N3 >= 1) rap = ((double)w.s3T / (3.0 * (double)w.N3)) / Tm;
    if (w.N5 >= 1) ppq = ((double)w.s5T / (5.0 * (double)w.N5)) / Tm;
    if (!w.zero_amp) {
      const double Am = (double)w.sA / (double)K;
      if (w.N2 >= 1) {
        sl = ((double)w.sdA / (double)w.N2) / Am;
        sdb = w.sdb / (double)w.N2;
      }
      if (w.N3 >= 1) apq3 = ((double)w.s3A / (3.0 * (double)w.N3)) / Am;
      if (w.N5 >= 1) apq5 = ((double)w.s5A / (5.0 * (double)w.N5)) / Am;
    }
  }
  double rho = (double)hd.Q / (32768.0 * (double)hd.nF);
  rho = fmin(fmax(rho, 1e-10), 1.0 - 1e-10);
  o->f0_hz = f0;
  o->jitter_local = jl;
  o->jitter_abs_s = jabs;
  o->jitter_rap = rap;
  o->jitter_ppq5 = ppq;
  o->shimmer_local = sl;
  o->shimmer_db = sdb;
  o->shimmer_apq3 = apq3;
  o->shimmer_apq5 = apq5;
  o->hnr_db = 10.0 * log10(rho / (1.0 - rho));
  o->p0 = w.nm > 0 ? w.p0 : 0;
  o->n_periods = K;
  o->first_mark = w.m0;
  o->status = (K < 2 ? VS_AC_FEW_PERIODS : 0) | (K >= 1 && w.zero_amp ? VS_AC_ZERO_AMPLITUDE : 0);
  g->n_segments = w.nseg;
  g->n_marks = w.nm;
  g->n_frames_walked = hd.nF;
  g->reserved_ = 0;
}

extern "C" hipError_t vs_launch_guided(const VsMgArgs *args, hipStream_t stream)
{
  if (args->n_lanes <= 0 || args->n_lanes > 0x7FFFFFFFL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vs_mg_plan_kernel, dim3((unsigned)args->n_lanes), dim3(64), 0, stream, *args);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vs_mg_walk_kernel, dim3((unsigned)((args->n_lanes + 63) / 64)), dim3(64), 0, stream, *args);
  return hipGetLastError();
}
