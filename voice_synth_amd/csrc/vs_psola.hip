/*
 * vs_psola.hip -- gfx950 kernels of PSOLA (include/voice_synth.h, "PSOLA"): the cycles of an int16 row already on the
 * device, placed at the instants a target of periods asks for.
 *
 * Two kernels on the context's stream, one behind the other:
 *
 *   vs_ps_plan_kernel: ONE LANE PER ROW, 64 rows per workgroup: stage A is a chain -- every synthesis mark needs the one
 *       before it -- and the rows are what runs side by side.  A run is checked in one pass over its marks (which also
 *       finds its shortest period); the walk then keeps O(1) state: the mark, its index, the governing cycle before, and
 *       a cursor into the target that only moves forward (the marks of a row increase, so the prefix scan of a later
 *       mark starts where the scan of an earlier one ended).  A run whose marks are sure to fit the slots that are left
 *       -- (E - a_0) / min(pmin, shortest period) + 2 of them -- is written as it is walked; else it is walked once to
 *       count and, if it fits, once more to write: nothing is stored that the row's count does not cover.  Next to
 *       every vs_psola_mark goes a VsPsAux into the launch's scratch.
 *
 *   vs_ps_ola_kernel: ONE WORKGROUP PER (ROW, TILE), 256 lanes, a lane per 16-byte piece of the OUTPUT row (8 samples;
 *       the tiles are cut at the row's 16-byte addresses, vs_psola.h).  The workgroup finds the first synthesis mark of
 *       its tile by a 256-way section of the row's records (every lane reads one record, a barrier counts the lanes at or
 *       below the tile's first sample, the stretch between two probes is searched next: two rounds for 65536 records),
 *       stages up to VS_PS_STAGE marks in LDS and, when the tile holds more, goes on from the last one staged.  A lane
 *       finds the interval of its first sample by bisection in LDS and steps on from there; copy regions -- in front of a
 *       run, behind it, rows without a run -- go through the same code.  A piece that lies inside the row is stored as
 *       one dwordx4, the pieces at the row's ends sample by sample.
 *
 * Every index into the PCM is checked against the row (outside it a sample reads as 0), every record index against
 * n_synth and the pitch: a wrong record costs wrong samples, never an access outside the arrays.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_psola.h"

#define PS_Q 32768
#define PS_INT_MAX 0x7FFFFFFF
#define PS_END_BIT 0x10000 /* in the staged gain word: the mark is a run's last */

__device__ __forceinline__ int ps_ld(const char *base, long index, int stride)
{
  return *(const int32_t *)(base + index * (long)stride);
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* plan                                                                                                              */

struct PsTarget {
  const char *start, *period, *gain; /* of the row */
  int ss, ps, gs;
  int J, pmin, pmax;
};

struct PsRun {
  const int32_t *a; /* the run's marks */
  int m, first;
};

__device__ __forceinline__ int ps_pr(const PsRun &r, int k)
{
  return k < r.m - 1 ? r.a[k + 1] - r.a[k] : r.a[k] - r.a[k - 1];
}
__device__ __forceinline__ int ps_pl(const PsRun &r, int k) { return k > 0 ? r.a[k] - r.a[k - 1] : r.a[1] - r.a[0]; }

/* Stage A on one usable run.  WRITE: the records go to rec[0..] and aux[0..] (the caller has made sure they fit);
 * else nothing is stored and the walk ends once it has counted more than `room` marks.  p: the target's cursor, the
 * first index whose start lies above the last mark that looked (J: none).  Returns the number of marks. */
template <bool WRITE>
__device__ int ps_walk(const PsRun &r, const PsTarget &tg, int &p, int room, vs_psola_mark *rec, VsPsAux *aux, int &governed)
{
  const int E = r.a[r.m - 1];
  int t = r.a[0], k = 0, ak = t, n = 0, gov = 0;
  int prev = -1, sprev = 0, tprev = 0; /* the governing cycle of the mark before, its start and period */
  for (;;) {
    int c = -1, sc = 0, tc = 0;
    if (prev >= 0 && prev + 1 < tg.J && (long)(sc = ps_ld(tg.start, prev + 1, tg.ss)) == (long)sprev + (long)tprev) {
      c = prev + 1;
      tc = ps_ld(tg.period, c, tg.ps);
    } else {
      while (p < tg.J && ps_ld(tg.start, p, tg.ss) <= t) p++;
      if (p > 0) {
        sc = ps_ld(tg.start, p - 1, tg.ss);
        tc = ps_ld(tg.period, p - 1, tg.ps);
        if ((long)t < (long)sc + (long)tc) c = p - 1;
      }
    }
    int g = PS_Q;
    if (c >= 0) {
      if (tg.gain) g = ps_ld(tg.gain, c, tg.gs);
      if (tc < tg.pmin || tc > tg.pmax || g < 0 || g > 65535) c = -1;
    }
    const int pr = ps_pr(r, k);
    const int Ti = c >= 0 ? tc : pr;
    if (c < 0) g = PS_Q;
    if (WRITE) {
      vs_psola_mark mk = {t, r.first + k, c, n == 0 ? PS_Q : g};
      VsPsAux ax = {ak, pr | (ps_pl(r, k) << 16)};
      rec[n] = mk;
      aux[n] = ax;
    }
    n++;
    gov += c >= 0;
    prev = c;
    sprev = sc;
    tprev = tc;
    if (E - t <= Ti + Ti / 2) {
      if (WRITE) {
        vs_psola_mark mk = {E, r.first + r.m - 1, VS_PS_RUN_END, PS_Q};
        VsPsAux ax = {E, ps_pr(r, r.m - 1) | (ps_pl(r, r.m - 1) << 16)};
        rec[n] = mk;
        aux[n] = ax;
      }
      n++;
      break;
    }
    if (!WRITE && n >= room) { /* this mark and the run's last: more than room */
      n = room + 1;
      break;
    }
    t += Ti;
    /* the nearest mark at or behind k, ties to the smaller: the distances fall, then rise */
    while (k < r.m - 1) {
      const int nx = r.a[k + 1];
      if (abs(nx - t) >= abs(ak - t)) break;
      ak = nx;
      k++;
    }
  }
  governed += gov;
  return n;
}

__global__ __launch_bounds__(64) void vs_ps_plan_kernel(VsPsArgs a)
{
  const long row = (long)blockIdx.x * 64 + threadIdx.x;
  if (row >= a.n_lanes) return;
  const int len = a.rows[row].length;
  const int32_t *marks = a.marks + row * a.marks_pitch;
  const vs_guided_rec gr = a.rec[row];
  vs_psola_mark *rec = a.synth + row * a.synth_pitch;
  VsPsAux *aux = a.aux + row * a.synth_pitch;
  const int slots = (int)a.synth_pitch;

  PsTarget tg;
  const long t0 = row * a.target_pitch;
  tg.start = a.start + t0 * a.start_stride;
  tg.period = a.period + t0 * a.period_stride;
  tg.gain = a.gain ? a.gain + t0 * a.gain_stride : nullptr;
  tg.ss = a.start_stride;
  tg.ps = a.period_stride;
  tg.gs = a.gain_stride;
  const int count = ps_ld(a.count, row, a.count_stride);
  tg.J = count < 0 ? 0 : (long)count > a.target_pitch ? (int)a.target_pitch : count;
  tg.pmin = a.pmin;
  tg.pmax = a.pmax;

  int n_runs;
  if (a.segs) n_runs = gr.n_segments < 0 ? 0 : (long)gr.n_segments > a.seg_pitch ? (int)a.seg_pitch : gr.n_segments;
  else n_runs = 1;
  const vs_guided_seg *segs = a.segs ? a.segs + row * a.seg_pitch : nullptr;

  int status = 0, done = 0, n_synth = 0, governed = 0;
  int prev_end = -1, p = 0;
  for (int q = 0; q < n_runs; q++) {
    int first, m;
    if (segs) {
      first = segs[q].first_mark_index;
      m = segs[q].n_marks;
    } else {
      first = 0;
      m = (long)gr.n_marks > a.marks_pitch ? (int)a.marks_pitch : gr.n_marks;
    }
    /* usable?  the ends first, then every step; the shortest period on the way */
    bool ok = m >= 2 && first >= 0 && (long)first + (long)m <= a.marks_pitch;
    int shortest = PS_INT_MAX;
    if (ok) {
      int before = marks[first];
      ok = before > prev_end && marks[first + m - 1] < len; /* (prev_end >= -1: the first mark is not negative) */
      for (int j = 1; j < m && ok; j++) {
        const int v = marks[first + j];
        const long step = (long)v - (long)before;
        ok = step > 0 && step <= VS_AC_MAX_LAG;
        shortest = step < shortest ? (int)step : shortest;
        before = v;
      }
    }
    if (!ok) {
      status |= VS_PS_BAD_RUN;
      continue;
    }
    PsRun r = {marks + first, m, first};
    const int room = slots - n_synth;
    const int least = shortest < tg.pmin ? shortest : tg.pmin;
    const long bound = (long)(r.a[m - 1] - r.a[0]) / least + 2;
    if (bound > room) {
      int pc = p, gc = 0;
      if (ps_walk<false>(r, tg, pc, room, nullptr, nullptr, gc) > room) {
        status |= VS_PS_OVERFLOW; /* this run and the later ones are copied */
        break;
      }
    }
    n_synth += ps_walk<true>(r, tg, p, room, rec + n_synth, aux + n_synth, governed);
    prev_end = r.a[m - 1];
    done++;
  }
  vs_psola_stat st;
  st.status = status | (done == 0 ? VS_PS_NO_RUN : 0);
  st.n_runs = n_runs;
  st.n_runs_done = done;
  st.n_synth = n_synth;
  st.n_governed = governed;
  st.n_clipped = 0; /* the overlap-add kernel adds */
  a.stat[row] = st;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* overlap-add                                                                                                       */

__global__ __launch_bounds__(VS_PS_BLOCK) void vs_ps_ola_kernel(VsPsArgs a, unsigned tiles)
{
  __shared__ int s_t[VS_PS_STAGE], s_a[VS_PS_STAGE], s_pp[VS_PS_STAGE], s_g[VS_PS_STAGE];
  __shared__ int s_count[4];
  const long row = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  const int tid = threadIdx.x;
  const int len = a.rows[row].length;
  const int16_t *x = a.pcm + row * a.pitch;
  int16_t *y = a.out + row * a.out_pitch;
  const int mis = (int)(((uintptr_t)y >> 1) & (VS_PS_PER_LANE - 1));
  const long tile0 = (long)tile * VS_PS_TILE - mis; /* y + tile0 is a 16-byte address */
  const long lo_n = tile0 < 0 ? 0 : tile0;
  const long hi_n = tile0 + VS_PS_TILE < (long)len ? tile0 + VS_PS_TILE : (long)len;
  if (lo_n >= hi_n) return; /* (the whole workgroup) */
  int ns = a.stat[row].n_synth;
  ns = ns < 0 ? 0 : (long)ns > a.synth_pitch ? (int)a.synth_pitch : ns;
  const vs_psola_mark *rec = a.synth + row * a.synth_pitch;
  const VsPsAux *aux = a.aux + row * a.synth_pitch;
  const long n0 = tile0 + (long)VS_PS_PER_LANE * tid; /* the lane's piece */
  int clipped = 0;

  long pos = tile0; /* what lies in front of it is done; always a piece's first sample */
  while (pos < hi_n) {
    const int from = (int)(pos < lo_n ? lo_n : pos);
    /* the number of records with t <= from, by section */
    long lo = 0, hi = ns;
    while (hi > lo) {
      const long step = (hi - lo + VS_PS_BLOCK - 1) / VS_PS_BLOCK;
      const long at = lo + tid * step;
      int below = 0;
      if (at < hi) below = rec[at].t <= from;
      if (tid == 0) s_count[0] = 0;
      __syncthreads();
      if (below) atomicAdd(&s_count[0], 1);
      __syncthreads();
      const int cnt = s_count[0];
      __syncthreads();
      if (cnt == 0) {
        hi = lo;
      } else {
        const long nhi = lo + cnt * step;
        lo = lo + (cnt - 1) * step + 1;
        hi = nhi < hi ? nhi : hi;
      }
    }
    const long first = lo > 0 ? lo - 1 : 0;
    const int cnt = (int)(ns - first < VS_PS_STAGE ? ns - first : VS_PS_STAGE);
    __syncthreads(); /* (the pass before has read what this one stages) */
    if (tid < cnt) {
      const vs_psola_mark mk = rec[first + tid];
      const VsPsAux ax = aux[first + tid];
      s_t[tid] = mk.t;
      s_a[tid] = ax.a;
      s_pp[tid] = ax.periods;
      s_g[tid] = (mk.gain & 0xFFFF) | (mk.cycle == VS_PS_RUN_END ? PS_END_BIT : 0);
    }
    __syncthreads();
    /* what the staged marks cover: up to the last of them, cut to a piece's first sample; everything when no record
     * is left behind them */
    long cov = hi_n;
    if (first + cnt < ns) {
      const long last = s_t[cnt - 1];
      if (last < hi_n) cov = tile0 + ((last - tile0) & ~(long)(VS_PS_PER_LANE - 1));
      if (cov <= pos) cov = hi_n; /* (cannot happen: VS_PS_STAGE marks lie at least VS_PS_STAGE - 1 samples apart) */
    }
    if (n0 >= pos && n0 < cov) {
      const long b = n0 < lo_n ? lo_n : n0, e = n0 + VS_PS_PER_LANE < hi_n ? n0 + VS_PS_PER_LANE : hi_n;
      /* the last staged mark at or before b; -1: none */
      int s = -1;
      {
        int l = 0, h = cnt;
        while (l < h) {
          const int mid = (l + h) >> 1;
          if (s_t[mid] <= b) l = mid + 1;
          else h = mid;
        }
        s = l - 1;
      }
      int cur = -2, t0 = 0, G = 0, A = 0, B = 0, L = 1, L2 = 1, g0 = 0, g1 = 0;
      union {
        int16_t v[VS_PS_PER_LANE];
        int4 q;
      } piece;
#pragma unroll
      for (int j = 0; j < VS_PS_PER_LANE; j++) {
        const long n = n0 + j;
        int16_t out = 0;
        if (n >= b && n < e) {
          while (s + 1 < cnt && s_t[s + 1] <= n) s++;
          if (s < 0 || s + 1 >= cnt || (s_g[s] & PS_END_BIT)) {
            out = x[n];
          } else {
            if (s != cur) {
              cur = s;
              t0 = s_t[s];
              G = s_t[s + 1] - t0;
              A = s_a[s];
              B = s_a[s + 1];
              const int pr = s_pp[s] & 0xFFFF, pl = (int)((unsigned)s_pp[s + 1] >> 16);
              L = G < pr ? G : pr;
              L2 = G < pl ? G : pl;
              g0 = s_g[s] & 0xFFFF;
              g1 = s_g[s + 1] & 0xFFFF;
            }
            const int d = (int)n - t0, ee = G - d;
            const int wl = d < L ? PS_Q - (int)((unsigned)(d * PS_Q) / (unsigned)L) : 0;
            const int wr = ee < L2 ? (int)((unsigned)((L2 - ee) * PS_Q) / (unsigned)L2) : 0;
            const long ia = (long)A + d, ib = (long)B - ee;
            const int xa = ia >= 0 && ia < len ? x[ia] : 0;
            const int xb = ib >= 0 && ib < len ? x[ib] : 0;
            long acc = (long)(xa * wl) * g0 + (long)(xb * wr) * g1 + (1L << 29);
            acc >>= 30;
            if (acc > 32767 || acc < -32768) {
              clipped++;
              acc = acc > 32767 ? 32767 : -32768;
            }
            out = (int16_t)acc;
          }
        }
        piece.v[j] = out;
      }
      if (b == n0 && e == n0 + VS_PS_PER_LANE) {
        *reinterpret_cast<int4 *>(y + n0) = piece.q;
      } else {
#pragma unroll
        for (int j = 0; j < VS_PS_PER_LANE; j++)
          if (n0 + j >= b && n0 + j < e) y[n0 + j] = piece.v[j];
      }
    }
    pos = cov;
  }
  if (clipped) atomicAdd(&a.stat[row].n_clipped, clipped);
}

extern "C" hipError_t vs_launch_psola(const VsPsArgs *args, hipStream_t stream)
{
  if (args->n_lanes <= 0 || args->n_lanes > 0x7FFFFFFFL) return hipErrorInvalidValue;
  const long tiles = (args->n_samples + (VS_PS_PER_LANE - 1) + (VS_PS_TILE - 1)) / VS_PS_TILE;
  if (tiles <= 0 || tiles > 0x7FFFFFFFL / args->n_lanes) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vs_ps_plan_kernel, dim3((unsigned)((args->n_lanes + 63) / 64)), dim3(64), 0, stream, *args);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vs_ps_ola_kernel, dim3((unsigned)(tiles * args->n_lanes)), dim3(VS_PS_BLOCK), 0, stream, *args,
                     (unsigned)tiles);
  return hipGetLastError();
}
