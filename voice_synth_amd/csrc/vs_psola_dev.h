/*
 * vs_psola_dev.h -- the device code that the kernels of PSOLA (vs_psola.hip) and of PSOLA with a time map
 * (vs_psola_ts.hip) share: the target of a row and the lookup of the cycle that governs an instant, the runs of a row
 * and the check that makes one usable, and the overlap-add core, which each file's kernel instantiates with its own
 * switch and its own LDS.
 *
 * Every index into the PCM is checked against the row (outside it a sample reads as 0), every record index against
 * n_synth and the pitch: a wrong record costs wrong samples, never an access outside the arrays.
 */
#ifndef VS_PSOLA_DEV_H
#define VS_PSOLA_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_psola.h"

#define VS_PS_Q 32768 /* a gain or a weight of 1 */
/* Bit 16 of the staged gain word (the gain itself is 0..65535).  In vs_ps_ola<false> it says that the mark is a run's
 * last: what lies behind it is copied.  In vs_ps_ola<true> it says that the mark's grain is read backwards. */
#define VS_PS_MARK_BIT 0x10000

__device__ __forceinline__ int vs_ps_ld(const char *base, long index, int stride)
{
  return *(const int32_t *)(base + index * (long)stride);
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* plan                                                                                                              */

struct VsPsTarget {
  const char *start, *period, *gain; /* of the row */
  int ss, ps, gs;
  int J, pmin, pmax;
};

__device__ __forceinline__ VsPsTarget vs_ps_target(const VsPsCommon &c, long row)
{
  VsPsTarget tg;
  const long t0 = row * c.target_pitch;
  tg.start = c.start + t0 * c.start_stride;
  tg.period = c.period + t0 * c.period_stride;
  tg.gain = c.gain ? c.gain + t0 * c.gain_stride : nullptr;
  tg.ss = c.start_stride;
  tg.ps = c.period_stride;
  tg.gs = c.gain_stride;
  const int count = vs_ps_ld(c.count, row, c.count_stride);
  tg.J = count < 0 ? 0 : (long)count > c.target_pitch ? (int)c.target_pitch : count;
  tg.pmin = c.pmin;
  tg.pmax = c.pmax;
  return tg;
}

/* The cycle that governs the instant t, or -1.  prev: the governing cycle of the mark before (-1: none), sprev and
 * tprev its start and period: the cycle behind it is tried first, if it begins where that one ends.  Else p, the
 * target's cursor, moves on to the first index whose start lies above t (J: none); it never moves backwards.  A cycle
 * whose period or gain is out of range governs nothing.  sc, tc: the start and period that were read; g: the cycle's
 * gain, VS_PS_Q without one. */
__device__ __forceinline__ int vs_ps_govern(const VsPsTarget &tg, int t, int &p, int prev, int sprev, int tprev, int &sc,
                                            int &tc, int &g)
{
  int c = -1;
  sc = tc = 0;
  if (prev >= 0 && prev + 1 < tg.J && (long)(sc = vs_ps_ld(tg.start, prev + 1, tg.ss)) == (long)sprev + (long)tprev) {
    c = prev + 1;
    tc = vs_ps_ld(tg.period, c, tg.ps);
  } else {
    while (p < tg.J && vs_ps_ld(tg.start, p, tg.ss) <= t) p++;
    if (p > 0) {
      sc = vs_ps_ld(tg.start, p - 1, tg.ss);
      tc = vs_ps_ld(tg.period, p - 1, tg.ps);
      if ((long)t < (long)sc + (long)tc) c = p - 1;
    }
  }
  g = VS_PS_Q;
  if (c >= 0) {
    if (tg.gain) g = vs_ps_ld(tg.gain, c, tg.gs);
    if (tc < tg.pmin || tc > tg.pmax || g < 0 || g > 65535) {
      c = -1;
      g = VS_PS_Q;
    }
  }
  return c;
}

/* the marks of a row and the runs they fall into */
struct VsPsRuns {
  const int32_t *marks;
  const vs_guided_seg *segs; /* NULL: one run */
  long marks_pitch;
  int n_runs, n_marks, len;
};

__device__ __forceinline__ VsPsRuns vs_ps_runs(const VsPsCommon &c, long row, int len)
{
  const vs_guided_rec gr = c.rec[row];
  VsPsRuns r;
  r.marks = c.marks + row * c.marks_pitch;
  r.segs = c.segs ? c.segs + row * c.seg_pitch : nullptr;
  r.marks_pitch = c.marks_pitch;
  r.n_marks = gr.n_marks;
  r.len = len;
  if (c.segs) r.n_runs = gr.n_segments < 0 ? 0 : (long)gr.n_segments > c.seg_pitch ? (int)c.seg_pitch : gr.n_segments;
  else r.n_runs = 1;
  return r;
}

/* Run q of the row: its first mark's index and its number of marks.  Usable?  The ends first -- inside the marks,
 * behind prev_end, the end of the usable run before (-1: none; the first mark is not negative), in front of the row's
 * end --, then every step against VS_AC_MAX_LAG.  Returns the run's shortest step, for whoever wants it in the same
 * pass (PSOLA's plan kernel; the time map's pt_row only asks whether it is 0 and finds its own step in PT_CHECK);
 * 0: the run is not usable -- a usable run has two marks at least and every step above 0. */
__device__ __forceinline__ int vs_ps_run(const VsPsRuns &r, int q, int prev_end, int &first, int &m)
{
  if (r.segs) {
    first = r.segs[q].first_mark_index;
    m = r.segs[q].n_marks;
  } else {
    first = 0;
    m = (long)r.n_marks > r.marks_pitch ? (int)r.marks_pitch : r.n_marks;
  }
  bool ok = m >= 2 && first >= 0 && (long)first + (long)m <= r.marks_pitch;
  int shortest = 0x7FFFFFFF;
  if (ok) {
    int before = r.marks[first];
    ok = before > prev_end && r.marks[first + m - 1] < r.len;
    for (int j = 1; j < m && ok; j++) {
      const int v = r.marks[first + j];
      const long step = (long)v - (long)before;
      ok = step > 0 && step <= VS_AC_MAX_LAG;
      shortest = step < shortest ? (int)step : shortest;
      before = v;
    }
  }
  return ok ? shortest : 0;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* overlap-add                                                                                                       */

/* One record into slot i of the staged marks, an overload on the scratch record's type.  PSOLA has one analysis mark a
 * record, left and right grain alike; the overload for VsPtAux is vs_psola_ts.hip's, declared in front of its kernel. */
__device__ __forceinline__ void vs_ps_stage(const vs_psola_mark &mk, const VsPsAux &ax, int i, int *s_t, int *s_al,
                                            int *s_ar, int *s_pp, int *s_g)
{
  s_t[i] = mk.t;
  s_al[i] = ax.a; /* (s_ar is s_al) */
  s_pp[i] = ax.periods;
  s_g[i] = (mk.gain & 0xFFFF) | (mk.cycle == VS_PS_RUN_END ? VS_PS_MARK_BIT : 0);
}
/* ONE WORKGROUP PER (ROW, TILE) of VS_PS_BLOCK lanes, a lane per 16-byte piece of the OUTPUT row (VS_PS_PER_LANE
 * samples; the tiles are cut at the row's 16-byte addresses, vs_psola.h).  The workgroup finds the first synthesis mark
 * of its tile by a 256-way section of the row's records (every lane reads one record, a barrier counts the lanes at or
 * below the tile's first sample, the stretch between two probes is searched next: two rounds for 65536 records), stages
 * up to VS_PS_STAGE marks in LDS and, when the tile holds more, goes on from the last one staged.  A lane finds the
 * interval of its first sample by bisection in LDS and steps on from there.  A piece that lies inside the row is stored
 * as one dwordx4, the pieces at the row's ends sample by sample.
 *
 * The input is read against len, the output written against len_out (PSOLA: the same).  TS = false, PSOLA: a sample
 * that no two records enclose, or that lies behind a run's last record, is x[n]; s_ar is s_al.  TS = true, the time
 * map: such a sample is 0, a grain may be read backwards, and L and L2 are at least 1 (a boundary record may carry the
 * periods of a stretch that is not its own).  The LDS is the calling kernel's: VS_PS_STAGE ints each, s_count 4. */
template <bool TS, typename Aux>
__device__ __forceinline__ void vs_ps_ola(const VsPsCommon &c, const Aux *aux_all, unsigned tiles, int len, int len_out,
                                          int *s_t, int *s_al, int *s_ar, int *s_pp, int *s_g, int *s_count)
{
  const long row = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  const int tid = threadIdx.x;
  const int16_t *x = c.pcm + row * c.pitch;
  int16_t *y = c.out + row * c.out_pitch;
  const int mis = (int)(((uintptr_t)y >> 1) & (VS_PS_PER_LANE - 1));
  const long tile0 = (long)tile * VS_PS_TILE - mis; /* y + tile0 is a 16-byte address */
  const long lo_n = tile0 < 0 ? 0 : tile0;
  const long hi_n = tile0 + VS_PS_TILE < (long)len_out ? tile0 + VS_PS_TILE : (long)len_out;
  if (lo_n >= hi_n) return; /* (the whole workgroup) */
  int ns = c.stat[row].n_synth;
  ns = ns < 0 ? 0 : (long)ns > c.synth_pitch ? (int)c.synth_pitch : ns;
  const vs_psola_mark *rec = c.synth + row * c.synth_pitch;
  const Aux *aux = aux_all + row * c.synth_pitch;
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
    if (tid < cnt) vs_ps_stage(rec[first + tid], aux[first + tid], tid, s_t, s_al, s_ar, s_pp, s_g);
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
      int cur = -2, t0 = 0, G = 0, A = 0, B = 0, L = 1, L2 = 1, g0 = 0, g1 = 0, sa = 1, sb = -1;
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
          if (s < 0 || s + 1 >= cnt || (!TS && (s_g[s] & VS_PS_MARK_BIT))) {
            if (!TS) out = x[n]; /* (the time map: a row without records is silence) */
          } else {
            if (s != cur) {
              cur = s;
              t0 = s_t[s];
              G = s_t[s + 1] - t0;
              A = s_al[s];
              B = s_ar[s + 1];
              const int pr = s_pp[s] & 0xFFFF, pl = (int)((unsigned)s_pp[s + 1] >> 16);
              L = G < pr ? G : pr;
              L2 = G < pl ? G : pl;
              g0 = s_g[s] & 0xFFFF;
              g1 = s_g[s + 1] & 0xFFFF;
              if (TS) {
                L = L < 1 ? 1 : L;
                L2 = L2 < 1 ? 1 : L2;
                sa = (s_g[s] & VS_PS_MARK_BIT) ? -1 : 1;     /* a flipped left grain reads x[A - d] */
                sb = (s_g[s + 1] & VS_PS_MARK_BIT) ? 1 : -1; /* a flipped right grain reads x[B + e] */
              }
            }
            const int d = (int)n - t0, ee = G - d;
            const int wl = d < L ? VS_PS_Q - (int)((unsigned)(d * VS_PS_Q) / (unsigned)L) : 0;
            const int wr = ee < L2 ? (int)((unsigned)((L2 - ee) * VS_PS_Q) / (unsigned)L2) : 0;
            const long ia = TS ? (long)A + sa * d : (long)A + d, ib = TS ? (long)B + sb * ee : (long)B - ee;
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
  if (clipped) atomicAdd(&c.stat[row].n_clipped, clipped);
}

#endif
