/*
 * vs_psola_ts.hip -- gfx950 kernels of PSOLA with a time map (include/voice_synth.h, "PSOLA with a time map"): the
 * cycles of an int16 row already on the device, placed at the instants a target of periods asks for, while a map from
 * output time to input time says which of them is due.
 *
 * Two kernels on the context's stream, one behind the other, shaped like those of vs_psola.hip:
 *
 *   vs_pt_plan_kernel: ONE LANE PER ROW, 64 rows per workgroup.  The row is walked as a chain of stretches: the gap in
 *       front of the next usable run, whose marks are made on the fly from (g0, g1, U), then the run.  A stretch is
 *       walked with O(1) state: the mark, its index, the governing cycle before, a cursor into the target, a cursor
 *       into the anchors for M (the synthesis instants increase) and one for Minv (the stretches' ends increase); none
 *       of them moves backwards.  The row's count must be known before a record is stored (a row that does not fit
 *       stores none), so a first pass over the runs finds the shortest step any stretch can take and bounds the count
 *       by len_out / step + stretches + 1; only a row whose bound exceeds synth_pitch is walked once to count.  Next to
 *       every vs_psola_mark goes a VsPtAux into the launch's scratch.
 *
 *   vs_pt_ola_kernel: ONE WORKGROUP PER (ROW, OUTPUT TILE), 256 lanes, a lane per 16-byte piece of the OUTPUT row.  The
 *       first synthesis mark of the tile by a 256-way section of the row's records, up to VS_PS_STAGE marks staged in
 *       LDS, several times when the tile holds more; a lane finds the interval of its first sample by bisection in LDS
 *       and steps on from there.  The input is read against len, the output written against len_out.  A piece that lies
 *       inside the row is stored as one dwordx4, the pieces at the row's ends sample by sample.
 *
 * Every index into the PCM is checked against the row (outside it a sample reads as 0), every record index against
 * n_synth and the pitch: a wrong record costs wrong samples, never an access outside the arrays.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_psola_ts.h"

#define PT_Q 32768
#define PT_FLIP_BIT 0x10000 /* in the staged gain word: the mark's grain is read backwards */

__device__ __forceinline__ int pt_ld(const char *base, long index, int stride)
{
  return *(const int32_t *)(base + index * (long)stride);
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* plan                                                                                                              */

struct PtTarget {
  const char *start, *period, *gain; /* of the row */
  int ss, ps, gs;
  int J, pmin, pmax;
};

/* a valid map and its two cursors */
struct PtMap {
  const vs_psola_anchor *an;
  int W, len, len_out;
  int jm, u0, v0, du, dv; /* M: the piece the last instant lay in */
  int jv;                 /* Minv: the first piece whose end reaches the last position */
};

__device__ __forceinline__ bool pt_map_valid(const vs_psola_anchor *an, int W, long map_pitch, int len, int len_out)
{
  if (W < 2 || (long)W > map_pitch) return false;
  vs_psola_anchor before = an[0];
  if (before.u != 0 || before.v != 0) return false;
  for (int j = 1; j < W; j++) {
    const vs_psola_anchor at = an[j];
    if (at.u <= before.u || at.v < before.v) return false;
    before = at;
  }
  return before.u == len_out && before.v == len;
}

__device__ __forceinline__ void pt_piece(PtMap &mp, int j)
{
  const vs_psola_anchor a0 = mp.an[j], a1 = mp.an[j + 1];
  mp.jm = j;
  mp.u0 = a0.u;
  mp.v0 = a0.v;
  mp.du = a1.u - a0.u;
  mp.dv = a1.v - a0.v;
}

/* M(n) for 0 <= n < len_out, n not below the n of the call before */
__device__ __forceinline__ int pt_M(PtMap &mp, int n)
{
  while (n >= mp.u0 + mp.du && mp.jm + 2 < mp.W) pt_piece(mp, mp.jm + 1);
  return mp.v0 + (int)(((long)(n - mp.u0) * (long)mp.dv) / (long)mp.du);
}

/* Minv(p), p not below the p of the call before: the first piece j with v_{j+1} >= p has v_j < p, and inside it the
 * smallest n with (n - u_j) * dv >= (p - v_j) * du */
__device__ __forceinline__ int pt_Minv(PtMap &mp, int p)
{
  if (p <= 0) return 0;
  if (p >= mp.len) return mp.len_out;
  while (mp.jv + 2 < mp.W && mp.an[mp.jv + 1].v < p) mp.jv++;
  const vs_psola_anchor a0 = mp.an[mp.jv], a1 = mp.an[mp.jv + 1];
  const long du = (long)a1.u - a0.u, dv = (long)a1.v - a0.v;
  if (dv <= 0) return a1.u; /* (cannot happen in a valid map) */
  return a0.u + (int)(((long)(p - a0.v) * du + dv - 1) / dv);
}

/* a stretch: the marks of a usable run, or the marks g0, g0 + U, .., g1 of a gap */
struct PtStretch {
  const int32_t *a; /* voiced: the run's marks */
  int m, first;     /* unvoiced: first = 0 */
  int g0, g1, U;
  bool voiced;
};

__device__ __forceinline__ int pt_b(const PtStretch s, int k)
{
  return s.voiced ? s.a[k] : k == s.m - 1 ? s.g1 : s.g0 + k * s.U;
}
__device__ __forceinline__ int pt_pr(const PtStretch s, int k)
{
  return k < s.m - 1 ? pt_b(s, k + 1) - pt_b(s, k) : pt_b(s, k) - pt_b(s, k - 1);
}
__device__ __forceinline__ int pt_pl(const PtStretch s, int k)
{
  return k > 0 ? pt_b(s, k) - pt_b(s, k - 1) : pt_b(s, 1) - pt_b(s, 0);
}

/* the records of a row so far, and what the end of the last stretch with marks leaves for the boundary */
struct PtOut {
  vs_psola_mark *rec;
  VsPtAux *aux;
  int slots, n, governed;
  bool have_end;
  int end_a, end_pl, end_pr, end_k;
};

/* Step 2 on one stretch with t_s < t_e: the records of all its marks but the last, which is the next stretch's first or
 * the row's last.  WRITE: they go to rec[] and aux[] (never past the slots); else they are counted, and the walk ends
 * once the row has more than the slots hold.  p: the target's cursor, as in vs_psola.hip. */
template <bool WRITE>
__device__ __forceinline__ void pt_walk(const PtStretch s, int ts, int te, PtMap &mp, const PtTarget &tg, int &p, PtOut &o)
{
  int t = ts, k = 0, bk = pt_b(s, 0), i = 0, flip = 0, kprev = -1;
  int prev = -1, sprev = 0, tprev = 0; /* the governing cycle of the mark before, its start and period */
  for (;;) {
    int c = -1, sc = 0, tc = 0, g = PT_Q;
    if (s.voiced) {
      if (prev >= 0 && prev + 1 < tg.J && (long)(sc = pt_ld(tg.start, prev + 1, tg.ss)) == (long)sprev + (long)tprev) {
        c = prev + 1;
        tc = pt_ld(tg.period, c, tg.ps);
      } else {
        while (p < tg.J && pt_ld(tg.start, p, tg.ss) <= t) p++;
        if (p > 0) {
          sc = pt_ld(tg.start, p - 1, tg.ss);
          tc = pt_ld(tg.period, p - 1, tg.ps);
          if ((long)t < (long)sc + (long)tc) c = p - 1;
        }
      }
      if (c >= 0) {
        if (tg.gain) g = pt_ld(tg.gain, c, tg.gs);
        if (tc < tg.pmin || tc > tg.pmax || g < 0 || g > 65535) c = -1;
      }
      if (c < 0) g = PT_Q;
    }
    const int pr = pt_pr(s, k);
    const int Ti = c >= 0 ? tc : pr;
    int code = c;
    if (!s.voiced) {
      flip = i > 0 && k == kprev ? !flip : 0;
      code = flip ? VS_PS_UNVOICED_FLIP : VS_PS_UNVOICED;
    }
    if (WRITE && o.n < o.slots) {
      int ar = bk, pl = pt_pl(s, k);
      if (i == 0 && o.have_end) { /* the boundary: the right grain is the end of the stretch before */
        ar = o.end_a;
        pl = o.end_pl;
      }
      vs_psola_mark mk = {t, s.first + k, code, i == 0 ? PT_Q : g};
      VsPtAux ax = {bk, ar, pr | (pl << 16)};
      o.rec[o.n] = mk;
      o.aux[o.n] = ax;
    }
    o.n++;
    o.governed += c >= 0;
    prev = c;
    sprev = sc;
    tprev = tc;
    kprev = k;
    i++;
    if (te - t <= Ti + Ti / 2) break;
    if (!WRITE && o.n > o.slots) break;
    t += Ti;
    /* the mark at or behind k that is nearest to M(t), ties to the smaller: the distances fall, then rise */
    const int at = pt_M(mp, t);
    while (k < s.m - 1) {
      const int nx = pt_b(s, k + 1);
      if (abs(nx - at) >= abs(bk - at)) break;
      bk = nx;
      k++;
    }
  }
  o.have_end = true;
  o.end_a = pt_b(s, s.m - 1);
  o.end_pl = pt_pl(s, s.m - 1);
  o.end_pr = pt_pr(s, s.m - 1);
  o.end_k = s.first + s.m - 1;
}

struct PtRow {
  const int32_t *marks;
  const vs_guided_seg *segs; /* NULL: one run */
  long marks_pitch;
  int n_runs, n_marks, len, len_out, U;
};

enum { PT_CHECK, PT_COUNT, PT_WRITE };

/* Step 1, and per stretch what MODE asks for.  PT_CHECK: the stretches are counted and `least` falls to the shortest
 * step one of them can take (a target period is at least pmin, which the caller puts there).  PT_COUNT and PT_WRITE:
 * step 2.  Returns the status bits of the runs; done: the usable runs. */
template <int MODE>
__device__ __forceinline__ int pt_row(const PtRow &r, PtMap mp, const PtTarget &tg, PtOut &o, int &done, int &least,
                                      int &n_stretches)
{
  int status = 0, q = 0, prev_end = -1, g0 = 0, p = 0, ts = 0;
  bool run_next = false, last = false;
  int first = 0, m = 0;
  done = 0;
  for (;;) {
    int step = 0x7FFFFFFF; /* PT_CHECK: the stretch's shortest analysis interval */
    int sm = m, s0 = 0, s1 = 0;
    const bool voiced = run_next;
    if (run_next) {
      const int32_t *ra = r.marks + first;
      if (MODE == PT_CHECK)
        for (int j = 1; j < m; j++) {
          const int d = ra[j] - ra[j - 1];
          step = d < step ? d : step;
        }
      prev_end = g0 = ra[m - 1];
      done++;
      run_next = false;
    } else {
      /* the next usable run: the ends first, then every step */
      bool ok = false;
      while (q < r.n_runs && !ok) {
        if (r.segs) {
          first = r.segs[q].first_mark_index;
          m = r.segs[q].n_marks;
        } else {
          first = 0;
          m = (long)r.n_marks > r.marks_pitch ? (int)r.marks_pitch : r.n_marks;
        }
        q++;
        ok = m >= 2 && first >= 0 && (long)first + (long)m <= r.marks_pitch;
        if (ok) {
          int before = r.marks[first];
          ok = before > prev_end && r.marks[first + m - 1] < r.len; /* (prev_end >= -1: the first mark is not negative) */
          for (int j = 1; j < m && ok; j++) {
            const int v = r.marks[first + j];
            const long d = (long)v - (long)before;
            ok = d > 0 && d <= VS_AC_MAX_LAG;
            before = v;
          }
        }
        if (!ok) status |= VS_PS_BAD_RUN;
      }
      run_next = ok;
      last = !ok;
      const int g1 = ok ? r.marks[first] : r.len;
      if (g1 <= g0) { /* no gap: a run that begins at 0, a row of length 0 */
        if (last) break;
        continue;
      }
      const int gap = g1 - g0, H = r.U + r.U / 2;
      s0 = g0;
      s1 = g1;
      sm = gap <= H ? 2 : (gap - H - 1) / r.U + 3; /* p_i for every i with gap - i*U > H, one more, and g1 */
      step = gap <= H ? gap : r.U / 2 + 1;
    }
    const PtStretch s = {voiced ? r.marks + first : nullptr, sm, voiced ? first : 0, s0, s1, r.U, voiced};
    if (MODE == PT_CHECK) {
      n_stretches++;
      least = step < least ? step : least;
    } else {
      const int te = pt_Minv(mp, pt_b(s, s.m - 1));
      if (te > ts) pt_walk<MODE == PT_WRITE>(s, ts, te, mp, tg, p, o);
      ts = te > ts ? te : ts;
      if (MODE == PT_COUNT && o.n > o.slots) break;
    }
    if (last) break;
  }
  return status;
}

__global__ __launch_bounds__(64) void vs_pt_plan_kernel(VsPtArgs a)
{
  const long row = (long)blockIdx.x * 64 + threadIdx.x;
  if (row >= a.n_lanes) return;
  const vs_guided_rec gr = a.rec[row];
  PtRow r;
  r.marks = a.marks + row * a.marks_pitch;
  r.segs = a.segs ? a.segs + row * a.seg_pitch : nullptr;
  r.marks_pitch = a.marks_pitch;
  r.n_marks = gr.n_marks;
  r.len = a.rows[row].length;
  r.len_out = a.rows[row].len_out;
  r.U = a.unvoiced;
  if (a.segs) r.n_runs = gr.n_segments < 0 ? 0 : (long)gr.n_segments > a.seg_pitch ? (int)a.seg_pitch : gr.n_segments;
  else r.n_runs = 1;

  PtTarget tg;
  const long t0 = row * a.target_pitch;
  tg.start = a.start + t0 * a.start_stride;
  tg.period = a.period + t0 * a.period_stride;
  tg.gain = a.gain ? a.gain + t0 * a.gain_stride : nullptr;
  tg.ss = a.start_stride;
  tg.ps = a.period_stride;
  tg.gs = a.gain_stride;
  const int count = pt_ld(a.count, row, a.count_stride);
  tg.J = count < 0 ? 0 : (long)count > a.target_pitch ? (int)a.target_pitch : count;
  tg.pmin = a.pmin;
  tg.pmax = a.pmax;

  vs_psola_stat st;
  st.n_runs = r.n_runs;
  st.n_runs_done = st.n_synth = st.n_governed = 0;
  st.n_clipped = 0; /* the overlap-add kernel adds */
  PtMap mp;
  mp.an = a.map + row * a.map_pitch;
  mp.W = a.map_count[row];
  mp.len = r.len;
  mp.len_out = r.len_out;
  if (!pt_map_valid(mp.an, mp.W, a.map_pitch, r.len, r.len_out)) {
    st.status = VS_PS_BAD_MAP | VS_PS_NO_RUN;
    a.stat[row] = st;
    return;
  }
  pt_piece(mp, 0);
  mp.jv = 0;

  PtOut o;
  o.rec = a.synth + row * a.synth_pitch;
  o.aux = a.aux + row * a.synth_pitch;
  o.slots = (int)a.synth_pitch;
  o.n = o.governed = 0;
  o.have_end = false;
  o.end_a = o.end_pl = o.end_pr = o.end_k = 0;

  int done = 0, least = tg.pmin, n_stretches = 0;
  int status = pt_row<PT_CHECK>(r, mp, tg, o, done, least, n_stretches);
  bool fits = (long)(r.len_out / least) + n_stretches + 1 <= (long)o.slots;
  int again = 0; /* (the later passes see the runs the first one saw: its status and count stand) */
  if (!fits) {
    PtOut oc = o;
    pt_row<PT_COUNT>(r, mp, tg, oc, again, least, n_stretches);
    fits = oc.n + (oc.have_end ? 1 : 0) <= o.slots;
  }
  if (fits) {
    pt_row<PT_WRITE>(r, mp, tg, o, again, least, n_stretches);
    if (o.have_end && o.n < o.slots) { /* the row's last record */
      vs_psola_mark mk = {r.len_out, o.end_k, VS_PS_RUN_END, PT_Q};
      VsPtAux ax = {o.end_a, o.end_a, o.end_pr | (o.end_pl << 16)};
      o.rec[o.n] = mk;
      o.aux[o.n] = ax;
      o.n++;
    }
    st.n_synth = o.n;
    st.n_governed = o.governed;
  } else {
    status |= VS_PS_OVERFLOW;
  }
  st.status = status | (done == 0 ? VS_PS_NO_RUN : 0);
  st.n_runs_done = done;
  a.stat[row] = st;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* overlap-add                                                                                                       */

__global__ __launch_bounds__(VS_PS_BLOCK) void vs_pt_ola_kernel(VsPtArgs a, unsigned tiles)
{
  __shared__ int s_t[VS_PS_STAGE], s_al[VS_PS_STAGE], s_ar[VS_PS_STAGE], s_pp[VS_PS_STAGE], s_g[VS_PS_STAGE];
  __shared__ int s_count[4];
  const long row = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  const int tid = threadIdx.x;
  const int len = a.rows[row].length;
  const int len_out = a.rows[row].len_out;
  const int16_t *x = a.pcm + row * a.pitch;
  int16_t *y = a.out + row * a.out_pitch;
  const int mis = (int)(((uintptr_t)y >> 1) & (VS_PS_PER_LANE - 1));
  const long tile0 = (long)tile * VS_PS_TILE - mis; /* y + tile0 is a 16-byte address */
  const long lo_n = tile0 < 0 ? 0 : tile0;
  const long hi_n = tile0 + VS_PS_TILE < (long)len_out ? tile0 + VS_PS_TILE : (long)len_out;
  if (lo_n >= hi_n) return; /* (the whole workgroup) */
  int ns = a.stat[row].n_synth;
  ns = ns < 0 ? 0 : (long)ns > a.synth_pitch ? (int)a.synth_pitch : ns;
  const vs_psola_mark *rec = a.synth + row * a.synth_pitch;
  const VsPtAux *aux = a.aux + row * a.synth_pitch;
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
      const VsPtAux ax = aux[first + tid];
      s_t[tid] = mk.t;
      s_al[tid] = ax.a_left;
      s_ar[tid] = ax.a_right;
      s_pp[tid] = ax.periods;
      s_g[tid] = (mk.gain & 0xFFFF) | (mk.cycle == VS_PS_UNVOICED_FLIP ? PT_FLIP_BIT : 0);
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
          if (s >= 0 && s + 1 < cnt) { /* (a row without records is silence) */
            if (s != cur) {
              cur = s;
              t0 = s_t[s];
              G = s_t[s + 1] - t0;
              A = s_al[s];
              B = s_ar[s + 1];
              const int pr = s_pp[s] & 0xFFFF, pl = (int)((unsigned)s_pp[s + 1] >> 16);
              L = G < pr ? G : pr;
              L2 = G < pl ? G : pl;
              L = L < 1 ? 1 : L;
              L2 = L2 < 1 ? 1 : L2;
              g0 = s_g[s] & 0xFFFF;
              g1 = s_g[s + 1] & 0xFFFF;
              sa = (s_g[s] & PT_FLIP_BIT) ? -1 : 1;     /* a flipped left grain reads x[A - d] */
              sb = (s_g[s + 1] & PT_FLIP_BIT) ? 1 : -1; /* a flipped right grain reads x[B + e] */
            }
            const int d = (int)n - t0, ee = G - d;
            const int wl = d < L ? PT_Q - (int)((unsigned)(d * PT_Q) / (unsigned)L) : 0;
            const int wr = ee < L2 ? (int)((unsigned)((L2 - ee) * PT_Q) / (unsigned)L2) : 0;
            const long ia = (long)A + sa * d, ib = (long)B + sb * ee;
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

extern "C" hipError_t vs_launch_psola_ts(const VsPtArgs *args, hipStream_t stream)
{
  if (args->n_lanes <= 0 || args->n_lanes > 0x7FFFFFFFL) return hipErrorInvalidValue;
  const long tiles = (args->out_samples + (VS_PS_PER_LANE - 1) + (VS_PS_TILE - 1)) / VS_PS_TILE;
  if (tiles <= 0 || tiles > 0x7FFFFFFFL / args->n_lanes) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vs_pt_plan_kernel, dim3((unsigned)((args->n_lanes + 63) / 64)), dim3(64), 0, stream, *args);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vs_pt_ola_kernel, dim3((unsigned)(tiles * args->n_lanes)), dim3(VS_PS_BLOCK), 0, stream, *args,
                     (unsigned)tiles);
  return hipGetLastError();
}
