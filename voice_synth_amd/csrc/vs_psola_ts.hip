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
 *   vs_pt_ola_kernel: ONE WORKGROUP PER (ROW, OUTPUT TILE), 256 lanes, a lane per 16-byte piece of the OUTPUT row: the
 *       overlap-add core of vs_psola_dev.h with the time map's switch -- two staged analysis marks a record, grains
 *       that may be read backwards, silence where no two records enclose a sample.  The input is read against len, the
 *       output written against len_out.
 *
 * The target, the governing-cycle lookup, the run check and the overlap-add core are vs_psola_dev.h's, shared with
 * vs_psola.hip; the walk over stretches and the map are this file's own.
 */
#include "vs_psola_ts.h"
#include "vs_psola_dev.h"

/* ---------------------------------------------------------------------------------------------------------------- */
/* plan                                                                                                              */

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
__device__ __forceinline__ void pt_walk(const PtStretch s, int ts, int te, PtMap &mp, const VsPsTarget &tg, int &p, PtOut &o)
{
  int t = ts, k = 0, bk = pt_b(s, 0), i = 0, flip = 0, kprev = -1;
  int prev = -1, sprev = 0, tprev = 0; /* the governing cycle of the mark before, its start and period */
  for (;;) {
    int c = -1, sc = 0, tc = 0, g = VS_PS_Q;
    if (s.voiced) c = vs_ps_govern(tg, t, p, prev, sprev, tprev, sc, tc, g);
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
      vs_psola_mark mk = {t, s.first + k, code, i == 0 ? VS_PS_Q : g};
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
  VsPsRuns runs;
  int len_out, U;
};

enum { PT_CHECK, PT_COUNT, PT_WRITE };

/* Step 1, and per stretch what MODE asks for.  PT_CHECK: the stretches are counted and `least` falls to the shortest
 * step one of them can take (a target period is at least pmin, which the caller puts there).  PT_COUNT and PT_WRITE:
 * step 2.  Returns the status bits of the runs; done: the usable runs. */
template <int MODE>
__device__ __forceinline__ int pt_row(const PtRow &r, PtMap mp, const VsPsTarget &tg, PtOut &o, int &done, int &least,
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
      const int32_t *ra = r.runs.marks + first;
      if (MODE == PT_CHECK)
        for (int j = 1; j < m; j++) {
          const int d = ra[j] - ra[j - 1];
          step = d < step ? d : step;
        }
      prev_end = g0 = ra[m - 1];
      done++;
      run_next = false;
    } else {
      bool ok = false; /* the next usable run */
      while (q < r.runs.n_runs && !ok) {
        ok = vs_ps_run(r.runs, q++, prev_end, first, m) != 0;
        if (!ok) status |= VS_PS_BAD_RUN;
      }
      run_next = ok;
      last = !ok;
      const int g1 = ok ? r.runs.marks[first] : r.runs.len;
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
    const PtStretch s = {voiced ? r.runs.marks + first : nullptr, sm, voiced ? first : 0, s0, s1, r.U, voiced};
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
  if (row >= a.c.n_lanes) return;
  PtRow r;
  r.runs = vs_ps_runs(a.c, row, a.rows[row].length);
  r.len_out = a.rows[row].len_out;
  r.U = a.unvoiced;
  const VsPsTarget tg = vs_ps_target(a.c, row);

  vs_psola_stat st;
  st.n_runs = r.runs.n_runs;
  st.n_runs_done = st.n_synth = st.n_governed = 0;
  st.n_clipped = 0; /* the overlap-add kernel adds */
  PtMap mp;
  mp.an = a.map + row * a.map_pitch;
  mp.W = a.map_count[row];
  mp.len = r.runs.len;
  mp.len_out = r.len_out;
  if (!pt_map_valid(mp.an, mp.W, a.map_pitch, r.runs.len, r.len_out)) {
    st.status = VS_PS_BAD_MAP | VS_PS_NO_RUN;
    a.c.stat[row] = st;
    return;
  }
  pt_piece(mp, 0);
  mp.jv = 0;

  PtOut o;
  o.rec = a.c.synth + row * a.c.synth_pitch;
  o.aux = a.aux + row * a.c.synth_pitch;
  o.slots = (int)a.c.synth_pitch;
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
      vs_psola_mark mk = {r.len_out, o.end_k, VS_PS_RUN_END, VS_PS_Q};
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
  a.c.stat[row] = st;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* overlap-add                                                                                                       */

/* one record into slot i of the staged marks (vs_psola_dev.h): two analysis marks a record, and the flip bit */
__device__ __forceinline__ void vs_ps_stage(const vs_psola_mark &mk, const VsPtAux &ax, int i, int *s_t, int *s_al,
                                            int *s_ar, int *s_pp, int *s_g)
{
  s_t[i] = mk.t;
  s_al[i] = ax.a_left;
  s_ar[i] = ax.a_right;
  s_pp[i] = ax.periods;
  s_g[i] = (mk.gain & 0xFFFF) | (mk.cycle == VS_PS_UNVOICED_FLIP ? VS_PS_MARK_BIT : 0);
}

__global__ __launch_bounds__(VS_PS_BLOCK) void vs_pt_ola_kernel(VsPtArgs a, unsigned tiles)
{
  __shared__ int s_t[VS_PS_STAGE], s_al[VS_PS_STAGE], s_ar[VS_PS_STAGE], s_pp[VS_PS_STAGE], s_g[VS_PS_STAGE];
  __shared__ int s_count[4];
  const VsPtRow r = a.rows[blockIdx.x / tiles];
  vs_ps_ola<true>(a.c, a.aux, tiles, r.length, r.len_out, s_t, s_al, s_ar, s_pp, s_g, s_count);
}

extern "C" hipError_t vs_launch_psola_ts(const VsPtArgs *args, hipStream_t stream)
{
  const long n_lanes = args->c.n_lanes;
  if (n_lanes <= 0 || n_lanes > 0x7FFFFFFFL) return hipErrorInvalidValue;
  const long tiles = (args->out_samples + (VS_PS_PER_LANE - 1) + (VS_PS_TILE - 1)) / VS_PS_TILE;
  if (tiles <= 0 || tiles > 0x7FFFFFFFL / n_lanes) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vs_pt_plan_kernel, dim3((unsigned)((n_lanes + 63) / 64)), dim3(64), 0, stream, *args);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vs_pt_ola_kernel, dim3((unsigned)(tiles * n_lanes)), dim3(VS_PS_BLOCK), 0, stream, *args,
                     (unsigned)tiles);
  return hipGetLastError();
}
