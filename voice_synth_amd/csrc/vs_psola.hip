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
 *   vs_ps_ola_kernel: ONE WORKGROUP PER (ROW, TILE), 256 lanes, a lane per 16-byte piece of the OUTPUT row: the
 *       overlap-add core of vs_psola_dev.h without the time map's switch.  Copy regions -- in front of a run, behind
 *       it, rows without a run -- go through the same code.
 *
 * The target, the governing-cycle lookup, the run check and the overlap-add core are vs_psola_dev.h's, shared with
 * vs_psola_ts.hip; the walk is this file's own.
 */
#include "vs_psola_dev.h"

/* ---------------------------------------------------------------------------------------------------------------- */
/* plan                                                                                                              */

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
__device__ int ps_walk(const PsRun &r, const VsPsTarget &tg, int &p, int room, vs_psola_mark *rec, VsPsAux *aux, int &governed)
{
  const int E = r.a[r.m - 1];
  int t = r.a[0], k = 0, ak = t, n = 0, gov = 0;
  int prev = -1, sprev = 0, tprev = 0; /* the governing cycle of the mark before, its start and period */
  for (;;) {
    int sc, tc, g;
    const int c = vs_ps_govern(tg, t, p, prev, sprev, tprev, sc, tc, g);
    const int pr = ps_pr(r, k);
    const int Ti = c >= 0 ? tc : pr;
    if (WRITE) {
      vs_psola_mark mk = {t, r.first + k, c, n == 0 ? VS_PS_Q : g};
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
        vs_psola_mark mk = {E, r.first + r.m - 1, VS_PS_RUN_END, VS_PS_Q};
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
  if (row >= a.c.n_lanes) return;
  const VsPsRuns runs = vs_ps_runs(a.c, row, a.rows[row].length);
  vs_psola_mark *rec = a.c.synth + row * a.c.synth_pitch;
  VsPsAux *aux = a.aux + row * a.c.synth_pitch;
  const int slots = (int)a.c.synth_pitch;
  const VsPsTarget tg = vs_ps_target(a.c, row);

  int status = 0, done = 0, n_synth = 0, governed = 0;
  int prev_end = -1, p = 0;
  for (int q = 0; q < runs.n_runs; q++) {
    int first, m;
    const int shortest = vs_ps_run(runs, q, prev_end, first, m);
    if (!shortest) {
      status |= VS_PS_BAD_RUN;
      continue;
    }
    PsRun r = {runs.marks + first, m, first};
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
  st.n_runs = runs.n_runs;
  st.n_runs_done = done;
  st.n_synth = n_synth;
  st.n_governed = governed;
  st.n_clipped = 0; /* the overlap-add kernel adds */
  a.c.stat[row] = st;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* overlap-add                                                                                                       */

__global__ __launch_bounds__(VS_PS_BLOCK) void vs_ps_ola_kernel(VsPsArgs a, unsigned tiles)
{
  __shared__ int s_t[VS_PS_STAGE], s_a[VS_PS_STAGE], s_pp[VS_PS_STAGE], s_g[VS_PS_STAGE];
  __shared__ int s_count[4];
  const int len = a.rows[blockIdx.x / tiles].length;
  vs_ps_ola<false>(a.c, a.aux, tiles, len, len, s_t, s_a, s_a, s_pp, s_g, s_count);
}

extern "C" hipError_t vs_launch_psola(const VsPsArgs *args, hipStream_t stream)
{
  const long n_lanes = args->c.n_lanes;
  if (n_lanes <= 0 || n_lanes > 0x7FFFFFFFL) return hipErrorInvalidValue;
  const long tiles = (args->n_samples + (VS_PS_PER_LANE - 1) + (VS_PS_TILE - 1)) / VS_PS_TILE;
  if (tiles <= 0 || tiles > 0x7FFFFFFFL / n_lanes) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vs_ps_plan_kernel, dim3((unsigned)((n_lanes + 63) / 64)), dim3(64), 0, stream, *args);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vs_ps_ola_kernel, dim3((unsigned)(tiles * n_lanes)), dim3(VS_PS_BLOCK), 0, stream, *args,
                     (unsigned)tiles);
  return hipGetLastError();
}
