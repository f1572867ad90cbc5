/*
 * vs_glottal.hip -- gfx950 kernel of the glottal parameters (include/voice_synth.h, "glottal parameters"): OQ, ClQ, SQ,
 * QOQ and NAQ of every cycle between the marks vs_ac_marks_kernel left on the device.
 *
 *   vs_glottal_kernel: ONE WAVEFRONT (one workgroup of 64 threads) PER ROW, its cycles in ascending order, so that the
 *       ordered sums of the row record need no reduction: lanes 0..4 carry one of the five each (one division per cycle
 *       for all five quotients) and write it.  The 64 lanes work on the samples of a cycle together, 64 consecutive
 *       samples at a time:
 *         - the M marks are checked as a whole, 64 at a time, before any sample is touched;
 *         - the samples [m_{c-1}, m_{c+1}) of cycle c lie in a ring of VS_GL_RING int16 in LDS.  The ring is filled
 *           ahead, up to m_{c-1} + VS_GL_RING, whenever a cycle reaches past what it holds (consecutive lanes load
 *           consecutive samples): every sample of a row comes from memory once, and the latency of that round of loads
 *           is paid once per ring, not once per cycle;
 *         - the trough is a per-lane minimum over (value, index) keys and one wave reduction that keeps the first
 *           index;
 *         - the crossings are __ballot masks of "not above the level" per chunk: chunks walk DOWN from the peak and the
 *           highest set bit gives the largest n (open), chunks walk UP from the peak and the lowest set bit gives the
 *           smallest n (close); both levels ride in the same pass (a crossing at q_o is one at q_h);
 *         - the steepest descent is a maximum over (difference, -index) keys, the first n on ties.
 *       A span beyond the ring (marks that are not vs_measure's: its periods stay within VS_AC_MAX_LAG) is read from
 *       the row in memory instead, by the same scans compiled a second time; every loop is bounded by marks that passed
 *       the check.
 *
 * Per-row and per-cycle status go into the records; there is no device trap.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_glottal.h"

#define VS_GL_RING (2 * VS_AC_MAX_LAG) /* samples: two periods of the measurement at their longest */

__shared__ int16_t gl_ring[VS_GL_RING]; /* sample n of the wavefront's row at gl_ring[n % VS_GL_RING], sign unchanged */

/* Wave reductions of 64-bit keys, the same in every lane afterwards, with all 64 lanes active.  Rows of 16 lanes reduce
 * by rotation within the row (DPP row_ror:1,2,4,8 -- every lane has a source, so there is no lane to mask), the four
 * rows through four pairs of v_readlane: a fraction of the latency of six rounds of ds_bpermute. */
template <int ROR> __device__ __forceinline__ long long gl_row_ror(long long v)
{
  const int lo = __builtin_amdgcn_update_dpp(0, (int)v, 0x120 + ROR, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(v >> 32), 0x120 + ROR, 0xF, 0xF, false);
  return ((long long)hi << 32) | (long long)(unsigned)lo;
}
__device__ __forceinline__ long long gl_row_of(long long v, int lane)
{
  const int lo = __builtin_amdgcn_readlane((int)v, lane), hi = __builtin_amdgcn_readlane((int)(v >> 32), lane);
  return ((long long)hi << 32) | (long long)(unsigned)lo;
}
__device__ __forceinline__ long long gl_min(long long a, long long b) { return b < a ? b : a; }
__device__ __forceinline__ long long gl_max(long long a, long long b) { return b > a ? b : a; }
__device__ __forceinline__ long long gl_wave_min(long long v)
{
  v = gl_min(v, gl_row_ror<1>(v));
  v = gl_min(v, gl_row_ror<2>(v));
  v = gl_min(v, gl_row_ror<4>(v));
  v = gl_min(v, gl_row_ror<8>(v));
  return gl_min(gl_min(gl_row_of(v, 0), gl_row_of(v, 16)), gl_min(gl_row_of(v, 32), gl_row_of(v, 48)));
}
__device__ __forceinline__ long long gl_wave_max(long long v)
{
  v = gl_max(v, gl_row_ror<1>(v));
  v = gl_max(v, gl_row_ror<2>(v));
  v = gl_max(v, gl_row_ror<4>(v));
  v = gl_max(v, gl_row_ror<8>(v));
  return gl_max(gl_max(gl_row_of(v, 0), gl_row_of(v, 16)), gl_max(gl_row_of(v, 32), gl_row_of(v, 48)));
}
/* a value every lane holds alike, where the compiler can see it */
__device__ __forceinline__ int gl_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ void gl_record_empty(vs_glottal_rec *o, int status)
{
  const double nan = __builtin_nan("");
  o->oq = nan;
  o->clq = nan;
  o->sq = nan;
  o->qoq = nan;
  o->naq = nan;
  o->n_cycles = 0;
  o->n_rejected = 0;
  o->status = status;
  o->reserved_ = 0;
}

struct GlCycle { /* step 2 of one cycle, the same in every lane */
  int lo, amp, open_o, open_h, close_o, close_h, gci, decl, status;
};

/* The scans of the cycle around the peak m1 between the marks m0 and m2 (0 <= m0 < m1 < m2 <= n_samples - 1), compiled
 * once for samples in the ring (RING: LDS reads; the ring holds [m0, m2)) and once for the row x in memory: a source
 * chosen per read would make every read a flat load.  y[n] = p * sample n. */
template <bool RING>
__device__ __forceinline__ GlCycle gl_scan(const int16_t *x, int p, int lane, int m0, int m1, int m2, int qo, int qh)
{
  auto Y = [&](int n) -> int {
    if constexpr (RING) return p * (int)gl_ring[n & (VS_GL_RING - 1)];
    else return p * (int)x[n];
  };
  GlCycle r = {0, 0, -1, -1, -1, -1, -1, 0, 0};

  /* the trough: first index of the minimum over [m0, m1) */
  long long key = 0x7FFFFFFFFFFFFFFFLL;
  for (int n = m0 + lane; n < m1; n += 64) {
    const long long k = ((long long)(Y(n) + 32768) << 32) | (long long)n;
    key = k < key ? k : key;
  }
  key = gl_wave_min(key);
  r.lo = gl_uniform((int)(key & 0xFFFFFFFFLL));
  const int b = gl_uniform((int)(key >> 32)) - 32768;
  r.amp = gl_uniform(Y(m1)) - b;
  if (r.amp <= 0) {
    r.status = VS_GLC_ZERO_AMPLITUDE;
    return r;
  }
  const int tho = qo * r.amp, thh = qh * r.amp; /* below 2^24, and so is 256*(y - b) */
  /* close: chunks upwards from m1 + 1, the lowest set bit */
  for (int s = m1 + 1; s < m2; s += 64) {
    const int n = s + lane;
    const bool valid = n < m2;
    const int v = valid ? 256 * (Y(n) - b) : 0;
    const unsigned long long mo = __ballot(valid && v <= tho), mh = __ballot(valid && v <= thh);
    if (r.close_h < 0 && mh) r.close_h = s + (int)__builtin_ctzll(mh);
    if (mo) {
      r.close_o = s + (int)__builtin_ctzll(mo);
      break;
    }
  }
  if (r.close_o < 0) {
    r.status = VS_GLC_NO_CLOSURE;
    r.close_h = -1;
    return r;
  }
  /* open: chunks downwards from m1, the highest set bit; lo itself is not above, so the chunk that holds it ends the
   * walk */
  for (int e = m1; e > r.lo; e -= 64) {
    const int n = e - 64 + lane;
    const bool valid = n >= r.lo;
    const int v = valid ? 256 * (Y(n) - b) : 0;
    const unsigned long long mo = __ballot(valid && v <= tho), mh = __ballot(valid && v <= thh);
    if (r.open_h < 0 && mh) r.open_h = e - (int)__builtin_clzll(mh);
    if (mo) {
      r.open_o = e - (int)__builtin_clzll(mo);
      break;
    }
  }
  /* the steepest descent over [m1, close_o): n + 1 <= close_o < m2 */
  long long dk = -1;
  for (int n = m1 + lane; n < r.close_o; n += 64) {
    const long long k = ((long long)(Y(n) - Y(n + 1) + 65536) << 32) | (long long)(0x7FFFFFFF - n);
    dk = k > dk ? k : dk;
  }
  dk = gl_wave_max(dk);
  r.decl = gl_uniform((int)(dk >> 32)) - 65536;
  r.gci = 0x7FFFFFFF - gl_uniform((int)(dk & 0xFFFFFFFFLL)) + 1;
  return r;
}

__global__ __launch_bounds__(64) void vs_glottal_kernel(VsGlArgs a)
{
  const int lane = threadIdx.x;
  const long row = blockIdx.x;
  vs_glottal_rec *o = a.out + row;
  const int K = a.meas[row].n_periods, ac_status = a.meas[row].status;
  const int32_t *mk = a.marks + row * a.marks_pitch;

  /* 1. the marks, before any sample */
  int empty = 0, M = 0;
  if (ac_status & (VS_AC_TOO_SHORT | VS_AC_UNVOICED)) {
    empty = VS_GL_NO_CYCLES;
  } else if (K < 0) {
    empty = VS_GL_BAD_MARKS;
  } else {
    M = K < a.marks_pitch ? K + 1 : a.marks_pitch;
    if (M < 3) empty = VS_GL_NO_CYCLES;
  }
  if (!empty) {
    int bad = 0;
    for (int j0 = 0; j0 < M; j0 += 64) { /* (M <= marks_pitch < 2^31 - 256) */
      const int j = j0 + lane;
      if (j < M) {
        const int m = mk[j];
        const int next = j + 1 < M ? mk[j + 1] : a.n_samples; /* m_j < m_{j+1}, m_{M-1} < n_samples */
        bad |= (m < 0) | (m >= next);
      }
    }
    if (__any(bad)) empty = VS_GL_BAD_MARKS;
  }
  if (empty) {
    if (lane == 0) gl_record_empty(o, empty);
    return;
  }

  const int16_t *x = a.pcm + row * a.pitch;
  const int p = a.polarity, qo = a.level_open, qh = a.level_mid;
  double sum = 0.0; /* lane 0: of OQ, 1: ClQ, 2: SQ, 3: QOQ, 4: NAQ */
  int n_acc = 0, n_rej = 0;
  int vlo = 0, vhi = 0;       /* the ring holds the row's samples [vlo, vhi) */
  const int last = mk[M - 1]; /* no cycle reads a sample at or beyond the last mark */
  int mbase = 0;              /* 64 marks in registers: lane l holds m_{mbase + l} */
  int mreg = lane < M ? mk[lane] : 0;
  int m0 = __builtin_amdgcn_readlane(mreg, 0), m1 = __builtin_amdgcn_readlane(mreg, 1);

  for (int c = 1; c <= M - 2; c++) {
    if (c + 1 - mbase >= 64) {
      mbase += 64;
      mreg = mbase + lane < M ? mk[mbase + lane] : 0;
    }
    const int m2 = __builtin_amdgcn_readlane(mreg, c + 1 - mbase);

    /* the samples [m0, m2): in the ring if they fit.  The ring holds [vlo, vhi); when the cycle reaches past vhi it is
     * filled as far ahead as it can be with m0 still in it, which serves a few dozen cycles of ordinary periods with
     * one round of loads */
    const bool in_lds = m2 - m0 <= VS_GL_RING;
    if (in_lds && !(vlo <= m0 && m2 <= vhi)) {
      const int upto = m0 + VS_GL_RING < last ? m0 + VS_GL_RING : last; /* >= m2 */
      const bool extend = vlo <= m0 && m0 <= vhi;
      __syncthreads();
      for (int n = (extend ? vhi : m0) + lane; n < upto; n += 64) gl_ring[n & (VS_GL_RING - 1)] = x[n];
      __syncthreads();
      vlo = extend && vlo > upto - VS_GL_RING ? vlo : (extend ? upto - VS_GL_RING : m0);
      vhi = upto;
    }

    /* 2. the cycle */
    const GlCycle r = in_lds ? gl_scan<true>(x, p, lane, m0, m1, m2, qo, qh)
                             : gl_scan<false>(x, p, lane, m0, m1, m2, qo, qh);
    const int T = m2 - m1;

    /* 3. the quotients, 4. the ordered sums */
    if (r.status == 0) {
      /* lanes 0..4 divide for OQ, ClQ, SQ, QOQ and NAQ, one division for the five; the other lanes' 0/T is not used */
      const double Td = (double)T;
      const int num = lane == 0 ? r.close_o - r.open_o : lane == 1 ? r.close_o - m1 : lane == 2 ? m1 - r.open_o
                      : lane == 3 ? r.close_h - r.open_h : lane == 4 ? r.amp : 0;
      const double den = lane == 2 ? (double)(r.close_o - m1) : lane == 4 ? (double)r.decl * Td : Td;
      sum = sum + (double)num / den;
      n_acc++;
    } else {
      n_rej++;
    }
    /* 5. the cycle record */
    if (a.cycles && c - 1 < a.cycles_pitch && lane == 0) {
      vs_glottal_cycle w;
      w.peak = m1;
      w.period = T;
      w.trough = r.lo;
      w.amp = r.amp;
      w.open = r.open_o;
      w.close = r.close_o;
      w.open_mid = r.open_h;
      w.close_mid = r.close_h;
      w.gci = r.gci;
      w.decl = r.decl;
      w.status = r.status;
      w.reserved_ = 0;
      a.cycles[row * a.cycles_pitch + (c - 1)] = w;
    }
    m0 = m1;
    m1 = m2;
  }

  if (n_acc == 0) {
    if (lane == 0) {
      gl_record_empty(o, VS_GL_REJECTED | VS_GL_ALL_REJECTED);
      o->n_rejected = n_rej;
    }
    return;
  }
  if (lane < 5) (&o->oq)[lane] = sum / (double)n_acc; /* oq, clq, sq, qoq, naq lie in this order */
  if (lane != 0) return;
  o->n_cycles = n_acc;
  o->n_rejected = n_rej;
  o->status = n_rej ? VS_GL_REJECTED : 0;
  o->reserved_ = 0;
}

extern "C" hipError_t vs_launch_glottal(const VsGlArgs *args, hipStream_t stream)
{
  if (args->n_lanes <= 0 || args->n_lanes > 0x7FFFFFFFL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vs_glottal_kernel, dim3((unsigned)args->n_lanes), dim3(64), 0, stream, *args);
  return hipGetLastError();
}
