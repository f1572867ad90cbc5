/*
 * vs_track.hip -- gfx950 kernels of the coefficient tracks (include/voice_synth.h, "coefficient tracks"): the all-pole
 * filter of vowel_new.c:266-289 on int16 flow rows in HBM, with a coefficient set that changes along the row.
 *
 * One row per lane, 64-lane workgroups (one wavefront), templated on the arithmetic, the window class and the mode:
 *
 *   - The filter core restates vs_filter_wide_kernel (vs_filter_wide.hip): a rotating register window with static indices,
 *     24 doubles for orders up to 22 and 48 for 23..40, 16-byte loads and stores on whole groups of eight samples and a
 *     scalar tail.  The row is walked in passes of VS_TRACK_GROUP = 24 samples; the wide class alternates between the two
 *     halves of its window (a scalar branch), so a set may change every 24 samples in both classes and the step-up below
 *     is in the code once.
 *   - The taps live in VGPRs (P of them: the class's maximum).  Lower orders carry zeros in the missing taps:
 *     acc - 0*y == acc for finite y, and in the step-up a + 0*b == a for finite a, b (up to the sign of a zero tap, which
 *     cannot reach the int16 output), so padding changes no output bit as long as the state is finite -- the argument
 *     the header makes for vs_lane.order < 22.  The step-up skips the steps beyond `order` altogether (a scalar branch).
 *   - Which set: k = min((m - offset) / hop, K - 1) is followed without a division: the lane keeps the sample at which
 *     k + 1 begins (64-bit) and advances while m has reached it.  The advance is a loop under the lanes' own condition:
 *     the wavefront skips it when no lane needs a new set (rows of one call usually share hop and offset, so it is
 *     uniform in practice), and every lane gets its own k when they differ.
 *   - Every set is tested exactly once, in order, when the walk reaches it (the sets the row never reaches are tested
 *     behind the last sample, for n_unusable); an unusable set leaves the previous one in place (forward fill).
 *   - Hold: a usable set's taps are loaded into the VGPRs.
 *   - Glide: ka and kb (the reflection coefficients of E_k and E_{k+1}) live in LDS, [2][P][64] doubles (40 KB per
 *     workgroup at 23..40 taps, 22.5 KB up to 22): with the window and the taps in VGPRs there is no room for them in
 *     registers, and no per-thread array is indexed at run time (that would be scratch).  The step-down of set k + 2
 *     runs IN the slot that ka leaves when k advances (runtime loops over the actual order, in pairs (j, i - j) like the
 *     Levinson recursion of vs_lpc.hip); when it fails, kb is copied over it.  The step-up runs in the tap registers, fully
 *     unrolled, whenever (k, t) has changed.
 *
 * Per-row status goes into vs_track_stat; there is no device trap.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_track.h"

typedef uint32_t trk_u32x4 __attribute__((ext_vector_type(4), aligned(4))); /* 16 bytes of a PCM row: rows are only 4-byte aligned */

/* round2int() of vowel_new.c:413-427, as vs_round2int of vs_dev_primitives.h (the reasoning is there) */
__device__ __forceinline__ int trk_round2int(double x)
{
  const double dec = __builtin_amdgcn_fract(x);
  x = x + ((dec > 0.5) ? 1.0 : 0.0);
  const int v = (int)floor(x);
  return (v > 32767) ? 32767 : ((v < -32767) ? -32767 : v);
}

__device__ __forceinline__ bool trk_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

/* hold: A[1..p] (and the gain) finite */
__device__ __forceinline__ bool trk_set_finite(const double *__restrict__ c, int p, const double *__restrict__ g)
{
  bool ok = g ? trk_finite(*g) : true;
  for (int j = 1; j <= p; ++j) ok = ok && trk_finite(c[j]);
  return ok;
}

template <int P>
__device__ __forceinline__ void trk_load_taps(double (&a)[P + 1], const double *__restrict__ c, int p)
{
#pragma unroll
  for (int j = 1; j <= P; ++j) a[j] = (j <= p) ? c[j] : 0.0;
}

/* glide: the set's usability test and its step-down into the lane's LDS slot S (S[(i - 1) * 64] = k_i); the slot's
 * content is undefined after a failure */
__device__ __forceinline__ bool trk_step_down(double *S, const double *__restrict__ c, int p, const double *__restrict__ g)
{
  bool ok = g ? trk_finite(*g) : true;
  for (int j = 1; j <= p; ++j) {
    const double v = c[j];
    ok = ok && trk_finite(v);
    S[(j - 1) * VS_TRACK_LANES] = v;
  }
  for (int i = p; i >= 1 && ok; --i) {
    const double k = S[(i - 1) * VS_TRACK_LANES];
    if (!(fabs(k) < 1.0)) {
      ok = false;
      break;
    }
    const double d = 1.0 - k * k;
    for (int j = 1; 2 * j <= i && j < i; ++j) {
      const double aj = S[(j - 1) * VS_TRACK_LANES], aij = S[(i - j - 1) * VS_TRACK_LANES];
      if (2 * j == i) {
        S[(j - 1) * VS_TRACK_LANES] = (aj - k * aj) / d;
      } else {
        S[(j - 1) * VS_TRACK_LANES] = (aj - k * aij) / d;
        S[(i - j - 1) * VS_TRACK_LANES] = (aij - k * aj) / d;
      }
    }
  }
  return ok;
}

/* one pass of VS_TRACK_GROUP samples from sample m on window positions T0 .. T0 + 23 (the core of vs_filter_wide_kernel) */
template <int ARITH, int P, int SS, int T0>
__device__ __forceinline__ void trk_pass(const double (&a)[P + 1], double (&y)[SS], const int16_t *__restrict__ irow,
                                         int16_t *__restrict__ orow, int m, int len, bool vec, double gain, double G,
                                         double pre)
{
#pragma unroll
  for (int g = 0; g < VS_TRACK_GROUP / 8; ++g) {
    const int n0 = m + 8 * g;
    const bool whole = vec && (n0 + 8 <= len);
    int xin[8];
    if (whole) {
      const trk_u32x4 v = *(const trk_u32x4 *)(irow + n0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xin[2 * e] = (int)(int16_t)(v[e] & 0xFFFFu);
        xin[2 * e + 1] = (int)(int16_t)(v[e] >> 16);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) xin[k] = (n0 + k < len) ? (int)irow[n0 + k] : 0;
    }
    int outv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int t = T0 + 8 * g + k;
      /* (double)x * gain, then * G: G is 1.0 without per-set gains, and acc * 1.0 == acc */
      double acc = ((double)xin[k] * gain) * G;
      const double y1 = y[(t + SS - 1) % SS];
      if (ARITH == VS_ARITH_EXACT) {
#pragma unroll
        for (int j = 1; j <= P; ++j) acc = acc - a[j] * y[(t + SS - j) % SS];
      } else {
        double p0 = acc, p1 = -(a[2] * y[(t + SS - 2) % SS]);
#pragma unroll
        for (int j = 3; j <= P; ++j) {
          const double yj = y[(t + SS - j) % SS];
          if (j & 1) p0 = __builtin_fma(-a[j], yj, p0);
          else p1 = __builtin_fma(-a[j], yj, p1);
        }
        acc = __builtin_fma(-a[1], y1, p0 + p1);
      }
      const double o = (ARITH == VS_ARITH_EXACT) ? (acc - pre * y1) : __builtin_fma(-pre, y1, acc);
      outv[k] = trk_round2int(o); /* vowel_new.c:284 */
      y[t] = acc;                 /* the window rotates by renaming, vowel_new.c:287-289 */
      __builtin_amdgcn_sched_barrier(0);
    }
    if (whole) {
      trk_u32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ((uint32_t)outv[2 * e] & 0xFFFFu) | ((uint32_t)outv[2 * e + 1] << 16);
      *(trk_u32x4 *)(orow + n0) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (n0 + k < len) orow[n0 + k] = (int16_t)outv[k];
    }
  }
}

template <int ARITH, int P, int MODE>
__global__ void __launch_bounds__(VS_TRACK_LANES) vs_track_kernel(VsTrackArgs args)
{
  constexpr int SS = (P <= VS_TRACK_P0) ? VS_TRACK_GROUP : 2 * VS_TRACK_GROUP;
  extern __shared__ double trk_lds[]; /* glide: [2][P][64] */
  const int lane = (int)threadIdx.x;
  const long gl = (long)blockIdx.x * VS_TRACK_LANES + lane;
  if (gl >= args.n_lanes) return; /* (no barrier below) */
  const vs_track_row R = args.rows[gl];
  const int p = args.order, K = R.n_sets;
  int len = R.length;
  const long long hop = R.hop;
  const double gain = (double)R.gain, pre = (double)R.pre_emphasis;
  const double *__restrict__ cs = args.coefs + gl * args.sets_pitch * (long)(p + 1);
  const double *__restrict__ gs = args.gains ? args.gains + gl * args.sets_pitch : nullptr;
  const int16_t *__restrict__ irow = args.in + gl * args.in_pitch;
  int16_t *__restrict__ orow = args.out + gl * args.out_pitch;
  const bool vec = args.vec_ok != 0;
  const long cstride = p + 1;

  double a[P + 1];
  double y[SS];
#pragma unroll
  for (int j = 0; j <= P; ++j) a[j] = 0.0;
#pragma unroll
  for (int j = 0; j < SS; ++j) y[j] = 0.0; /* vowel_new.c:222-224 */
  double G = 1.0, ga = 1.0, gb = 1.0;
  int sa = 0; /* glide: the slot of ka; kb is in the other */
  double *const S0 = trk_lds + lane;
#define TRK_SLOT(s) (S0 + (long)(s) * (P * VS_TRACK_LANES))

  /* E_{-1}: the first usable set */
  int nt = 0, nun = 0; /* sets tested so far, unusable ones among them */
  bool have = false;
  while (nt < K && !have) {
    const double *c = cs + nt * cstride;
    const double *g = gs ? gs + nt : nullptr;
    if (MODE == VS_TRACK_HOLD) {
      have = trk_set_finite(c, p, g);
      if (have) {
        trk_load_taps<P>(a, c, p);
        if (g) G = *g;
      }
    } else {
      have = trk_step_down(TRK_SLOT(0), c, p, g);
      if (have && g) ga = *g;
    }
    if (!have) nun++;
    nt++;
  }
  if (!have) { /* VS_TRACK_NO_SET: zeros */
    for (int n = 0; n < len; ++n) orow[n] = 0;
    len = 0;
  }

  int kc = 0;                                  /* the k of the pass */
  long long nextb = (long long)R.offset + hop; /* the sample at which k = kc + 1 begins */
  /* glide: kb = the reflection coefficients of E_{kc+1} into the free slot; set kc + 1 is tested here if it has not been
   * (those up to the first usable set have: E_{kc+1} is E_kc then, as it is behind the last set) */
#define TRK_FILL_KB()                                            \
  {                                                              \
    const int cand = kc + 1;                                     \
    bool ok = false;                                             \
    if (cand < K && cand >= nt) {                                \
      const double *g = gs ? gs + cand : nullptr;                \
      nt = cand + 1;                                             \
      ok = trk_step_down(TRK_SLOT(sa ^ 1), cs + cand * cstride, p, g); \
      if (ok && g) gb = *g;                                      \
      if (!ok) nun++;                                            \
    }                                                            \
    if (!ok) {                                                   \
      const double *src = TRK_SLOT(sa);                          \
      double *dst = TRK_SLOT(sa ^ 1);                            \
      for (int i = 0; i < p; ++i) dst[i * VS_TRACK_LANES] = src[i * VS_TRACK_LANES]; \
      gb = ga;                                                   \
    }                                                            \
  }
  if (MODE == VS_TRACK_GLIDE && have) TRK_FILL_KB();

  int last_k = -1;
  double last_t = 0.0;
  int half = 0;
  for (int m = 0; m < len; m += VS_TRACK_GROUP) {
    while (kc < K - 1 && (long long)m >= nextb) { /* skipped by the wavefront when no lane's k moves */
      kc++;
      nextb += hop;
      if (MODE == VS_TRACK_HOLD) {
        if (kc >= nt) {
          const double *c = cs + kc * cstride;
          const double *g = gs ? gs + kc : nullptr;
          nt = kc + 1;
          if (trk_set_finite(c, p, g)) {
            trk_load_taps<P>(a, c, p);
            if (g) G = *g;
          } else {
            nun++;
          }
        }
      } else {
        sa ^= 1;
        ga = gb;
        TRK_FILL_KB();
      }
    }
    if (MODE == VS_TRACK_GLIDE) {
      double t = 0.0;
      if ((long long)m >= (long long)R.offset && kc < K - 1) t = (double)((long long)m - (nextb - hop)) / (double)hop;
      if (kc != last_k || t != last_t) {
        last_k = kc;
        last_t = t;
        const double *Ka = TRK_SLOT(sa), *Kb = TRK_SLOT(sa ^ 1);
#pragma unroll
        for (int i = 1; i <= P; ++i) {
          if (i <= p) { /* scalar: p is the call's */
            const double ka = Ka[(i - 1) * VS_TRACK_LANES], kb = Kb[(i - 1) * VS_TRACK_LANES];
            const double kap = ka + t * (kb - ka);
#pragma unroll
            for (int j = 1; 2 * j <= i; ++j) {
              if (j < i) {
                const double aj = a[j], aij = a[i - j];
                if (2 * j == i) {
                  a[j] = aj + kap * aj;
                } else {
                  a[j] = aj + kap * aij;
                  a[i - j] = aij + kap * aj;
                }
              }
            }
            a[i] = kap;
          }
        }
        G = ga + t * (gb - ga);
      }
    }
    if (SS == VS_TRACK_GROUP || half == 0) trk_pass<ARITH, P, SS, 0>(a, y, irow, orow, m, len, vec, gain, G, pre);
    else trk_pass<ARITH, P, SS, SS - VS_TRACK_GROUP>(a, y, irow, orow, m, len, vec, gain, G, pre);
    half ^= 1;
  }

  /* the sets the row did not reach: tested for n_unusable only (glide: in kb's slot, which nothing reads any more) */
  for (; nt < K; ++nt) {
    const double *c = cs + nt * cstride;
    const double *g = gs ? gs + nt : nullptr;
    const bool ok = (MODE == VS_TRACK_HOLD) ? trk_set_finite(c, p, g) : trk_step_down(TRK_SLOT(sa ^ 1), c, p, g);
    if (!ok) nun++;
  }
  if (args.stat) {
    vs_track_stat st;
    st.status = have ? 0 : VS_TRACK_NO_SET;
    st.n_unusable = nun;
    args.stat[gl] = st;
  }
#undef TRK_FILL_KB
#undef TRK_SLOT
}

template <int ARITH, int P>
static hipError_t trk_launch(int mode, const VsTrackArgs *args, unsigned grid, hipStream_t stream)
{
  if (mode == VS_TRACK_HOLD) {
    hipLaunchKernelGGL((vs_track_kernel<ARITH, P, VS_TRACK_HOLD>), dim3(grid), dim3(VS_TRACK_LANES), 0, stream, *args);
  } else {
    const size_t lds = (size_t)vs_track_lds_doubles(P) * sizeof(double);
    hipLaunchKernelGGL((vs_track_kernel<ARITH, P, VS_TRACK_GLIDE>), dim3(grid), dim3(VS_TRACK_LANES), lds, stream, *args);
  }
  return hipGetLastError();
}

extern "C" hipError_t vs_launch_track(int arith, int mode, const VsTrackArgs *args, hipStream_t stream)
{
  if (args->n_lanes <= 0) return hipSuccess;
  if (args->order < 1 || args->order > VS_MAX_ORDER || (mode != VS_TRACK_HOLD && mode != VS_TRACK_GLIDE))
    return hipErrorInvalidValue;
  const long blocks = (args->n_lanes + VS_TRACK_LANES - 1) / VS_TRACK_LANES;
  if (blocks > 0x7FFFFFFFL) return hipErrorInvalidValue;
  const bool wide = args->order > VS_TRACK_P0;
  /* (VS_ARITH_F32 as well: the track kernels have no single-precision form) */
  if (arith == VS_ARITH_EXACT)
    return wide ? trk_launch<VS_ARITH_EXACT, VS_TRACK_P1>(mode, args, (unsigned)blocks, stream)
                : trk_launch<VS_ARITH_EXACT, VS_TRACK_P0>(mode, args, (unsigned)blocks, stream);
  return wide ? trk_launch<VS_ARITH_FMA, VS_TRACK_P1>(mode, args, (unsigned)blocks, stream)
              : trk_launch<VS_ARITH_FMA, VS_TRACK_P0>(mode, args, (unsigned)blocks, stream);
}
